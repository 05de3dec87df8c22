"""developer: the pulse path (respmon_amd/pulse.py, rm_bgr_block_sums / rm_pulse_pos / rm_pulse_map) beside a plain stream of the same
bytes (rm_bgr_to_gray) and the rate map of the same buffer (rm_rate_map at level 4), in ONE process, alternating.

    python tools/bench_pulse.py [--reps 9] [--inner 10] [--frames 256] [--out profiles/pulse.json]

1080p x 256 frames 'bgr8' (1.59 GB: larger than the Infinity Cache), 20 fps, block 16 (68 x 120 = 8 160 blocks), window 32, band
0.7 - 3.0 Hz, nfreq 64: the defaults of pulse.pulse_map.  Timed with device events around `inner` back-to-back calls:
  block_sums_ms   rm_bgr_block_sums of the resident buffer (bytes model: 3 N H W read, 12 N Hb Wb written)
  pos_ms          rm_pulse_pos on the [N, 8160, 3] sums
  pulse_map_ms    rm_pulse_map: those two and the spectral peak
  bgr_to_gray_ms  rm_bgr_to_gray over the same buffer (reads the same 3 N H W bytes, writes N H W)
  rate_map_ms     rm_rate_map of the same buffer at level 4
rm_pulse_map is asserted equal to its parts, and the sums to a torch reduction of the first frames, before anything is timed.  Prints
one JSON line: medians of the alternating repetitions, every repetition kept beside them, the block-sum pass as a fraction of the
rm_bgr_to_gray stream and of 6.3 TB/s.  No threshold is set on these figures: they are recorded."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, FPS, BLOCK, FMIN, FMAX, NFREQ = 1080, 1920, 20.0, 16, 0.7, 3.0, 64
STREAM_CEILING = 6.3e12      # achievable HBM streaming rate, bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from respmon_amd import _capi, device, pulse, rate, transforms
    lib = _capi.load()
    N = a.frames
    window = pulse.default_window(FPS)
    # a skin-coloured left half under a flickering lamp with sensor noise, made on the device (the host generator takes minutes at this size)
    g = torch.Generator(device="cuda").manual_seed(1234)
    base = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    base[:, :W // 2] = torch.tensor([110.0, 140.0, 200.0], device="cuda")
    base[:, W // 2:] = 120.0
    frames = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    for n in range(N):
        t = n / FPS
        pulse_term = 0.004 * torch.tensor([0.53, 0.77, 0.33], device="cuda") * math.sin(2 * math.pi * 1.25 * t)
        f = base * (1 + 0.02 * math.sin(2 * math.pi * 0.9 * t))
        f[:, :W // 2] *= 1 + pulse_term
        frames[n] = (f + torch.randn((H, W, 3), generator=g, device="cuda")).round().clamp(0, 255).to(torch.uint8)
    hb, wb = -(-H // BLOCK), -(-W // BLOCK)
    gray = torch.empty((N, H, W), dtype=torch.uint8, device="cuda")
    sums = pulse.block_sums(frames, BLOCK)
    few = min(N, 4)
    want = frames[:few].to(torch.int64)
    want = torch.nn.functional.pad(want, (0, 0, 0, wb * BLOCK - W, 0, hb * BLOCK - H)).reshape(few, hb, BLOCK, wb, BLOCK, 3).sum(dim=(2, 4))
    assert torch.equal(sums[:few].view(torch.int32).to(torch.int64), want), "block sums differ from a torch reduction"
    h = pulse.pos(sums, window)
    pm = pulse.pulse_map(frames, FPS, BLOCK, window, FMIN, FMAX, NFREQ)
    sp = transforms.spectral_peak(h, FPS, FMIN, FMAX, NFREQ)
    for u, v in zip((pm.freq, pm.power, pm.total), sp[:3]):
        assert torch.equal(torch.nan_to_num(u, nan=-1.0), torch.nan_to_num(v, nan=-1.0)), "rm_pulse_map differs from its parts"
    assert torch.equal(pm.index, sp.index)

    def to_gray():
        _capi.check(lib, lib.rm_bgr_to_gray(device.ctx(), device.ptr(frames), N * H * W, device.ptr(gray), device.stream_ptr()), "rm_bgr_to_gray")
    calls = {
        "block_sums_ms": lambda: pulse.block_sums(frames, BLOCK),
        "pos_ms": lambda: pulse.pos(sums, window),
        "pulse_map_ms": lambda: pulse.pulse_map(frames, FPS, BLOCK, window, FMIN, FMAX, NFREQ),
        "bgr_to_gray_ms": to_gray,
        "rate_map_ms": lambda: rate.buffer_rate_map(frames, FPS, 0.1, 1.0, 4, NFREQ),
    }
    for fn in calls.values():          # warm up every shape that is timed
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()       # (untimed: rm_pulse_map and rm_rate_map share the context's one cached spectral operator, and alternating evicts it)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / a.inner)
    res = {"tool": "bench_pulse", "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "N": N, "shape": [H, W], "fps": FPS,
           "block": BLOCK, "blocks": hb * wb, "window": window, "band": [FMIN, FMAX], "nfreq": NFREQ,
           "skin_blocks_within_a_step_of_1.25Hz": int(((pm.freq[:, :wb // 2] - 1.25).abs() <= (FMAX - FMIN) / (NFREQ - 1)).sum()),
           "skin_blocks": hb * (wb // 2)}
    for k, v in t.items():
        res[k] = statistics.median(v)
        res[k + "_all"] = v
    nbytes = 3 * N * H * W
    res["block_sums_bytes_model"] = nbytes
    res["block_sums_TBps"] = nbytes / (res["block_sums_ms"] * 1e-3) / 1e12
    res["block_sums_fraction_of_6.3TBps"] = nbytes / (res["block_sums_ms"] * 1e-3) / STREAM_CEILING
    res["bgr_to_gray_TBps_read"] = nbytes / (res["bgr_to_gray_ms"] * 1e-3) / 1e12
    res["block_sums_rate_over_bgr_to_gray_rate"] = res["bgr_to_gray_ms"] / res["block_sums_ms"]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
