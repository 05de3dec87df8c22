"""developer: the rate map (respmon_amd/rate.py, rm_rate_map / rm_window_rate_map / rm_spectral_peak) beside the pass it cannot avoid,
rm_shard_pyramid alone on the same buffer (frames -> Gaussian level), in ONE process, alternating.

    python tools/bench_rate_map.py [--reps 9] [--levels 4,2] [--dtypes uint8,float64] [--out profiles/rate_map.json]

1080p x 256 frames, 10 fps, band 0.1 - 1.0 Hz, nfreq 64.  For each level (4: 68 x 120 = 8 160 pixels, the K-split form; 2: 270 x 480 =
129 600 pixels, the wide form) and frame dtype:
  pyramid_ms           rm_shard_pyramid of the resident buffer (pyramid_levels 9 / skip 4, resp. 4 / 2: its rows are the Gaussian level)
  rate_map_ms          rm_rate_map of the resident buffer: that pass plus the spectral peak
  peak_ms              rm_spectral_peak alone on the [T, NP] level array
  window_rate_map_ms   rm_window_rate_map from a full, wrapped ring (head != 0: the RING variants); the pyramid pass was paid at push time
The ring ends holding the frames of the resident buffer: the buffer's map, the ring's map and rm_spectral_peak of the level array are
asserted equal, bit for bit, before anything is timed.  Prints one JSON line; medians of the alternating
repetitions, every repetition kept beside them.  No threshold is set on these figures: they are recorded."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, H, W, FPS, FMIN, FMAX, NFREQ = 256, 1080, 1920, 10.0, 0.1, 1.0, 64
PYRAMID = {4: (9, 4), 2: (4, 2)}      # level -> (pyramid_levels, skip_levels_at_top) whose rm_shard_pyramid rows are that level


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--levels", default="4,2")
    ap.add_argument("--dtypes", default="uint8,float64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from respmon_amd import _capi, device, rate, synth, transforms
    from respmon_amd.window import SlidingCalibration
    lib = _capi.load()
    extra = 48                                           # frames pushed beyond the first fill: the ring ends wrapped
    vid = synth.synth_breathing_blocks(T + extra, H, W, seed=1234, workers=16)
    res = {"tool": "bench_rate_map", "device": torch.cuda.get_device_name(0), "reps": a.reps, "T": T, "shape": [H, W], "fps": FPS,
           "band": [FMIN, FMAX], "nfreq": NFREQ, "runs": []}
    for dt in a.dtypes.split(","):
        stream = torch.from_numpy(vid).cuda()
        if dt == "float64":
            stream = stream.double() * (1. / 255)
        resident = stream[extra:T + extra].contiguous()
        for level in (int(v) for v in a.levels.split(",")):
            L, S = PYRAMID[level]
            h, w = rate.level_shape(H, W, level)
            NP = ctypes.c_size_t()
            _capi.check(lib, lib.rm_shard_layout_flags(H, W, L, S, 0, ctypes.byref(NP)), "rm_shard_layout_flags")
            assert NP.value == h * w, "the rows of rm_shard_pyramid are not the Gaussian level here"
            g = torch.empty((T, h * w), dtype=torch.float64, device="cuda")

            def pyramid():
                _capi.check(lib, lib.rm_shard_pyramid(device.ctx(), device.ptr(resident), device.buffer_dtype_code(resident), T, H, W, L, S, 0,
                                                      device.ptr(g), device.stream_ptr()), "rm_shard_pyramid")
            buffer_map = lambda: rate.buffer_rate_map(resident, FPS, FMIN, FMAX, level, NFREQ)
            peak = lambda: transforms.spectral_peak(g, FPS, FMIN, FMAX, NFREQ)
            win = SlidingCalibration(T, H, W, L, S)
            win.push(stream[:T])
            for k in range(T, T + extra, 16):
                win.push(stream[k:k + 16])
            assert win.count == T and win.head == extra % T != 0
            ring_map = lambda: win.rate_map(FPS, FMIN, FMAX, NFREQ)
            pyramid()
            m_buf, m_peak, m_ring = buffer_map(), peak(), ring_map()
            for u, v in zip((m_buf.freq, m_buf.power, m_buf.total), m_peak[:3]):
                assert torch.equal(torch.nan_to_num(u.reshape(-1), nan=-1.0), torch.nan_to_num(v, nan=-1.0))
            assert torch.equal(m_buf.index.reshape(-1), m_peak.index) and torch.equal(m_ring.index, m_buf.index)   # (the ring holds the same frames)
            t = {"pyramid_ms": [], "rate_map_ms": [], "peak_ms": [], "window_rate_map_ms": []}
            for i in range(a.reps):
                t["pyramid_ms"].append(timed(torch, pyramid)[0])
                t["rate_map_ms"].append(timed(torch, buffer_map)[0])
                t["peak_ms"].append(timed(torch, peak)[0])
                t["window_rate_map_ms"].append(timed(torch, ring_map)[0])
            run = {"dtype": dt, "level": level, "pixels": h * w, "moving_pixels": int((m_buf.index >= 0).sum())}
            for k, v in t.items():
                run[k] = statistics.median(v)
                run[k + "_all"] = v
            res["runs"].append(run)
            win.close()
            del g, win
        del stream, resident
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
