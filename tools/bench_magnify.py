"""developer: rm_magnify (the magnified video in one fused pass) against the composition it replaces, in ONE process on the same resident
frame buffer, the two forms alternating.

    python tools/bench_magnify.py [--reps 5] [--out profiles/magnify.json] [--only NAME]

Composition (what a caller had to write before rm_magnify existed): rm_eulerian_magnification_bandpass with the raw output only (a [T,H,W]
float64 array, written level by level, mirrored, scanned for its extrema), then `frames.double() * (1./255) + raw` and the clamp / conversion
in torch.  Shapes: uint8 -> uint8 and float64 -> float64 at 1080p x 256 (pyramid_levels 9, skip 4) and 720p x 128 (4, 2).  The outputs of both
forms are asserted equal before anything is timed.  Per shape: the median milliseconds of both forms, the achieved GB/s of rm_magnify on
B_alg = T H W (s_in + s_out) and its fraction of 8 TB/s, and two floors measured in the same process: `convert_only_ms`, rm_magnify with nothing
filtered (skip >= levels - 1: the same bytes through k_magnify_plain, no front half, no evaluation), and `copy_ms`, a device copy that moves
twice the output bytes (B_alg when input and output are as wide).
A colour row per shape (`*_bgr`): rm_magnify_bgr on a [T,H,W,3] BGR buffer against ITS composition (the same raw, then the per-channel sum, clamp
and conversion in torch through [T,H,W,3] float64 temporaries), and against the gray rm_magnify (BGR8 -> RM_U8) on the same buffer in the same
rounds: `gray_ms`, `extra_ms_over_gray` = the colour call minus the gray one, and `extra_bytes_GBs` = the 2 T H W bytes the colour call writes
on top of the gray one over that difference.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0
SHAPES = [("1080p_x256_L9S4", 256, 1080, 1920, 9, 4), ("720p_x128_L4S2", 128, 720, 1280, 4, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    a = ap.parse_args()
    import torch
    from respmon_amd import _capi, device, synth
    lib = _capi.load()
    ctx = device.ctx()
    fps, fmin, fmax, amp = 10.0, 0.1, 1.0, 500.0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res = {"tool": "bench_magnify", "device": torch.cuda.get_device_name(0), "peak_GBs": PEAK_GBS, "reps": a.reps, "cases": {}}
    for name, T, H, W, L, S in SHAPES:
        u8 = torch.from_numpy(synth.synth_breathing(T, H, W, seed=11)).cuda()
        for dt, code in ((torch.uint8, _capi.RM_U8), (torch.float64, _capi.RM_F64)):
            case = "%s_%s" % (name, "u8" if dt == torch.uint8 else "f64")
            if a.only and a.only not in case:
                continue
            vid = u8 if dt == torch.uint8 else u8.double() * (1.0 / 255)
            out = torch.empty((T, H, W), dtype=dt, device="cuda")
            raw = torch.empty((T, H, W), dtype=torch.float64, device="cuda")
            sp = device.stream_ptr()

            def fused(levels=L, skip=S):
                _capi.check(lib, lib.rm_magnify(ctx, device.ptr(vid), code, T, H, W, fps, fmin, fmax, amp, levels, skip, device.ptr(out), code, sp),
                            "rm_magnify")

            def composed():
                _capi.check(lib, lib.rm_eulerian_magnification_bandpass(ctx, device.ptr(vid), code, T, H, W, fps, fmin, fmax, amp, L, S, 0.7, None,
                                                                        device.ptr(raw), None, sp), "bandpass")
                m = (vid.double() * (1.0 / 255) if dt == torch.uint8 else vid) + raw
                return (m.clamp_(0.0, 1.0) * 255).to(torch.uint8) if dt == torch.uint8 else m

            fused()
            ref = composed()
            assert torch.equal(out, ref), "rm_magnify differs from the composition"
            del ref
            tf, tc, tz, tcp = [], [], [], []
            half = torch.empty(out.numel() * out.element_size(), dtype=torch.uint8, device="cuda")
            for _ in range(a.reps):
                tf.append(timed(fused))
                tc.append(timed(composed))
                tz.append(timed(lambda: fused(2, 4)))
                tcp.append(timed(lambda: half.copy_(out.view(torch.uint8).reshape(-1))))
            b_alg = T * H * W * (vid.element_size() + out.element_size())
            ms = statistics.median(tf)
            res["cases"][case] = {"T": T, "H": H, "W": W, "pyramid_levels": L, "skip_levels_at_top": S, "B_alg_bytes": b_alg,
                                  "magnify_ms": ms, "composition_ms": statistics.median(tc), "speedup": statistics.median(tc) / ms,
                                  "magnify_GBs_on_B_alg": b_alg / ms / 1e6, "fraction_of_peak": b_alg / ms / 1e6 / PEAK_GBS,
                                  "convert_only_ms": statistics.median(tz), "copy_ms": statistics.median(tcp),
                                  "copy_bytes": 2 * half.numel(),
                                  "magnify_ms_all": tf, "composition_ms_all": tc}
            del out, raw, half, vid
            torch.cuda.empty_cache()
        case = "%s_bgr" % name
        if a.only and a.only not in case:
            continue
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        vid = (u8.unsqueeze(-1).to(torch.int16) + torch.randint(-20, 21, (T, H, W, 3), device="cuda", generator=gen, dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)
        out = torch.empty_like(vid)
        gray = torch.empty((T, H, W), dtype=torch.uint8, device="cuda")
        raw = torch.empty((T, H, W), dtype=torch.float64, device="cuda")
        sp = device.stream_ptr()

        def colour(levels=L, skip=S):
            _capi.check(lib, lib.rm_magnify_bgr(ctx, device.ptr(vid), T, H, W, fps, fmin, fmax, amp, levels, skip, device.ptr(out), sp), "rm_magnify_bgr")

        def gray_call():
            _capi.check(lib, lib.rm_magnify(ctx, device.ptr(vid), _capi.RM_BGR8, T, H, W, fps, fmin, fmax, amp, L, S, device.ptr(gray), _capi.RM_U8, sp), "rm_magnify")

        def composed_colour():
            _capi.check(lib, lib.rm_eulerian_magnification_bandpass(ctx, device.ptr(vid), _capi.RM_BGR8, T, H, W, fps, fmin, fmax, amp, L, S, 0.7, None,
                                                                    device.ptr(raw), None, sp), "bandpass")
            m = vid.double() * (1.0 / 255) + raw.unsqueeze(-1)
            return (m.clamp_(0.0, 1.0) * 255).to(torch.uint8)

        colour()
        ref = composed_colour()
        assert torch.equal(out, ref), "rm_magnify_bgr differs from the composition"
        del ref
        torch.cuda.empty_cache()
        tf, tc, tg, tz, tcp = [], [], [], [], []
        half = torch.empty(out.numel(), dtype=torch.uint8, device="cuda")
        for _ in range(a.reps):
            tf.append(timed(colour))
            tg.append(timed(gray_call))
            tc.append(timed(composed_colour))
            tz.append(timed(lambda: colour(2, 4)))
            tcp.append(timed(lambda: half.copy_(out.reshape(-1))))
        b_alg = 2 * vid.numel()
        ms, gms = statistics.median(tf), statistics.median(tg)
        extra = 2 * T * H * W
        res["cases"][case] = {"T": T, "H": H, "W": W, "pyramid_levels": L, "skip_levels_at_top": S, "B_alg_bytes": b_alg,
                              "magnify_bgr_ms": ms, "composition_ms": statistics.median(tc), "speedup": statistics.median(tc) / ms,
                              "magnify_bgr_GBs_on_B_alg": b_alg / ms / 1e6, "fraction_of_peak": b_alg / ms / 1e6 / PEAK_GBS,
                              "gray_ms": gms, "extra_ms_over_gray": ms - gms, "extra_bytes": extra,
                              "extra_bytes_GBs": (extra / (ms - gms) / 1e6) if ms > gms else None,
                              "convert_only_ms": statistics.median(tz), "copy_ms": statistics.median(tcp), "copy_bytes": 2 * half.numel(),
                              "magnify_bgr_ms_all": tf, "gray_ms_all": tg, "composition_ms_all": tc}
        del out, raw, half, vid, gray
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
