"""developer: uint16 frame buffers (RM_U16) beside the float16 buffer -- the same bytes and the same chain geometry: the yardstick -- and the
uint8 buffer of the same shapes, in ONE process, the dtypes alternating inside every round (tools/ab_inproc.py's way).

    python tools/bench_u16.py [--reps 7] [--out profiles/u16.json] [--only NAME]

rm_locate at 1080p x 256 (pyramid_levels 9, skip 4) and 720p x 128 (4, 2): per dtype the median host milliseconds of the call (it ends in a
stream wait) and, from a second pass with rm_profile_enable(2), the frame-buffer kernel's own time (rm_profile_read phase 0).
rm_magnify uint16 -> uint16 at 1080p x 256 beside uint8 -> uint8, with GB/s on B_alg = T H W (s_in + s_out).
The two unpack forms of the uint16 chain are compared at kernel level by bench_micro/dc16_bench.hip (the library ships one of them).
The 16-bit video is synth_breathing in the upper byte with uniform noise in the lower (synth.synth_breathing16's model; the noise is
drawn on the device here); the float16 buffer holds the same picture rounded to half.  Prints one JSON line."""
import argparse
import ctypes
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="substring of the shape names to run")
    a = ap.parse_args()
    import numpy as np
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

    res = {"tool": "bench_u16", "device": torch.cuda.get_device_name(0), "peak_GBs": PEAK_GBS, "reps": a.reps,
           "kernel_source_sha": lib.rm_debug_kernel_source_stamp().decode(), "locate": {}, "magnify": {}}
    for name, T, H, W, L, S in SHAPES:
        if a.only and a.only not in name:
            continue
        u8 = torch.from_numpy(synth.synth_breathing(T, H, W, seed=11)).cuda()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(16)
        k = (u8.to(torch.int32) << 8) | torch.randint(0, 256, (T, H, W), device="cuda", generator=gen, dtype=torch.int32)
        u16 = k.to(torch.int16).view(torch.uint16)            # (the low 16 bits: int32 -> int16 wraps, the view reads them unsigned)
        f16 = (k.to(torch.float32) * (1.0 / 65535)).to(torch.float16)
        del k
        bufs = {"u16": (u16, _capi.RM_U16), "f16": (f16, _capi.RM_F16), "u8": (u8, _capi.RM_U8)}
        xywh = np.zeros(4, np.int32)
        sp = device.stream_ptr()

        def locate(key):
            buf, code = bufs[key]
            rc = _capi.check(lib, lib.rm_locate(ctx, device.ptr(buf), code, T, H, W, fps, fmin, fmax, amp, L, S, 0.7, 20, 0,
                                                ctypes.c_void_p(xywh.ctypes.data), sp), "rm_locate")
            return None if rc == _capi.RM_NO_CONTOUR else [int(v) for v in xywh]

        rois = {key: locate(key) for key in bufs}            # (warm-up of every dtype's kernels, and the answer)
        for key in bufs:
            locate(key)
        ms = {key: [] for key in bufs}
        for _ in range(a.reps):
            for key in bufs:
                ms[key].append(timed(lambda: locate(key)))
        kern = {key: [] for key in bufs}
        _capi.check(lib, lib.rm_profile_enable(ctx, 2), "rm_profile_enable")
        phases, n = (ctypes.c_double * 4)(), ctypes.c_int()
        for _ in range(a.reps):
            for key in bufs:
                locate(key)
                _capi.check(lib, lib.rm_profile_read(ctx, phases, ctypes.byref(n)), "rm_profile_read")
                kern[key].append(phases[0] / max(n.value, 1))
        _capi.check(lib, lib.rm_profile_enable(ctx, 0), "rm_profile_enable")
        row = {"T": T, "H": H, "W": W, "pyramid_levels": L, "skip_levels_at_top": S}
        for key, (buf, _) in bufs.items():
            nbytes = buf.numel() * buf.element_size()
            kms = statistics.median(kern[key])
            row[key] = {"roi": rois[key], "locate_ms": statistics.median(ms[key]), "locate_ms_all": ms[key],
                        "frame_buffer_kernel_ms": kms, "frame_buffer_kernel_ms_all": kern[key], "buffer_bytes": nbytes,
                        "kernel_GBs_on_buffer_bytes": nbytes / kms / 1e6, "fraction_of_peak": nbytes / kms / 1e6 / PEAK_GBS}
        row["u16_over_f16_locate"] = row["u16"]["locate_ms"] / row["f16"]["locate_ms"]
        row["u16_over_f16_kernel"] = row["u16"]["frame_buffer_kernel_ms"] / row["f16"]["frame_buffer_kernel_ms"]
        res["locate"][name] = row
        if T == 256:
            mag = {}
            outs = {"u16": torch.empty((T, H, W), dtype=torch.int16, device="cuda").view(torch.uint16), "u8": torch.empty_like(u8)}

            def magnify(key):
                buf, code = bufs[key]
                _capi.check(lib, lib.rm_magnify(ctx, device.ptr(buf), code, T, H, W, fps, fmin, fmax, amp, L, S, device.ptr(outs[key]), code, sp), "rm_magnify")

            for key in outs:
                magnify(key)
            tm = {key: [] for key in outs}
            for _ in range(a.reps):
                for key in outs:
                    tm[key].append(timed(lambda: magnify(key)))
            for key in outs:
                b_alg = 2 * bufs[key][0].numel() * bufs[key][0].element_size()
                m = statistics.median(tm[key])
                mag[key] = {"magnify_ms": m, "magnify_ms_all": tm[key], "B_alg_bytes": b_alg, "GBs_on_B_alg": b_alg / m / 1e6,
                            "fraction_of_peak": b_alg / m / 1e6 / PEAK_GBS}
            res["magnify"][name] = mag
            del outs
        del bufs, u8, u16, f16
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
