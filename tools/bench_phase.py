"""Time phase-based magnification (respmon_amd.live.PhaseMagnifier, rm_phase_push) on the GPU: ms per frame at 1080p in pushes of 16,
uint8 in -> uint8 out, pyramid_levels 5, at skip_levels_at_top 0 and 1, with LiveMagnifier (the linear method, same frames, same pushes)
beside it for scale.  Prints one JSON line.  The bytes model of the two new kernels, per frame:

    k_phase_time    NP * (8 read + 24 written) + NP * 2 * 8 * (5 + 4 nsec) / n        the level once, three planes, the state once per push
    k_phase_space   NP * (24 + 8 read + 8 written)                                    three planes and the level once, L' once

NP: pixels of the processed levels.  The share of each kernel in the time comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/bench_phase.py); the model's bytes over a kernel's traced time is its achieved bandwidth.

    python tools/bench_phase.py [--height 1080 --width 1920 --push 16 --pushes 8 --warmup 2 --order 1]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def processed_pixels(H, W, levels, skip):
    n = 0
    for l in range(levels):
        if skip <= l <= levels - 2:
            n += H * W
        H, W = (H + 1) // 2, (W + 1) // 2
    return n


def time_pushes(t, mag, chunks, warmup):
    for c in chunks[:warmup]:
        mag.push(c)
    t.cuda.synchronize()
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    for c in chunks[warmup:]:
        mag.push(c)
    b.record()
    t.cuda.synchronize()
    return a.elapsed_time(b) / sum(len(c) for c in chunks[warmup:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--push", type=int, default=16)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--order", type=int, default=1)
    ap.add_argument("--levels", type=int, default=5)
    a = ap.parse_args()
    import torch as t
    from respmon_amd import synth
    from respmon_amd.live import LiveMagnifier, PhaseMagnifier
    H, W, n = a.height, a.width, a.push
    clip = synth.synth_breathing(n, H, W, seed=3)                      # one push worth of frames, rolled along x from push to push
    chunks = [t.from_numpy(clip).cuda().roll(k, dims=2).contiguous() for k in range(a.warmup + a.pushes)]
    res = {"H": H, "W": W, "push": n, "pushes": a.pushes, "order": a.order, "pyramid_levels": a.levels}
    for skip in (0, 1):
        with PhaseMagnifier(H, W, 30.0, 0.1, 1.0, amplification=10, pyramid_levels=a.levels, skip_levels_at_top=skip, order=a.order) as pm:
            res["phase_skip%d_ms_per_frame" % skip] = round(time_pushes(t, pm, chunks, a.warmup), 4)
            res["phase_skip%d_state_MiB" % skip] = round(pm.state_bytes / 2 ** 20, 1)
        NP = processed_pixels(H, W, a.levels, skip)
        res["model_skip%d_time_kernel_MB_per_frame" % skip] = round(NP * (32 + 16 * (5 + 4 * a.order) / n) / 1e6, 2)
        res["model_skip%d_space_kernel_MB_per_frame" % skip] = round(NP * 40 / 1e6, 2)
        with PhaseMagnifier(H, W, 30.0, 0.1, 1.0, amplification=10, pyramid_levels=a.levels, skip_levels_at_top=skip, order=a.order, blur=False) as pm:
            res["phase_noblur_skip%d_ms_per_frame" % skip] = round(time_pushes(t, pm, chunks, a.warmup), 4)
    with LiveMagnifier(H, W, 30.0, 0.1, 1.0, amplification=10, pyramid_levels=a.levels, skip_levels_at_top=1, order=a.order) as lm:
        res["linear_skip1_ms_per_frame"] = round(time_pushes(t, lm, chunks, a.warmup), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
