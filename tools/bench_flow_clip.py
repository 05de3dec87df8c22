"""developer: the per-frame motion calls against the whole-clip calls, in ONE process on the same resident frames, alternating.

    python tools/bench_flow_clip.py [--frames 256] [--reps 5] [--out FILE]

Three shapes: 100 corners on a 351x235 ROI of 1080p uint8 frames; 1 000 points on 256x256 (bench.py config F); rm_roi_mean against
rm_roi_mean_clip on the 1080p frames.  Per-frame form: rm_flow_step + rm_pca_reduce per frame, as bench.py's roi_flow / F legs run
it.  Clip form: one rm_flow_clip + one rm_pca_reduce_windows.  The outputs of both forms are asserted equal before anything is timed.
Prints one JSON line: ms per frame of both forms per shape (the median of the alternating repetitions)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LK = ((15, 15), 2, (3, 10, 0.03))
WINDOW = 128      # RespiratoryMonitor.measure_buffer_length


def flow_shape(be, torch, frames, roi, begin, reps):
    n = len(frames) - 1

    def loop():
        st = be.flow_state()
        be.flow_begin(st, frames[0], *roi, *begin)
        motion, vals, ngs = [], [], []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            mean, ng = be.flow_step(st, frames[i + 1], *roi, *LK)
            ngs.append(ng)
            if ng:
                motion.append([mean[0], mean[1]])
            if ng and len(motion) >= 2:
                vals.append(be.pca_reduce(np.array(motion[-WINDOW:], dtype=np.float32)))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, np.array(motion, np.float32), np.array(vals), np.array(ngs), be.flow_points(st, begin[0])

    def clip():
        st = be.flow_state()
        be.flow_begin(st, frames[0], *roi, *begin)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mean, ng = be.flow_clip(st, frames[1:], *roi, *LK)
        motion = mean[ng > 0]
        vals = be.pca_reduce_windows(motion, 1, WINDOW) if len(motion) >= 2 else np.empty(0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, motion, vals, ng, be.flow_points(st, begin[0])

    a, b = loop(), clip()          # warm-up of both forms, and the check
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), "the clip form differs from the per-frame loop"
    tl, tc = [], []
    for _ in range(reps):
        tl.append(loop()[0])
        tc.append(clip()[0])
    return {"frames": n, "points": int(a[3][0]), "points_at_end": int(a[3][-1]), "loop_ms_per_frame": statistics.median(tl) * 1e3,
            "clip_ms_per_frame": statistics.median(tc) * 1e3, "loop_ms_all": [t * 1e3 for t in tl], "clip_ms_all": [t * 1e3 for t in tc]}


def mean_shape(be, torch, frames, roi, reps):
    n = len(frames)

    def loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = np.array([be.roi_mean(frames[i], *roi) for i in range(n)])
        return (time.perf_counter() - t0) / n, out

    def clip():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = be.roi_mean_clip(frames, *roi)
        return (time.perf_counter() - t0) / n, out

    a, b = loop(), clip()
    assert np.array_equal(a[1], b[1]), "rm_roi_mean_clip differs from rm_roi_mean"
    tl, tc = [], []
    for _ in range(reps):
        tl.append(loop()[0])
        tc.append(clip()[0])
    return {"frames": n, "loop_ms_per_frame": statistics.median(tl) * 1e3, "clip_ms_per_frame": statistics.median(tc) * 1e3,
            "loop_ms_all": [t * 1e3 for t in tl], "clip_ms_all": [t * 1e3 for t in tc]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop-only", action="store_true", help="only the per-frame loops, untimed: the run to put under a kernel trace")
    a = ap.parse_args()
    import torch
    from respmon_amd import synth
    from respmon_amd.base import _Backend
    be = _Backend()
    N = a.frames
    shift = lambda t: (1.5 * np.sin(2 * np.pi * 0.4 * t / 30), 0.5 * np.sin(2 * np.pi * 0.4 * t / 30 + np.pi / 3))
    # 1080p uint8 frames whose 351x235 ROI holds a moving texture (the rest of the frame does not matter to the motion path)
    roi = (784, 422, 351, 235)
    render = synth.synth_texture(235, 351, seed=4321)
    big = torch.full((N + 1, 1080, 1920), 128, dtype=torch.uint8, device="cuda")
    for t in range(N + 1):
        big[t, roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]] = torch.from_numpy(render(*shift(t))).cuda()
    render = synth.synth_texture(256, 256, seed=4321)
    small = torch.from_numpy(np.stack([render(*shift(t)) for t in range(N + 1)])).cuda()
    if a.loop_only:
        for frames, r, begin in ((big, roi, (100, 0.3, 7, 7)), (small, (0, 0, 256, 256), (1000, 0.01, 3, 7))):
            st = be.flow_state()
            be.flow_begin(st, frames[0], *r, *begin)
            for i in range(N):
                be.flow_step(st, frames[i + 1], *r, *LK)
        return
    res = {"tool": "bench_flow_clip", "device": torch.cuda.get_device_name(0),
           "roi_351x235_100_corners": flow_shape(be, torch, big, roi, (100, 0.3, 7, 7), a.reps),
           "256x256_1000_points": flow_shape(be, torch, small, (0, 0, 256, 256), (1000, 0.01, 3, 7), a.reps),
           "roi_mean_351x235": mean_shape(be, torch, big[1:], roi, a.reps)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
