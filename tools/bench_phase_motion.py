"""developer: the 'phase' motion signal (rm_phase_motion_clip) per frame and per clip, beside the flow clip path and the ROI mean on the
same resident frames, in ONE process, alternating.

    python tools/bench_phase_motion.py [--frames 256] [--reps 5] [--out FILE]

The located 351x235 ROI of 1080p uint8 frames at pyramid levels 0, 1, 2.  Clip form: one rm_phase_motion_clip + one
rm_pca_reduce_windows.  Per-frame form: one rm_phase_motion_clip of N == 1 + one rm_pca_reduce per frame, as extract_motion('phase')
runs it.  K = 4 subjects: four 351x235 rectangles in one rm_phase_motion_multi_clip + one rm_pca_reduce_windows_multi, per frame of
the clip (all four subjects together).  Beside them rm_flow_clip + rm_pca_reduce_windows (100 corners) and rm_roi_mean_clip on the same
clip.  The outputs of the forms are asserted equal before anything is timed.  Prints one JSON line: ms per frame (the median of the
alternating repetitions)."""
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


def rows_of(sums):
    s = sums[sums[:, 0] > 0]
    return np.stack([s[:, 1] / s[:, 0], s[:, 2] / s[:, 0]], axis=1).astype(np.float32)


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from respmon_amd import synth
    from respmon_amd.base import _Backend
    be = _Backend()
    N = a.frames
    shift = lambda t: (0.4 * np.sin(2 * np.pi * 0.4 * t / 30), 0.15 * np.sin(2 * np.pi * 0.4 * t / 30 + np.pi / 3))
    roi = (784, 422, 351, 235)
    x, y, w, h = roi
    render = synth.synth_texture(h, w, seed=4321)
    frames = torch.full((N, 1080, 1920), 128, dtype=torch.uint8, device="cuda")
    rois4 = [roi, (100, 100, w, h), (1300, 700, w, h), (1500, 50, w, h)]       # disjoint: every subject sees the moving texture
    for t in range(N):
        tex = torch.from_numpy(render(*shift(t))).cuda()
        for rx, ry, _, _ in rois4:
            frames[t, ry:ry + h, rx:rx + w] = tex

    one = {level: be.phase_motion_state(w, h, level) for level in (0, 1, 2)}       # the sessions live outside the timed region
    four = {level: [be.phase_motion_state(w, h, level) for _ in rois4] for level in (0, 1, 2)}

    def phase_clip(level):
        st = one[level]
        st.reset()
        sums = be.phase_motion_clip(st, frames, x, y)
        rows = rows_of(sums[1:])
        return sums, be.pca_reduce_windows(rows, 1, WINDOW)

    def phase_loop(level):
        st = one[level]
        st.reset()
        sums, rows, vals = [], [], []
        for i in range(N):
            s = be.phase_motion_clip(st, frames[i:i + 1], x, y)[0]
            sums.append(s)
            if i and s[0] > 0:
                rows.append([np.float32(s[1] / s[0]), np.float32(s[2] / s[0])])
                if len(rows) >= 2:
                    vals.append(be.pca_reduce(np.array(rows[-WINDOW:], dtype=np.float32)))
        return np.array(sums), np.array(vals)

    def phase_multi(level):
        sts = four[level]
        for st in sts:
            st.reset()
        sums = be.phase_motion_multi_clip(sts, frames, rois4)
        rows = [rows_of(sums[1:, k]) for k in range(4)]
        return sums, be.pca_reduce_windows_multi(rows, [1] * 4, WINDOW)

    def flow_clip():
        st = be.flow_state()
        be.flow_begin(st, frames[0], *roi, 100, 0.3, 7, 7)
        mean, ng = be.flow_clip(st, frames[1:], *roi, *LK)
        motion = mean[ng > 0]
        return be.pca_reduce_windows(motion, 1, WINDOW) if len(motion) >= 2 else np.empty(0)

    def mean_clip():
        return be.roi_mean_clip(frames, *roi)

    res = {"tool": "bench_phase_motion", "device": torch.cuda.get_device_name(0), "frames": N, "roi": list(roi)}
    forms = {}
    for level in (0, 1, 2):
        c, l, m = phase_clip(level), phase_loop(level), phase_multi(level)      # warm-up of the forms, and the check
        assert np.array_equal(c[0], l[0]) and np.array_equal(c[1], l[1]), "the clip form differs from the per-frame loop"
        assert np.array_equal(m[0][:, 0], c[0]) and np.array_equal(m[1][0], c[1]), "the multi form differs from the clip form"
        forms["phase_clip_level%d" % level] = lambda level=level: phase_clip(level)
        forms["phase_loop_level%d" % level] = lambda level=level: phase_loop(level)
        forms["phase_multi4_level%d" % level] = lambda level=level: phase_multi(level)
    flow_clip(); mean_clip()
    forms["flow_clip_100_corners"] = flow_clip
    forms["roi_mean_clip"] = mean_clip
    times = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            times[k].append(timed(torch, fn)[0] / N * 1e3)
    for k, v in times.items():
        res[k + "_ms_per_frame"] = statistics.median(v)
        res[k + "_ms_all"] = v
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
