"""developer: several subjects per frame against the one-subject calls they replace, in ONE process on the same resident buffer,
alternating.

    python tools/bench_subjects.py [--frames 128] [--reps 7] [--out profiles/subjects.json]

1080p uint8, N = 128 frames, K = 1, 4, 16 subjects with 351x235 ROIs:
  roi_mean  one rm_roi_mean_multi_clip call against K rm_roi_mean_clip calls (outputs asserted equal before anything is timed)
  locate    rm_locate_multi(max_rois = K) against rm_locate on a buffer with sixteen breathing blobs (entry 0 asserted equal)
  flow      one rm_flow_multi_clip + one rm_pca_reduce_windows_multi against K rm_flow_clip + K rm_pca_reduce_windows, 100 corners per
            subject on textured frames, K fresh states per repetition (begun outside the timed part; outputs asserted equal first).
            rm_flow_clip and rm_pca_reduce_windows are the K = 1 entries of the code behind the multi calls, so at K = 1 both forms
            time one code path against itself (a check of the noise, not a comparison); K = 4 and K = 16 compare one call with K.
Prints one JSON line: milliseconds per call of both forms (the median of the alternating repetitions).  No threshold is set on
these figures: they are recorded."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 4, 16)
ROI_W, ROI_H = 351, 235


def rois_for(K, H, W):
    """K rectangles of ROI_W x ROI_H on a grid over the frame (they overlap from K = 16 on: 4 x 4 of them on 1080p)"""
    nx = int(np.ceil(np.sqrt(K)))
    ny = (K + nx - 1) // nx
    out = []
    for k in range(K):
        i, j = k % nx, k // nx
        out.append((int(round(i * (W - ROI_W) / max(nx - 1, 1))), int(round(j * (H - ROI_H) / max(ny - 1, 1))), ROI_W, ROI_H))
    return out


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def flow_section(a, torch, be, res):
    from respmon_amd import synth
    N, H, W = a.frames, 1080, 1920
    render = synth.synth_texture(H, W, seed=4321)
    tex = torch.from_numpy(np.stack([render(1.5 * np.sin(2 * np.pi * 0.4 * t / 30), 0.5 * np.sin(2 * np.pi * 0.4 * t / 30 + np.pi / 3))
                                     for t in range(N + 1)])).cuda()
    lk = dict(winSize=(15, 15), maxLevel=2, criteria=(3, 10, 0.03))
    window = 128
    for K in KS:
        rois = rois_for(K, H, W)

        def begin():
            states = [be.flow_state() for _ in rois]
            npts = [len(be.flow_begin(st, tex[0], *r, 100, 0.3, 7, 7)) for st, r in zip(states, rois)]
            return states, npts

        def multi(states):
            mean, ng = be.flow_multi_clip(states, tex[1:], rois, **lk)
            assert (ng > 0).all()
            return mean, ng, be.pca_reduce_windows_multi([mean[:, k] for k in range(K)], [0] * K, window)

        def loop(states):
            out = [be.flow_clip(st, tex[1:], *r, **lk) for st, r in zip(states, rois)]
            return (np.stack([m for m, _ in out], axis=1), np.stack([n for _, n in out], axis=1),
                    [be.pca_reduce_windows(m, 0, window) for m, _ in out])

        (sm, npts), (sl, _) = begin(), begin()
        gm, gl = multi(sm), loop(sl)
        assert np.array_equal(gm[0], gl[0]) and np.array_equal(gm[1], gl[1]), "rm_flow_multi_clip differs from rm_flow_clip"
        assert all(np.array_equal(x, y) for x, y in zip(gm[2], gl[2])), "rm_pca_reduce_windows_multi differs from rm_pca_reduce_windows"
        tm, tl = [], []
        for _ in range(a.reps):
            sl, _ = begin()
            tl.append(timed(torch, lambda: loop(sl))[0])
            sm, _ = begin()
            tm.append(timed(torch, lambda: multi(sm))[0])
        res["flow"]["K%d" % K] = {"points": npts, "multi_ms": statistics.median(tm), "k_calls_ms": statistics.median(tl), "multi_ms_all": tm,
                                  "k_calls_ms_all": tl}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from respmon_amd import synth
    from respmon_amd.base import _Backend
    be = _Backend()
    N, H, W = a.frames, 1080, 1920
    centers = [((j + 0.5) / 4, (i + 0.5) / 4) for j in range(4) for i in range(4)]
    vid = synth.synth_breathing_dense(N, H, W, seed=4321, noise=0.02, centers=centers, sigma=(0.05, 0.04), phase_step=0.0, workers=16)
    frames = torch.from_numpy(vid).cuda()
    res = {"tool": "bench_subjects", "device": torch.cuda.get_device_name(0), "frames": N, "shape": [H, W], "roi": [ROI_W, ROI_H],
           "roi_mean": {}, "locate": {}, "flow": {}}
    for K in KS:
        rois = rois_for(K, H, W)
        multi = lambda: be.roi_mean_multi_clip(frames, rois)
        loop = lambda: np.stack([be.roi_mean_clip(frames, *r) for r in rois], axis=1)
        assert np.array_equal(multi(), loop()), "rm_roi_mean_multi_clip differs from rm_roi_mean_clip"
        tm, tl = [], []
        for _ in range(a.reps):
            tl.append(timed(torch, loop)[0])
            tm.append(timed(torch, multi)[0])
        res["roi_mean"]["K%d" % K] = {"multi_ms": statistics.median(tm), "k_calls_ms": statistics.median(tl), "multi_ms_all": tm, "k_calls_ms_all": tl}
    one = lambda: be.locate(frames, 10, 0.1, 1.0, 500, 9, 4, 0.7, 20)
    for K in KS:
        many = lambda: be.locate_multi(frames, 10, max_rois=K)
        r1, rk = one(), many()
        assert (rk[0] if rk else None) == r1, "entry 0 of rm_locate_multi differs from rm_locate"
        tm, tl = [], []
        for _ in range(a.reps):
            tl.append(timed(torch, one)[0])
            tm.append(timed(torch, many)[0])
        res["locate"]["K%d" % K] = {"rois_found": len(rk), "multi_ms": statistics.median(tm), "single_ms": statistics.median(tl),
                                    "multi_ms_all": tm, "single_ms_all": tl}
    flow_section(a, torch, be, res)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
