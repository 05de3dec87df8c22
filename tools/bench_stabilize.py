"""developer: camera stabilisation (rm_stab_push) per frame at 1080p, in pushes of 16 frames, for uint8 gray and for BGR frames, with
the estimate and the warp timed separately, beside rm_window_push and rm_stream_push on the same resident frames, in ONE process,
alternating.

    python tools/bench_stabilize.py [--frames 64] [--push 16] [--reps 5] [--out FILE]
    python tools/bench_stabilize.py --section similarity [--out profiles/stabilize_similarity.json]

Forms: `push` (rm_stab_push: estimate + warp), `estimate` (rm_stab_push with out_dev NULL), `warp` (rm_warp_shift with the shifts the
push reported), each for uint8 and BGR, at the defaults (levels (3, 0), 2 iterations, max_shift 8).  The frames are synth_texture
moved by a known +-3 px; the reported shifts are asserted against the truth, and push == warp(estimate) bit for bit, before anything
is timed.  Prints one JSON line: ms per frame (the median of the alternating repetitions), and the bytes model of every kernel at this
size.

Section `similarity`: the similarity model (rm_stab_sim_push, estimate only, rm_warp_similarity) at its defaults (levels (3, 0),
level_linear 1, 2 iterations, max_shift 8, max_linear 0.03) on frames rolled by +-0.15 degrees, zoomed by +-0.2 % and moved by +-3 px,
for uint8 and BGR, timed beside rm_stab_push on the same frames in the same process, alternating; the reported parameters are asserted
against the truth (the four frame corners) and push == warp(estimate) bit for bit before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bytes_model(H, W, lc, lf, iters, in_bytes, out_bytes):
    """HBM bytes per frame of every kernel, as launched: what it must read and write once (the taps of a tile come from cache)"""
    px = [((H + (1 << l) - 1) >> l) * ((W + (1 << l) - 1) >> l) for l in range(lc + 1)]
    m = {"k_stab_gray": px[0] * (in_bytes + 8),
         "k_stab_down": sum(8 * (px[l - 1] + px[l]) for l in range(1, lc + 1)),
         "k_stab_resid": sum(iters * 16 * px[l] for l in range(lf, lc + 1)),     # F_l and R_l once each per iteration
         "k_stab_warp": px[0] * (in_bytes + out_bytes)}
    m["estimate"] = m["k_stab_gray"] + m["k_stab_down"] + m["k_stab_resid"]
    m["push"] = m["estimate"] + m["k_stab_warp"]
    return m


def bytes_model_similarity(H, W, lc, lf, iters, in_bytes, out_bytes):
    """the same level bytes as the shift model: k_stab_resid_sim reads F_l and R_l once per iteration like k_stab_resid (its taps are
    gathered along a slightly rotated row, still from the rows a tile holds in cache); what grows is the float64 arithmetic per pixel"""
    m = bytes_model(H, W, lc, lf, iters, in_bytes, out_bytes)
    m["k_stab_resid(_sim)"] = m.pop("k_stab_resid")
    m["k_stab_warp_sim"] = m.pop("k_stab_warp")
    return m


def similarity_section(a):
    import torch
    from respmon_amd import synth
    from respmon_amd.stabilize import Stabilizer
    H, W, N, P = 1080, 1920, a.frames, a.push
    rng = np.random.Generator(np.random.PCG64(12))
    true_p = synth.similarity_params(rng.uniform(-0.15, 0.15, P), rng.uniform(0.998, 1.002, P), rng.uniform(-3.0, 3.0, P), rng.uniform(-3.0, 3.0, P))
    true_p[0] = 0.0
    render = synth.synth_texture(H, W, seed=4321)
    distinct = torch.stack([torch.from_numpy(render.at(*synth.similarity_scene_coords(H, W, p))) for p in true_p]).cuda()
    gray = distinct[torch.arange(N) % P].contiguous()
    true = true_p[np.arange(N) % P]
    bgr = torch.stack([gray, torch.roll(gray, 3, dims=2), 255 - gray], dim=-1).contiguous()
    src = {"u8": gray, "bgr": bgr}
    st = {(m, k): Stabilizer(H, W, model=m) for m in ("shift", "similarity") for k in ("u8", "bgr")}
    params = {}

    def corners(p):
        cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
        u, v = np.array([-cx, cx, -cx, cx]), np.array([-cy, -cy, cy, cy])
        return np.stack([cx + (1 + p[:, :1]) * u - p[:, 1:2] * v + p[:, 2:3], cy + p[:, 1:2] * u + (1 + p[:, :1]) * v + p[:, 3:4]], axis=-1)

    def push(model, kind):
        s = st[model, kind]
        s.reset()
        outs = [s.push(src[kind][k:k + P]) for k in range(0, N, P)]
        return torch.cat([o[0] for o in outs]), np.concatenate([o[1] for o in outs]), np.concatenate([o[2] for o in outs])

    def estimate(model, kind):
        s = st[model, kind]
        s.reset()
        outs = [s.estimate(src[kind][k:k + P]) for k in range(0, N, P)]
        return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])

    def warp(model, kind):
        return torch.cat([st[model, kind].warp(src[kind][k:k + P], params[kind][k:k + P]) for k in range(0, N, P)])

    res = {"tool": "bench_stabilize", "section": "similarity", "device": torch.cuda.get_device_name(0), "frames": N, "push": P, "H": H, "W": W,
           "levels": [3, 0], "level_linear": 1, "iterations": 2, "max_shift": 8.0, "max_linear": 0.03, "roll_deg": 0.15, "zoom": 0.002, "shift_px": 3.0}
    forms = {}
    for kind in ("u8", "bgr"):
        out, par, fl = push("similarity", kind)
        params[kind] = par
        est = estimate("similarity", kind)
        err = float(np.abs(corners(par) - corners(true)).max())
        sh = push("shift", kind)[1]
        err_shift = float(np.abs(corners(np.concatenate([np.zeros((N, 2)), sh], axis=1)) - corners(true)).max())
        assert not fl.any() and err < 0.25, "the estimate puts a corner %.3f px off the truth (%s)" % (err, kind)
        assert np.array_equal(est[0], par) and np.array_equal(est[1], fl), "estimate-only differs from the push (%s)" % kind
        assert torch.equal(warp("similarity", kind), out), "push differs from warp(estimate) (%s)" % kind
        res["max_corner_error_px_" + kind] = err
        res["max_corner_error_px_shift_model_" + kind] = err_shift
        forms["stab_push_%s" % kind] = lambda kind=kind: push("shift", kind)
        for name, fn in (("push", push), ("estimate", estimate), ("warp", warp)):
            forms["stab_sim_%s_%s" % (name, kind)] = lambda fn=fn, kind=kind: fn("similarity", kind)
    times = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            times[k].append(timed(torch, fn)[0] / N * 1e3)
    for k, v in times.items():
        res[k + "_ms_per_frame"] = statistics.median(v)
        res[k + "_ms_all"] = v
    res["bytes_per_frame_u8"] = bytes_model_similarity(H, W, 3, 0, 2, 1, 1)
    res["bytes_per_frame_bgr"] = bytes_model_similarity(H, W, 3, 0, 2, 3, 3)
    return res


def emit(a, res):
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("shift", "similarity"), default="shift")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--push", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.section == "similarity":
        return emit(a, similarity_section(a))
    import torch
    from scipy.signal import sosfilt_zi  # noqa: F401  (LiveMagnifier needs scipy: fail here, not in the timed region)
    from respmon_amd import synth
    from respmon_amd.live import LiveMagnifier
    from respmon_amd.stabilize import Stabilizer
    from respmon_amd.window import SlidingCalibration
    H, W, N, P = 1080, 1920, a.frames, a.push
    rng = np.random.Generator(np.random.PCG64(11))
    # one push worth of distinct frames (the numpy render of a 1080p texture takes about a second), repeated: every push sees the same
    # P frames, the first of them unmoved
    moves = rng.uniform(-3.0, 3.0, size=(P, 2))
    moves[0] = 0.0
    render = synth.synth_texture(H, W, seed=4321)
    distinct = torch.stack([torch.from_numpy(render(*m)) for m in moves]).cuda()
    gray = distinct[torch.arange(N) % P].contiguous()
    true = moves[np.arange(N) % P]
    bgr = torch.stack([gray, torch.roll(gray, 3, dims=2), 255 - gray], dim=-1).contiguous()

    st = {"u8": Stabilizer(H, W), "bgr": Stabilizer(H, W)}
    src = {"u8": gray, "bgr": bgr}
    shifts = {}

    def push(kind):
        s = st[kind]
        s.reset()
        outs = [s.push(src[kind][k:k + P]) for k in range(0, N, P)]
        return torch.cat([o[0] for o in outs]), np.concatenate([o[1] for o in outs]), np.concatenate([o[2] for o in outs])

    def estimate(kind):
        s = st[kind]
        s.reset()
        outs = [s.estimate(src[kind][k:k + P]) for k in range(0, N, P)]
        return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])

    def warp(kind):
        return torch.cat([st[kind].warp(src[kind][k:k + P], shifts[kind][k:k + P]) for k in range(0, N, P)])

    win = SlidingCalibration(256, H, W)
    live = LiveMagnifier(H, W, 30.0)

    def window_push():
        for k in range(0, N, P):
            win.push(gray[k:k + P])

    def stream_push():
        return [live.push(gray[k:k + P]) for k in range(0, N, P)]

    res = {"tool": "bench_stabilize", "device": torch.cuda.get_device_name(0), "frames": N, "push": P, "H": H, "W": W,
           "levels": [3, 0], "iterations": 2, "max_shift": 8.0}
    forms = {}
    for kind in ("u8", "bgr"):
        out, sh, fl = push(kind)
        shifts[kind] = sh
        est = estimate(kind)
        err = float(np.abs(sh - true).max())
        assert not fl.any() and err < 0.05, "the estimate is off the true shift by %.3f px (%s)" % (err, kind)
        assert np.array_equal(est[0], sh) and np.array_equal(est[1], fl), "estimate-only differs from the push (%s)" % kind
        assert torch.equal(warp(kind), out), "push differs from warp(estimate) (%s)" % kind
        res["max_error_px_" + kind] = err
        for name, fn in (("push", push), ("estimate", estimate), ("warp", warp)):
            forms["stab_%s_%s" % (name, kind)] = lambda fn=fn, kind=kind: fn(kind)
    window_push(); stream_push()
    forms["window_push_u8"] = window_push
    forms["stream_push_u8"] = stream_push
    times = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            times[k].append(timed(torch, fn)[0] / N * 1e3)
    for k, v in times.items():
        res[k + "_ms_per_frame"] = statistics.median(v)
        res[k + "_ms_all"] = v
    res["bytes_per_frame_u8"] = bytes_model(H, W, 3, 0, 2, 1, 1)
    res["bytes_per_frame_bgr"] = bytes_model(H, W, 3, 0, 2, 3, 3)
    emit(a, res)


if __name__ == "__main__":
    main()
