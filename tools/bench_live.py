"""developer: the live magnifier (respmon_amd/live.py, rm_stream_push) against the two ways to get a live view without it, in ONE process.

    python tools/bench_live.py [--reps 9] [--configs A,B,C,D] [--out profiles/live_magnify.json]

  A   1080p, pyramid_levels 9 / skip 4, uint8 -> uint8
  B   1080p, pyramid_levels 9 / skip 4, float64 -> float64
  C   720p, pyramid_levels 4 / skip 2, uint8 -> uint8
  D   1080p, pyramid_levels 9 / skip 4, BGR -> BGR
For each, after a warm-up that fills the filter state:
  push_n1_ms_per_frame / push_n16_ms_per_frame    LiveMagnifier.push of 1 / 16 frames, per frame
  resident_ms_per_displayed_frame                 the live view available without the stream: ONE rm_magnify (rm_magnify_bgr for D) over a
                                                  resident 256-frame buffer per displayed frame
  unfused_ms_per_frame                            the composition the stream is defined by, unfused: eulerian_magnification_bandpass with
                                                  temporal_bandpass_filter_sos on 256 frames, + frames, divided by 256 (gray, float64)
Wall clock around a synchronised call; medians of the repetitions, every repetition kept beside them.  Prints one JSON line.  No
threshold is set on these figures: they are recorded."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"A": dict(H=1080, W=1920, levels=9, skip=4, dtype="uint8"),
           "B": dict(H=1080, W=1920, levels=9, skip=4, dtype="float64"),
           "C": dict(H=720, W=1280, levels=4, skip=2, dtype="uint8"),
           "D": dict(H=1080, W=1920, levels=9, skip=4, dtype="bgr")}
T_RESIDENT = 256
FPS, FMIN, FMAX, AMP = 30.0, 0.1, 1.0, 50.0


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--configs", default="A,B,C,D")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from respmon_amd import synth, transforms
    from respmon_amd.live import LiveMagnifier
    res = {"tool": "bench_live", "device": torch.cuda.get_device_name(0), "reps": a.reps, "fps": FPS, "band": [FMIN, FMAX], "order": 6,
           "resident_frames": T_RESIDENT, "runs": []}
    med = statistics.median
    for name in a.configs.split(","):
        c = CONFIGS[name]
        H, W, L, S, dt = c["H"], c["W"], c["levels"], c["skip"], c["dtype"]
        vid = torch.from_numpy(synth.synth_breathing_blocks(T_RESIDENT, H, W, seed=1234, workers=16)).cuda()
        if dt == "float64":
            vid = vid.double() * (1. / 255)
        elif dt == "bgr":
            vid = vid.unsqueeze(-1).expand(-1, -1, -1, 3).contiguous()
        colour = dt == "bgr"
        lm = LiveMagnifier(H, W, FPS, FMIN, FMAX, AMP, L, S, color=colour)
        lm.push(vid[:64])                                    # warm-up: workspace, state
        t_p1, t_p16 = [], []
        for i in range(a.reps):
            f1 = vid[(3 * i) % 200:(3 * i) % 200 + 1]
            f16 = vid[(16 * i) % 200:(16 * i) % 200 + 16]
            t_p1.append(timed(torch, lambda: lm.push(f1))[0])
            t_p16.append(timed(torch, lambda: lm.push(f16))[0] / 16)
        state_bytes = lm.state_bytes
        lm.close()
        resident = lambda: transforms.eulerian_magnification_video(vid, FPS, FMIN, FMAX, AMP, L, S, color=colour)
        resident()
        t_res = [timed(torch, resident)[0] for _ in range(a.reps)]
        run = {"config": name, "shape": [H, W], "pyramid_levels": L, "skip_levels_at_top": S, "dtype": dt, "state_bytes": state_bytes,
               "buffer_bytes": vid.numel() * vid.element_size(), "push_n1_ms_per_frame": med(t_p1), "push_n16_ms_per_frame": med(t_p16),
               "resident_ms_per_displayed_frame": med(t_res), "push_n1_ms_all": t_p1, "push_n16_ms_per_frame_all": t_p16,
               "resident_ms_all": t_res}
        if not colour:
            def unfused():
                f = vid if dt == "float64" else transforms.uint8_to_float(vid)
                raw = transforms.eulerian_magnification_bandpass(vid, FPS, FMIN, FMAX, AMP, L, S,
                                                                 temporal_filter_function=transforms.temporal_bandpass_filter_sos)[1]
                return f + raw
            unfused()
            t_un = [timed(torch, unfused)[0] / T_RESIDENT for _ in range(max(3, a.reps // 3))]
            run["unfused_ms_per_frame"] = med(t_un)
            run["unfused_ms_per_frame_all"] = t_un
        res["runs"].append(run)
        del vid
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
