"""developer: the sliding-window calibration (respmon_amd/window.py, rm_window_*) against rm_locate on the equivalent resident buffer, in
ONE process, alternating.

    python tools/bench_window.py [--reps 9] [--configs P,Q] [--out profiles/window.json]

  P   1080p x 256, pyramid_levels 9 / skip 4, uint8 and float64 frames
  Q   720p x 128, pyramid_levels 4 / skip 2, uint8 frames
For each: the ring is filled and wrapped (head != 0, so the relocation runs the RING variants of the temporal kernels), then
  push_n1_ms_per_frame / push_n16_ms_per_frame    rm_window_push of 1 / 16 frames, per frame
  relocate_ms                                     rm_window_locate from the full ring
  locate_ms                                       rm_locate on the contiguous [T,H,W] buffer of the frames the ring holds (ROI asserted equal
                                                  before anything is timed)
with ring_bytes next to buffer_bytes.  Prints one JSON line; medians of the alternating repetitions, every repetition kept beside them.
No threshold is set on these figures: they are recorded."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"P": dict(T=256, H=1080, W=1920, levels=9, skip=4, dtypes=("uint8", "float64")),
           "Q": dict(T=128, H=720, W=1280, levels=4, skip=2, dtypes=("uint8",))}


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--configs", default="P,Q")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from respmon_amd import synth
    from respmon_amd.base import _Backend
    from respmon_amd.window import SlidingCalibration
    be = _Backend()
    res = {"tool": "bench_window", "device": torch.cuda.get_device_name(0), "reps": a.reps, "runs": []}
    for name in a.configs.split(","):
        c = CONFIGS[name]
        T, H, W, L, S = c["T"], c["H"], c["W"], c["levels"], c["skip"]
        extra = 48                                           # frames pushed beyond the first fill: the ring ends wrapped
        vid = synth.synth_breathing_blocks(T + extra, H, W, seed=1234, workers=16)
        for dt in c["dtypes"]:
            stream = torch.from_numpy(vid).cuda()
            if dt == "float64":
                stream = stream.double() * (1. / 255)
            win = SlidingCalibration(T, H, W, L, S)
            win.push(stream[:T])
            for k in range(T, T + extra, 16):
                win.push(stream[k:k + 16])
            assert win.count == T and win.head == extra % T != 0
            resident = stream[extra:T + extra].contiguous()
            relocate = lambda: win.locate(10)
            locate = lambda: be.locate(resident, 10, 0.1, 1.0, 500, L, S, 0.7, 20)
            r_win, r_buf = relocate(), locate()
            assert r_win == r_buf and r_win is not None, (r_win, r_buf)
            t_re, t_lo, t_p1, t_p16 = [], [], [], []
            for i in range(a.reps):
                t_lo.append(timed(torch, locate)[0])
                t_re.append(timed(torch, relocate)[0])
            # pushes last: they slide the window (frames of the stream again, so the ring keeps real content)
            for i in range(a.reps):
                f1 = stream[(3 * i) % T:(3 * i) % T + 1]
                f16 = stream[(16 * i) % T:(16 * i) % T + 16]
                t_p1.append(timed(torch, lambda: win.push(f1))[0])
                t_p16.append(timed(torch, lambda: win.push(f16))[0] / 16)
            med = statistics.median
            res["runs"].append({"config": name, "T": T, "shape": [H, W], "pyramid_levels": L, "skip_levels_at_top": S, "dtype": dt,
                                "ring_bytes": win.ring_bytes, "buffer_bytes": resident.numel() * resident.element_size(), "roi": list(r_win),
                                "push_n1_ms_per_frame": med(t_p1), "push_n16_ms_per_frame": med(t_p16), "relocate_ms": med(t_re),
                                "locate_ms": med(t_lo), "relocate_ms_all": t_re, "locate_ms_all": t_lo, "push_n1_ms_all": t_p1,
                                "push_n16_ms_per_frame_all": t_p16})
            win.close()
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
