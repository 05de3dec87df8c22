"""Parse hipcc's -Rpass-analysis=kernel-resource-usage remarks (respmon_amd/csrc/build_resources.txt, written by the Makefile) into a
table and FAIL when a frame-buffer kernel of the shipped library uses scratch (spilled registers): those kernels stream the
[T,H,W] buffer and every spilled VGPR is HBM traffic on top of it (1.60x the algorithmic bytes on the uint8 chain).
FAIL as well when a kernel occurs more than once in the report: every kernel is compiled in the one translation unit that launches it
(respmon_amd/csrc/rm_internal.h).  A second copy means that a header several units include has begun to launch it, or that two units
launch it themselves instead of going through one launcher.

    python tools/check_resources.py [remarks file] [--all]      exit code 1 on a violation
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = os.path.join(ROOT, "respmon_amd", "csrc", "build_resources.txt")
# kernels that must hold their state in registers: the hot (VB = false) instantiations of the float64 chain and every narrow chain
# ... and the per-clip LK tracker (rm_flow_multi.h): its wave walks all frames of a chunk, scratch would be paid once per frame and point
# ... and the live stream (rm_stream.hip): k_sosfilt keeps the 2 x nsec state values of its element in registers over a whole call, and the
#     SYM = 0 instances of k_magnify (one frame tile in flight) fall under the k_magnify pattern with the SYM = 1 ones
# ... and phase-based magnification (rm_phase.hip): k_phase_time keeps 5 + 4 nsec state values of its pixel in registers over a whole push,
#     k_phase_space streams three planes per frame
# ... and the 'phase' motion signal (rm_phase_motion.hip): k_pm_reduce keeps the previous frame's I, R1, R2, A of its pixel in registers over a chunk
# ... and the multi-subject ROI mean (rm_subjects.h): a workgroup per (frame, subject) pair streams its rectangle once
MUST_NOT_SPILL = re.compile(r"^(void )?rm::k_down_chain<[^>]*, false>|^(void )?rm::k_down_chain_stitch<|^(void )?rm::k_down_chain_u8<|^(void )?rm::k_down_chain_narrow<|"
                            r"^(void )?rm::k_magnify<|^(void )?rm::k_roi_mean_multi_clip<|"
                            r"^(void )?rm::k_lk_track_multi_clip<|^(void )?rm::k_sosfilt<|^(void )?rm::k_phase_time<|^(void )?rm::k_phase_space<|^(void )?rm::k_pm_reduce\b")
# kernels (mangled names, as the report spells them) that may be compiled in more than one unit, each with its reason.  None: wherever
# several units need a kernel, one of them holds a launcher for it (launch_state_init, threshold_mask, launch_heat_minmax, ...).
MAY_REPEAT = set()


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return out.strip().split("\n")
    except Exception:
        return names


def parse(path):
    rows, cur = [], None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        txt = m.group(1).strip()
        if txt.startswith("Function Name:"):
            cur = {"name": txt.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in txt:
            k, v = txt.rsplit(":", 1)
            cur[k.strip()] = v.strip()
    names = demangle([r["name"] for r in rows])
    for r, n in zip(rows, names):
        r["demangled"] = n.split("(")[0]
    return rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else DEFAULT
    rows = parse(path)
    if not rows:
        print("check_resources: no kernel-resource-usage remarks in %s" % path)
        return 1
    bad = []
    show_all = "--all" in sys.argv
    print("%-72s %5s %5s %8s %6s %4s" % ("kernel", "VGPR", "AGPR", "scratch", "spill", "occ"))
    for r in rows:
        scratch = int(r.get("ScratchSize [bytes/lane]", "0"))
        must = bool(MUST_NOT_SPILL.search(r["demangled"]))
        if must and scratch > 0:
            bad.append(r)
        if show_all or must or scratch > 0:
            print("%-72s %5s %5s %8d %6s %4s%s" % (r["demangled"][:72], r.get("VGPRs", "?"), r.get("AGPRs", "?"), scratch, r.get("VGPRs Spill", "?"),
                                                 r.get("Occupancy [waves/SIMD]", "?"), "   <-- must not spill" if must and scratch else ""))
    copies = {}
    for r in rows:
        copies[r["name"]] = copies.get(r["name"], 0) + 1
    repeated = sorted(n for n, c in copies.items() if c > 1 and n not in MAY_REPEAT)
    for n, d in zip(repeated, demangle(repeated)):
        print("%-72s compiled in %d units" % (d.split("(")[0][:72], copies[n]))
    if bad:
        print("check_resources: %d frame-buffer kernel(s) use scratch" % len(bad))
    if repeated:
        print("check_resources: %d kernel(s) are compiled in more than one translation unit" % len(repeated))
    if bad or repeated:
        return 1
    print("check_resources: ok (%d kernels, each compiled once, frame-buffer kernels hold their state in registers)" % len(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
