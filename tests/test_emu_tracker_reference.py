"""calcOpticalFlowPyrLK against a Lucas-Kanade functional in real arithmetic (tests/tracker_reference.py) on the cases of
tests/tracker_cases.py: the oracle's restatement (oracle/cvref_flow.c -- this is the run that pins it) and the host-emulated kernels
(k_lk_track / lk_track_point, and rm_flow_clip's use of it).  Also the judge's own teeth, and the oracle's LK pyramid level and Scharr image
against the integer statement; the kernels' are not readable (rm_debug_workspace names the context's buffers, not the flow workspace), so
for them the multi-level cases stand.  The GPU twin is tests/test_gpu_tracker_reference.py."""
import numpy as np
import pytest

from tests import tracker_cases as tc
from tests.emu_harness import DT, ptr


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


class _EmuTracker:
    """tracker_cases' backend interface on the emulated C-ABI."""

    def __init__(self, emu):
        self.emu = emu

    def track(self, prev, nxt, pts, win, max_level, criteria):
        q, st = self.emu.pyr_lk(prev, nxt, pts, winSize=win, maxLevel=max_level, criteria=criteria)
        return q.reshape(-1, 2), st.reshape(-1)

    def crop(self, frame, roi):
        x, y, w, h = roi
        f = np.ascontiguousarray(frame)
        out = np.empty((h, w), np.uint8)
        self.emu.ck(self.emu.lib.rm_roi_to_uint8(self.emu.ctx, ptr(f), DT[f.dtype], f.shape[0], f.shape[1], x, y, w, h, ptr(out), None), "roi_to_uint8")
        return out

    def clip(self, frames, roi, begin, win, max_level, criteria):
        emu = self.emu
        st = emu.flow_state()
        assert emu.flow_begin(frames[0], *roi, *begin, state=st) is not None
        f = np.ascontiguousarray(frames[1:])
        n, H, W = f.shape
        mean, ng = np.empty((n, 2), np.float32), np.empty(n, np.int32)
        emu.ck(emu.lib.rm_flow_clip(emu.ctx, st, ptr(f), DT[f.dtype], n, H, W, *roi, win[0], win[1], max_level, criteria[1], float(criteria[2]),
                                    ptr(mean), ptr(ng), None), "flow_clip")
        return emu.flow_points(begin[0], state=st), ng


STATS = {"oracle": {}, "emu": {}}


@pytest.mark.parametrize("name", list(tc.CASES))
def test_oracle_tracker_meets_the_reference(oracle, name):
    tc.check_case(tc.OracleTracker(oracle), tc.CASES[name], STATS["oracle"])


@pytest.mark.parametrize("name", list(tc.CASES))
def test_emu_tracker_meets_the_reference(emu, name):
    tc.check_case(_EmuTracker(emu), tc.CASES[name], STATS["emu"])


def test_status_images_do_their_job():
    tc.check_status_images_do_their_job()


def test_emu_flow_clip_meets_the_reference(emu):
    tc.check_clip(_EmuTracker(emu))


def test_oracle_lk_images_are_the_integer_statement(oracle):
    tc.check_oracle_images(oracle)


def test_judge_rejects_spoiled_outputs(oracle):
    """The oracle's outputs pass untouched; pushed 3 tol away, with x and y exchanged, or tracked from p + (1, 0), at least 90 % of the
    eligible points are rejected."""
    tally = tc.teeth(tc.OracleTracker(oracle))
    print("tracker-reference teeth (rejected, eligible):", tally)
    assert tally.pop("none")[0] == 0
    for way, (rejected, eligible) in tally.items():
        assert eligible >= 500 and rejected >= 0.9 * eligible, (way, rejected, eligible)


def test_judge_sees_exchanged_window_sides(oracle):
    """win_w bounding y and win_h bounding x moves q* by less than most tolerances, so no 90 % here: but each oblong case must lose points
    in the distance check, and the border probes must show it in the status check."""
    got = tc.window_mixup(tc.OracleTracker(oracle))
    print("tracker-reference exchanged window sides (case, distance rejections, status errors):", got)
    assert all(far > 0 and status > 0 for _, far, status in got), got


def test_recorded_figures():
    """Not a threshold: prints, per subject and regime, the largest |q - q*| / tol over the cases that ran in this session."""
    for subject, stats in STATS.items():
        for regime in tc.REGIMES:
            rows = [(v["worst"], k[0]) for k, v in stats.items() if k[1] == regime and v["reach"]]
            if rows:
                print("tracker-reference %s %s: worst ratio %.3f (%s), largest share left out of (a) %.3f, of (b) %.3f"
                      % (subject, regime, max(rows)[0], max(rows)[1], max(v["left_out"] for k, v in stats.items() if k[1] == regime),
                         max(v["band"] for k, v in stats.items() if k[1] == regime)))
