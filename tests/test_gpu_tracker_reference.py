"""calcOpticalFlowPyrLK on the GPU (k_pyr_down_u8, k_scharr, k_lk_track<4> / <16>, and rm_flow_clip's use of lk_track_point) against a
Lucas-Kanade functional in real arithmetic (tests/tracker_reference.py), on every case of tests/tracker_cases.py.  The host-emulated
twin, which also judges the oracle and the judge itself, is tests/test_emu_tracker_reference.py."""
import numpy as np
import pytest

from tests import tracker_cases as tc

pytestmark = pytest.mark.gpu


class _GpuTracker:
    """tracker_cases' backend interface on the product's C-ABI (device images)."""

    def __init__(self):
        import torch
        assert torch.cuda.is_available()
        from respmon_amd.base import _Backend
        self.torch, self.be = torch, _Backend()

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def track(self, prev, nxt, pts, win, max_level, criteria):
        q, st = self.be.calc_optical_flow_pyr_lk(self.dev(prev), self.dev(nxt), pts, winSize=win, maxLevel=max_level, criteria=criteria)
        return q.reshape(-1, 2), st.reshape(-1)

    def crop(self, frame, roi):
        return self.be.roi_to_uint8(self.dev(frame), *roi).cpu().numpy()

    def clip(self, frames, roi, begin, win, max_level, criteria):
        st = self.be.flow_state()
        assert self.be.flow_begin(st, self.dev(frames[0]), *roi, *begin) is not None
        _, ng = self.be.flow_clip(st, self.dev(frames[1:]), *roi, win, max_level, criteria)
        return self.be.flow_points(st, begin[0]), ng


@pytest.fixture(scope="module")
def be():
    return _GpuTracker()


STATS = {}


@pytest.mark.parametrize("name", list(tc.CASES))
def test_gpu_tracker_meets_the_reference(be, name):
    tc.check_case(be, tc.CASES[name], STATS)


def test_gpu_flow_clip_meets_the_reference(be):
    tc.check_clip(be)


def test_gpu_recorded_figures():
    """Not a threshold: prints, per regime, the largest |q - q*| / tol over the cases that ran in this session."""
    for regime in tc.REGIMES:
        rows = [(v["worst"], k[0]) for k, v in STATS.items() if k[1] == regime and v["reach"]]
        if rows:
            print("tracker-reference gpu %s: worst ratio %.3f (%s), largest share left out of (a) %.3f, of (b) %.3f"
                  % (regime, max(rows)[0], max(rows)[1], max(v["left_out"] for k, v in STATS.items() if k[1] == regime),
                     max(v["band"] for k, v in STATS.items() if k[1] == regime)))
