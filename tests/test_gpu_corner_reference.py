"""The corner list on the GPU (k_gftt_cov, k_gftt_eig, k_gftt_candidates and rm_flow.h's selection) against an exact-integer
Shi-Tomasi map (tests/corner_reference.py): rm_good_features_to_track and rm_flow_begin + rm_flow_points on every case of the table
of the host-emulated twin (tests/test_emu_corner_reference.py), which also holds the mutation check of the judge itself."""
import numpy as np
import pytest

from tests import corner_reference as cr

pytestmark = pytest.mark.gpu


class _GpuCorners:
    """check_group's backend interface on the product's C-ABI (device images)."""

    def __init__(self):
        import torch
        assert torch.cuda.is_available()
        from respmon_amd.base import _Backend
        self.torch, self.be = torch, _Backend()
        self.state = self.be.flow_state()

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def gftt(self, img, n, q, d, bs):
        return self.be.good_features_to_track(self.dev(img), n, q, d, bs)

    def begin(self, frame, roi, n, q, d, bs, state=None):
        x, y, w, h = roi
        st = state or self.state
        f = self.dev(frame)
        pts = self.be.flow_begin(st, f, x, y, w, h, n, q, d, bs)
        kept = self.be.flow_points(st, w * h)
        assert (pts is None and len(kept) == 0) or np.array_equal(pts, kept)
        return pts, self.be.roi_to_uint8(f, x, y, w, h).cpu().numpy()

    def states(self, k):
        return [self.be.flow_state() for _ in range(k)]


@pytest.fixture(scope="module")
def be():
    return _GpuCorners()


TALLY = {}


@pytest.mark.parametrize("name", list(cr.GROUPS))
def test_corner_lists_pass_the_exact_tensor(be, name):
    TALLY[name] = cr.check_group(be, name, cr.Tally())


def test_three_subject_begin(be):
    cr.check_three_subjects(be)


def test_completeness_check_is_not_vacuous(be):
    """On the GPU's own lists: every textured and random case but the 3 x 3 crops has a sure pixel, and the completeness check
    examines at least as many sure pixels as the lists hold points."""
    sure = points = 0
    for name in cr.GROUPS:
        t = TALLY.get(name) or cr.check_group(be, name, cr.Tally())
        assert all(c.startswith(("texture_3x3_", "random_3x3_")) for c, _, _ in t.without_sure), t.without_sure[:5]
        sure += t.sure; points += t.points
    print("corner-reference: %d sure pixels examined, %d points listed" % (sure, points))
    assert sure >= points > 10000
