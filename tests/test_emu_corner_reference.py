"""The corner list against an exact-integer Shi-Tomasi map (tests/corner_reference.py) on the host-emulated build (tests/emu):
rm_good_features_to_track and rm_flow_begin + rm_flow_points on every case of the table, the condition that keeps the completeness
check from being vacuous, and the mutation check that shows the judge sees the errors it is there for.  The GPU twin is
tests/test_gpu_corner_reference.py."""
import ctypes

import numpy as np
import pytest

from tests import corner_reference as cr
from tests.emu_harness import DT, ptr


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


class _EmuCorners:
    """check_group's backend interface on the emulated C-ABI."""

    def __init__(self, emu):
        self.emu = emu
        self.state = emu.flow_state()

    def gftt(self, img, n, q, d, bs):
        return self.emu.good_features(img, n, q, d, bs)

    def begin(self, frame, roi, n, q, d, bs, state=None):
        x, y, w, h = roi
        st = state or self.state
        pts = self.emu.flow_begin(frame, x, y, w, h, n, q, d, bs, state=st)
        kept = self.emu.flow_points(w * h, state=st)
        assert (pts is None and len(kept) == 0) or np.array_equal(pts, kept)
        crop = np.empty((h, w), np.uint8)
        f = np.ascontiguousarray(frame)
        self.emu.ck(self.emu.lib.rm_roi_to_uint8(self.emu.ctx, ptr(f), DT[f.dtype], f.shape[0], f.shape[1], x, y, w, h, ptr(crop), None), "roi_to_uint8")
        return pts, crop

    def states(self, k):
        return [self.emu.flow_state() for _ in range(k)]


TALLY = {}


@pytest.mark.parametrize("name", list(cr.GROUPS))
def test_emu_corner_lists_pass_the_exact_tensor(emu, name):
    TALLY[name] = cr.check_group(_EmuCorners(emu), name, cr.Tally())


def test_emu_three_subject_begin(emu):
    cr.check_three_subjects(_EmuCorners(emu))


def test_emu_completeness_check_is_not_vacuous(emu, oracle):
    """Every textured and every random case has a sure pixel (a 3 x 3 crop cannot: tests/corner_reference.py _with_sure), and over the
    table the completeness check examines at least as many sure pixels as the lists hold points -- for the oracle's lists and for the
    emulated build's."""
    assert cr.check_3x3_has_no_sure_pixel() > 300
    for be in (cr.OracleCorners(oracle), None):
        sure = points = 0
        for name in cr.GROUPS:
            t = cr.check_group(be, name, cr.Tally()) if be is not None else (TALLY.get(name) or cr.check_group(_EmuCorners(emu), name, cr.Tally()))
            assert all(c.startswith(("texture_3x3_", "random_3x3_")) for c, _, _ in t.without_sure), t.without_sure[:5]
            sure += t.sure; points += t.points
        print("corner-reference: %d sure pixels examined, %d points listed" % (sure, points))
        assert sure >= points > 10000


def test_emu_mutated_references_reject_the_oracle(oracle):
    """The oracle's lists of 200 seeded cases: the reference rejects none, and each deliberately wrong reference (Sobel border
    symmetric, box border symmetric, one tensor entry doubled) rejects more than half."""
    rejected = cr.mutation_sweep(oracle, 200)
    print("corner-reference: rejected of 200:", rejected)
    assert rejected.pop("none") == 0
    assert all(v > 100 for v in rejected.values()), rejected
