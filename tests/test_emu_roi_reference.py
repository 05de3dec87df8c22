"""The ROI winner against a reference that follows no border (tests/roi_reference.py), on the host-emulated build (tests/emu): the
reference against the oracle on the case table and a seeded random sweep, every path of the product's contour stage against the
reference, rm_heatmap_to_rois at every K and min_area, and the table itself.  The GPU twin is tests/test_gpu_roi_reference.py."""
import numpy as np
import pytest

from tests import roi_reference as rr
from tests import subjects_cases as sc
from tests.emu_harness import ptr


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


_EmuRoi = rr.EmuRoi          # check_product's backend on this build (tests/roi_reference.py)


@pytest.mark.parametrize("geometry", rr.GEOMETRIES + [(720, 1280)], ids=lambda g: "%dx%d" % g)
def test_emu_reference_equals_oracle_on_the_table(oracle, geometry):
    """check 1: list (in findContours' order), areas and winner of every case up to 1300 x 800 -- the 720p images of the GPU module
    included --, under both frame rules."""
    n = 0
    for case in rr.cases(*geometry) if geometry in rr.GEOMETRIES else rr.cases(*geometry, families=rr.GPU_FAMILIES):
        for clip in (False, True):
            n += rr.check_against_oracle(oracle, case.m, clip)
    assert n > 0 or geometry == (1, 1)


def test_emu_reference_equals_oracle_on_a_random_sweep(oracle):
    """check 1 on 2500 seeded random images from 1 x 1 to 40 x 60 (noise at densities 0.05 to 0.95, smooth blobs, blobs with specks),
    both frame rules: more than 20 000 external contours and more than 100 exact ties for the maximum."""
    rng = np.random.default_rng(7)
    contours = ties = 0
    for i in range(2500):
        m = rr.random_image(rng)
        contours += rr.check_against_oracle(oracle, m, bool(i & 1))
        a = sorted(c[4] for c in rr.ranked(m, bool(i & 1)))
        ties += len(a) > 1 and a[-1] == a[-2]
    print("roi-reference: %d contours, %d ties for the maximum" % (contours, ties))
    assert contours > 20000 and ties > 100


# A call of the emulated build costs 50 ms on a 64 x 64 image and 1.5 s at 352 x 640 (every lane is a fiber), and the whole table makes
# some 20 000 of them.  The emulated twin therefore leaves out 352 x 640, takes a selection of 64 x 128 and 96 x 192, and asks for the
# labelled path once under the <= 3.1 frame rule (which the host path alone serves); the GPU module runs every case through everything.
EMU_PATHS = (rr.cases(64, 64) + rr.cases(33, 70) + rr.cases(65, 129) +                           # every family: one tile column, ragged rows
             [c for c in rr.cases(64, 128) if c.name.startswith(("a_noise0.45", "b_blobs_specks", "c_"))] +        # the tile kernels
             [c for c in rr.cases(96, 192) if c.name.startswith(("a_noise0.62", "c_checker"))] +                   # 3 x 3 tiles
             rr.cases(1, 1) + rr.cases(3, 3) + rr.cases(1, 200)[:2] + rr.cases(200, 1)[:2])
EMU_LISTS = rr.cases(33, 70)                                                                     # every family, the tie permutations included


@pytest.mark.parametrize("case", EMU_PATHS, ids=repr)
def test_emu_contour_stage_equals_reference(emu, case):
    """check 2: borders followed on the host, labelled components with and without the area bound, tiles and table on and off, under
    both frame rules."""
    rr.check_product(_EmuRoi(emu), case, lists=False, clip_labelled=False)


@pytest.mark.parametrize("case", EMU_LISTS, ids=repr)
def test_emu_ranked_list_equals_reference(emu, case):
    """check 3: rm_heatmap_to_rois at every K and min_area, rectangles and areas, under both frame rules."""
    rr.check_product(_EmuRoi(emu), case, paths=False)


def test_emu_table_reaches_what_it_is_for(emu):
    """check 4: ties tie, the box-bound leader loses, the island outweighs its ring, the frame rules differ; and the labelled path
    both settles a winner by the area bound alone (path 4) and has to follow a border (path 3) somewhere in the table."""
    rr.check_table()
    be = _EmuRoi(emu)
    for case in rr.cases(65, 129):
        be.roi(case.heat, False, True)
    assert {3, 4} <= be.paths, be.paths
