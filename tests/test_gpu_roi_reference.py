"""The ROI winner on the GPU against a reference that follows no border (tests/roi_reference.py): every path of the contour stage
(borders followed on the host; rm_ccl.h's labelled components with and without the area bound, tile kernels and bbox table on and
off) and rm_heatmap_to_rois at every K and min_area, under both frame rules, on the table of the host-emulated twin
(tests/test_emu_roi_reference.py) and on 720p / 1080p images."""
import ctypes

import numpy as np
import pytest

from tests import roi_reference as rr
from tests import subjects_cases as sc

pytestmark = pytest.mark.gpu


_GpuRoi = rr.GpuRoi          # check_product's backend on this build (tests/roi_reference.py)


@pytest.fixture(scope="module")
def be():
    return _GpuRoi()


@pytest.mark.parametrize("geometry", rr.GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_contour_stage_equals_reference(be, geometry):
    """checks 2 and 3 on the table the host-emulated build passes."""
    for case in rr.cases(*geometry):
        rr.check_product(be, case)


@pytest.mark.parametrize("geometry", rr.GPU_GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_contour_stage_equals_reference_at_video_sizes(be, geometry):
    """checks 2 and 3 on three images each of 720p and 1080p: noise, smooth blobs among specks, a hollow frame beside a block."""
    made = rr.cases(*geometry, families=rr.GPU_FAMILIES)
    assert len(made) == 3
    for case in made:
        rr.check_product(be, case)


def test_table_reaches_what_it_is_for(be):
    """check 4; the reference against the oracle on the table (check 1) is tests/test_emu_roi_reference.py's, which needs no GPU."""
    rr.check_table()
    be.paths.clear()
    for case in rr.cases(65, 129) + rr.cases(96, 192):
        be.roi(be.dev(case.heat), False, True)
    assert {3, 4} <= be.paths, be.paths
