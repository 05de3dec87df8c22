"""uint16 frame buffers (RM_U16, include/respmon_hip.h) on the host-emulated build (tests/emu): every entry point given a uint16 buffer
returns, bit for bit, what it returns on the float64 buffer of k * (1./65535) (tests/u16_cases.py).  The shapes are the smallest that
reach each path of the frame-buffer kernels.  The GPU twin is tests/test_gpu_u16.py."""
import ctypes

import numpy as np
import pytest

from tests import u16_cases as uc


@pytest.fixture(scope="module")
def be():
    from tests.emu_harness import Emu
    emu = Emu()

    class B:
        lib, ctx = emu.lib, emu.ctx
        stream = staticmethod(lambda: None)
        dev = staticmethod(lambda a: np.array(a, order="C"))       # (a copy: the shared videos are read-only arrays)
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        np = staticmethod(lambda a: a)
    return B


@pytest.fixture(scope="module")
def identity(be):
    return uc.check_conversions(be)


def test_emu_u16_conversions(be, identity):
    # u16(k * (1./65535) * 65535) is NOT assumed to be k: the table is what rm_float_to_uint16 and numpy agree on
    assert identity.dtype == np.uint16 and identity.shape == (65536,)
    assert np.array_equal(identity, (np.arange(65536) * uc.SCALE * 65535).astype(np.int64).astype(np.uint16))


# (T, H, W, levels, skip, flags): the path each reaches
CALIBRATION = [(2, 67, 131, 5, 3, 0),      # ragged width: the generic chain
               (1, 135, 240, 6, 4, 0),     # the register chain at depth 4
               (1, 40, 800, 4, 2, 0),      # ... at depth 2 (hot blocks)
               (1, 48, 704, 6, 4, 0),
               (1, 36, 401, 5, 3, 0),
               (1, 70, 1936, 6, 4, 0),     # three strips
               (3, 48, 64, 3, 0, 0),       # skip 0: no chain, the conversion kernel
               (3, 64, 96, 4, 2, 2),       # one pyrDown launch per level
               (3, 64, 96, 4, 2, 64 | 8)]  # tiny strips


@pytest.mark.parametrize("case", CALIBRATION, ids=str)
def test_emu_u16_calibration_equals_the_f64_buffer(be, case):
    uc.check_calibration(be, *case)


def test_emu_u16_every_level_at_depth_1(be):
    uc.check_calibration(be, 1, 256, 256, 3, 1, frames=uc.every_level())


def test_emu_u16_locate_equals_the_oracle_and_ignores_the_sample_alignment(be):
    uc.check_locate_oracle(be, 32, 96, 128, 4, 2)


def test_emu_u16_roi_means_and_crops(be):
    uc.check_motion(be)


def test_emu_u16_flow_clip(be):
    uc.check_flow_clip(be)


@pytest.mark.parametrize("shape", [(5, 40, 80, 5, 3), (4, 70, 70, 7, 5)], ids=str)     # fused k_magnify / the plain kernel behind a materialised raw
def test_emu_u16_magnify(be, identity, shape):
    uc.check_magnify(be, *shape, identity=identity)


def test_emu_u16_magnify_clamps(be):
    uc.check_magnify_clamp(be)


def test_emu_u16_stream_pushes(be):
    uc.check_stream(be)


def test_emu_u16_arguments(be):
    uc.check_arguments(be)
