"""The rate map (include/respmon_hip.h rm_spectral_operator / rm_spectral_peak / rm_rate_map / rm_window_rate_map) on the host-emulated
build (tests/emu): the MFMA contraction in both forms, the LDS epilogue, the ring variant and the host orchestration against the
reference of tests/rate_cases.py (cases 1-6; the emulated contractions stay at T <= 128).  The GPU twin is tests/test_gpu_rate_map.py."""
import ctypes

import numpy as np
import pytest

from tests import rate_cases as rc


@pytest.fixture(scope="module")
def be():
    from tests.emu_harness import Emu
    emu = Emu()

    class B:
        lib, ctx = emu.lib, emu.ctx
        cus = 256                        # what the emulated hipDeviceGetAttribute answers
        stream = staticmethod(lambda: None)
        dev = staticmethod(np.ascontiguousarray)
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        out = staticmethod(lambda shape: np.full(shape, np.nan))
        out_i32 = staticmethod(lambda shape: np.full(shape, -7, np.int32))
        np = staticmethod(lambda a: a)
    return B


@pytest.mark.parametrize("case", rc.OPERATOR_CASES, ids=str)
def test_emu_spectral_operator(be, case):
    rc.check_operator(be.lib, case)


def test_reference_meets_the_caps_on_its_own_inputs():
    """no ambiguous pixel and every frequency bound far below 1e-6 on the inputs of case 1 at three of its sizes,
    by the reference alone (no library involved)"""
    for T, F in ((128, 64), (64, 16), (33, 17)):
        _, ref = rc._ref_case1(T, F)
        assert not ref.ambiguous.any(), (T, F)
        fin = ref.inner & np.isfinite(ref.delta_bound)
        assert fin.sum() > 100 and ref.delta_bound[fin].max() < 1e-9, (T, F, float(ref.delta_bound[fin].max()))


@pytest.mark.parametrize("F", rc.FS)
@pytest.mark.parametrize("T", rc.TS)
def test_emu_spectral_peak_against_reference(be, T, F):
    rc.check_peak(be, T, F)


def test_emu_spectral_peak_either_side_of_the_form_switch(be):
    rc.check_form_switch(be)


def test_emu_degenerate_columns(be):
    rc.check_degenerate(be)


@pytest.mark.parametrize("T", (16, 9))
@pytest.mark.parametrize("geom", rc.RATE_GEOMS, ids=str)
def test_emu_rate_map_equals_peak_of_pyr_down(be, geom, T):
    rc.check_rate_map_equals_peak(be, geom, T)


@pytest.mark.parametrize("T", (16, 9))
def test_emu_window_rate_map_equals_rate_map(be, T):
    rc.check_window(be, T)


def test_purpose_criteria_are_met_by_the_reference_alone():
    freq, power, index = rc.purpose_reference()
    worst = rc.purpose_criteria(freq, power, index, "reference")
    assert worst < 0.5          # (the criterion is one step; the estimator itself stays well inside)


def test_emu_purpose_three_blobs(be):
    rc.check_purpose(be)


def test_emu_rate_argument_errors(be):
    rc.check_argument_errors(be)
