"""Phase-based magnification (include/respmon_hip.h rm_phase_*) on the host-emulated build (tests/emu): the time kernel, the space
kernel with its LDS staging and repeated reflection, the conversion and the host orchestration against the numpy restatement of
tests/phase_reference.py (cases 1-9 of tests/phase_cases.py), and what the reference must show on its own.  The same 64 D rule applies
here: numpy's sin, cos and atan2 need not equal the host libm's.  The GPU twin is tests/test_gpu_phase.py."""
import ctypes

import numpy as np
import pytest

from tests import phase_cases as pc


@pytest.fixture(scope="module")
def be():
    from tests.emu_harness import Emu
    emu = Emu()

    class B:
        lib, ctx = emu.lib, emu.ctx
        stream = staticmethod(lambda: None)
        dev = staticmethod(lambda a: np.array(a, order="C"))
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        full = staticmethod(lambda shape, dtype, value: np.full(shape, value, dtype=dtype))
        np = staticmethod(lambda a: a)
    return B


# ---- the reference alone ---------------------------------------------------------------------------------------------------------
def test_reference_alone_stays_under_the_integer_cap():
    pc.check_reference_alone_meets_the_integer_cap()


def test_reference_alone_meets_the_purpose():
    ref, D = pc.reference("bars")
    assert 0 < D < 1e-12
    pc.purpose_criteria(ref, "reference")


def test_reference_perturbation_is_small_and_a_wrong_tap_is_not():
    """D stays near the rounding of the three functions; a changed tap of the blur moves the output by far more than 64 D"""
    from tests import phase_reference as pr
    name = "moving_37x45_skip0_nsec1_f64"
    ref, D = pc.reference(name)
    assert 0 < D < 1e-13, D
    c = pc.CASES[name]
    keep = pr.KERNEL.copy()
    try:
        pr.KERNEL[3], pr.KERNEL[5] = keep[5] * 1.01, keep[3] * 0.99
        wrong = pr.phase_magnify(pc.video_of(c), c["levels"], c["skip"], pc.sos_of(c), c["amp"])
    finally:
        pr.KERNEL[:] = keep
    assert np.abs(wrong - ref).max() > 1e-6


# ---- the emulated build --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.REFERENCE_CASES)
def test_emu_phase_against_reference(be, name):
    pc.check_reference_case(be, name)


@pytest.mark.parametrize("name", pc.INTEGER_CASES)
def test_emu_phase_uint8_out(be, name):
    pc.check_integer_case(be, name)


def test_emu_phase_uint16_and_float32_out(be):
    pc.check_u16_out(be)


def test_emu_phase_first_frame_is_its_own_collapse(be, oracle):
    pc.check_first_frame(be, oracle)


def test_emu_phase_degenerate_regions(be):
    pc.check_degenerate(be)


def test_emu_phase_does_not_depend_on_the_cut(be):
    pc.check_chunk_invariance(be, internal=True)


def test_emu_phase_nothing_processed(be, oracle):
    pc.check_nothing_processed(be, oracle)


def test_emu_phase_purpose_bars(be):
    pc.check_purpose(be)


def test_emu_phase_argument_errors(be):
    pc.check_argument_errors(be)


def test_emu_phase_is_declared(be):
    pc.check_declared(be.lib)
