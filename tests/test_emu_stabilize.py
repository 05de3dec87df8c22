"""Camera stabilisation (include/respmon_hip.h rm_stab_*, rm_warp_shift) on the host-emulated build (tests/emu): the pyramid, the
reductions with their DPP and LDS folds, the update on the device, the warp and the host orchestration against the numpy restatement
of tests/stabilize_reference.py (the checks of tests/stabilize_cases.py), and what the restatement must show on its own.  The GPU twin
is tests/test_gpu_stabilize.py."""
import ctypes

import numpy as np
import pytest

from tests import stabilize_cases as sc
from tests import stabilize_reference as sr


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


@pytest.fixture(scope="module")
def be(emu):
    class B:
        lib, ctx = emu.lib, emu.ctx
        stream = staticmethod(lambda: None)
        dev = staticmethod(lambda a: np.array(a, order="C"))
        full = staticmethod(lambda shape, dtype, value: np.full(shape, value, dtype=dtype))
        np = staticmethod(lambda a: a)
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        debug_set = staticmethod(emu.debug_set)
    return B


# ---- the restatement alone ---------------------------------------------------------------------------------------------------------
def test_restatement_accuracy_against_the_true_shift():
    e_fine, e_coarse = sc.check_reference_accuracy()
    assert e_coarse < 0.5                                                                  # (levels (3, 1): recorded, not demanded beyond sanity)


def test_restatement_alone_meets_the_purpose():
    still, shaken, true = sc.purpose_scene()
    out, shifts, flags = sr.stabilize(shaken, np.uint8, **sc.PURPOSE_STAB)
    assert not flags.any() and np.abs(shifts - true).max() < 0.05
    sc.purpose_criteria(out, "restatement")


def test_restatement_spread_across_summation_orders():
    D = sc.spread()
    print("D = %.3g px (recorded %.3g); bound max(64 D, 2^-40) = %.3g px" % (D, sc.RECORDED_D, sc.tolerance()))
    assert D < 1e-9                                                                        # a wrong tap or sign shows at 1e-3 px


def test_restatement_warp_is_a_translation_for_integer_shifts():
    f = sc.clip(45, 67, 4.0)[:1]
    got = sr.warp(f, [[3.0, -2.0]], np.uint8)
    ys, xs = np.arange(45), np.arange(67)
    assert np.array_equal(got[0], sr.convert(f[0] * (1. / 255), np.uint8)[np.clip(ys - 2, 0, 44)][:, np.clip(xs + 3, 0, 66)])


# ---- the emulated build --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", sc.WARP_OUTS, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind", sc.WARP_KINDS)
def test_emu_warp_bit_for_bit(be, kind, out_dtype):
    sc.check_warp(be, kind, out_dtype)


def test_emu_warp_bgr_bit_for_bit(be):
    sc.check_warp(be, "bgr", np.uint8)


def test_emu_warp_integer_shift_is_a_translation(be):
    sc.check_warp_integer_shift_is_a_translation(be)


@pytest.mark.parametrize("name", list(sc.ESTIMATE_CASES))
def test_emu_estimate_against_restatement(be, name):
    sc.check_estimate_case(be, name)


def test_emu_push_is_warp_of_the_reported_shifts(be):
    sc.check_composition(be)


@pytest.mark.parametrize("name,out_dtype", [("45x67_odd", np.uint8), ("48x64_f32", np.float64), ("45x67_bgr", np.uint8)])
def test_emu_does_not_depend_on_the_cut(be, name, out_dtype):
    sc.check_cuts(be, name, out_dtype)


def test_emu_constant_reference(be):
    sc.check_constant_reference(be)


def test_emu_far_frame_raises_the_clamp_flag(be):
    sc.check_far_frame(be)


def test_emu_purpose(be):
    sc.check_purpose(be)


def test_emu_refusals(be):
    sc.check_refusals(be)


def test_emu_stab_is_declared(be):
    sc.check_declared(be.lib)
