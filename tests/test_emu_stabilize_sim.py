"""The similarity stabiliser (include/respmon_hip.h rm_stab_sim_*, rm_warp_similarity) on the host-emulated build (tests/emu): the ten
sums with their DPP and LDS folds, the L D L^T factorisation and the substitutions on the device, the gathered residual, the warp and
the host orchestration against the numpy restatement of tests/stabilize_sim_reference.py (the checks of tests/stabilize_sim_cases.py),
and what the restatement must show on its own.  The GPU twin is tests/test_gpu_stabilize_sim.py."""
import ctypes

import numpy as np
import pytest

from tests import stabilize_reference as sr
from tests import stabilize_sim_cases as sc
from tests import stabilize_sim_reference as ssr


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
def test_restatement_accuracy_against_the_truth():
    e_sim, e_shift = sc.check_reference_accuracy()
    assert e_sim < 0.05
    assert e_shift > 0.5


def test_restatement_alone_meets_the_purpose():
    still, shaken, true, _, _ = sc.purpose_scene()
    out, par, flags = ssr.stabilize(shaken, np.uint8, **sc.PURPOSE_STAB)
    out_shift, shifts, _ = sr.stabilize(shaken, np.uint8, **sc.PURPOSE_SHIFT)
    assert not flags.any()
    sc.purpose_criteria(out_shift, out, "restatement")


def test_restatement_alone_meets_the_crop_condition():
    still, shaken, true, _, _ = sc.purpose_scene(sc.CROP_SEED)
    out, par, flags = ssr.stabilize(shaken, np.uint8, **sc.PURPOSE_STAB)
    sc.crop_criteria(out, "restatement")


def test_restatement_spread_across_summation_orders():
    D = sc.spread()
    print("D = %.3g px (recorded %.3g); bound max(64 D, 2^-40) = %.3g px" % (D, sc.RECORDED_D, sc.tolerance()))
    assert D < 1e-9                                                                        # a wrong tap or sign shows at 1e-3 px


def test_restatement_without_linear_levels_is_the_shift_restatement():
    f = sc.frames_of("45x67_odd")
    par, flags = ssr.estimate_clip(f, level_coarse=2, level_fine=0, level_linear=-1, iterations=2, max_shift=4.0, max_linear=0.03)
    shifts, want = sr.estimate_clip(f, level_coarse=2, level_fine=0, iterations=2, max_shift=4.0)
    assert np.array_equal(par[:, 2:], shifts) and not par[:, :2].any() and np.array_equal(flags, want)
    assert sc.same(ssr.warp(f, par, np.uint8), sr.warp(f, shifts, np.uint8))


def test_restatement_far_frames_raise_the_linear_clamp_flag():
    f, (rp, rf) = sc.far_clip()
    assert rf[0] == 0 and (rf[1:] & ssr.FLAG_LINEAR_CLAMPED).any(), rf


def test_valid_rect_arithmetic():
    sc.check_valid_rect_arithmetic()


def test_synth_similarity_scene():
    from respmon_amd import synth
    still, shaken, true = synth.synth_shaky_breathing_similarity(6, 40, 56, jitter=2.0, rot_deg=1.5, zoom=0.015, seed=3)
    assert still.shape == shaken.shape == (6, 40, 56) and still.dtype == shaken.dtype == np.uint8 and true.shape == (6, 4)
    assert np.array_equal(still[0], shaken[0]) and not true[0].any() and not np.array_equal(still[1], shaken[1])   # the first frame is not moved
    assert np.abs(ssr.rotation_deg(true)).max() <= 1.5 and np.abs(ssr.zoom(true) - 1).max() <= 0.015 + 1e-12 and np.abs(true[:, 2:]).max() <= 2.0
    # the inverse coordinates are the inverse of the rule's transform
    x, y = synth.similarity_scene_coords(40, 56, true[2])
    fx, fy = ssr.positions(true[2], 27.5, 19.5, x[7, :], [0.0], true[2, 2], true[2, 3])
    fy = ssr.positions(true[2], 27.5, 19.5, x[7, :], y[7, :], true[2, 2], true[2, 3])[1]
    assert np.abs(np.diag(fy) - 7.0).max() < 1e-9
    # ... and synth_texture itself renders what it rendered: render(dx, dy) is at(xx - dx, yy - dy)
    r = synth.synth_texture(40, 56)
    yy, xx = np.mgrid[0:40, 0:56].astype(np.float64)
    assert np.array_equal(r(1.25, -0.5), r.at(xx - 1.25, yy + 0.5))


# ---- the emulated build --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", sc.WARP_OUTS, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind", sc.WARP_KINDS)
def test_emu_warp_bit_for_bit(be, kind, out_dtype):
    sc.check_warp(be, kind, out_dtype)


def test_emu_warp_bgr_bit_for_bit(be):
    sc.check_warp(be, "bgr", np.uint8)


def test_emu_warp_with_zero_linear_part_is_warp_shift(be):
    sc.check_warp_zero_linear_is_warp_shift(be)


@pytest.mark.parametrize("name", list(sc.ESTIMATE_CASES))
def test_emu_estimate_against_restatement(be, name):
    sc.check_estimate_case(be, name)


def test_emu_no_linear_level_is_the_shift_model(be):
    sc.check_no_linear_level_is_the_shift_model(be)


def test_emu_push_is_warp_of_the_reported_parameters(be):
    sc.check_composition(be)


@pytest.mark.parametrize("name,out_dtype", [("45x67_odd", np.uint8), ("48x64_f32", np.float64), ("45x67_bgr", np.uint8)])
def test_emu_does_not_depend_on_the_cut(be, name, out_dtype):
    sc.check_cuts(be, name, out_dtype)


def test_emu_constant_reference(be):
    sc.check_constant_reference(be)


def test_emu_far_frame_raises_the_linear_clamp_flag(be):
    sc.check_far_frame(be)


def test_emu_purpose(be):
    sc.check_purpose(be)


def test_emu_crop(be):
    sc.check_crop(be)


def test_emu_valid_rect_on_warped_frames(be):
    sc.check_valid_rect_on_warped_frames(be)


def test_emu_refusals(be):
    sc.check_refusals(be)


def test_emu_stab_sim_is_declared(be):
    sc.check_declared(be.lib)
