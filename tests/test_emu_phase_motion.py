"""The 'phase' motion signal (include/respmon_hip.h rm_phase_motion_*, RespiratoryMonitor / SubjectTracker with
motion_extraction_method='phase') on the host-emulated build (tests/emu): the front kernels, the reduction with its DPP and LDS folds,
the finish and the host orchestration against the numpy restatement of tests/phase_motion_reference.py (cases 1-7 of
tests/phase_motion_cases.py), and what the reference must show on its own.  The GPU twin is tests/test_gpu_phase_motion.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import synth
from tests import phase_motion_cases as pm
from tests import phase_motion_reference as pmr


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
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        debug_set = staticmethod(emu.debug_set)
    return B


# ---- the reference alone ---------------------------------------------------------------------------------------------------------
def test_reference_alone_meets_the_purpose():
    f, roi, level = pm.frames_of("roi_l1")
    cx, cy, kx, ky = pm.purpose_criteria(pmr.fsums(pmr.terms(f, roi, level)), "reference")
    assert 0.2 < kx < 0.6 and 0.2 < ky < 0.6


def test_reference_bound_is_tight_enough_to_see_a_wrong_weight():
    pm.check_reference_sees_a_wrong_tap()


# ---- the emulated build --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pm.CASES))
def test_emu_phase_motion_against_reference(be, name):
    pm.check_reference_case(be, name)


def test_emu_phase_motion_zeros_constants_and_first_frames(be):
    pm.check_zeros_and_constants(be)


def test_emu_phase_motion_does_not_depend_on_the_cut(be):
    pm.check_cuts(be)


def test_emu_phase_motion_dtypes_equal_their_widened_forms(be):
    pm.check_dtypes_equal_their_widened_forms(be)


def test_emu_phase_motion_multi_equals_singles(be):
    pm.check_multi_equals_singles(be)


def test_emu_phase_motion_purpose(be):
    pm.check_purpose(be)


def test_emu_phase_motion_refusals(be):
    pm.check_refusals(be)


def test_emu_phase_motion_is_declared(be):
    pm.check_declared(be.lib)


# ---- the Python layer on the emulated C-ABI ------------------------------------------------------------------------------------
class _EmuBackend:
    """The monitor's and the tracker's backend interface on the emulated C-ABI (numpy arrays stand in for device memory)."""

    def __init__(self, emu, be):
        self.emu, self.be = emu, be

    def alloc_buffer(self, T, H, W, dtype):
        raise AssertionError("a monitor past skip_calibration allocates its buffer, but never with this backend in these tests")

    def phase_motion_state(self, w, h, level):
        return pm.Session(self.be, w, h, level)

    def phase_motion_clip(self, state, frames, x, y):
        return state.clip(frames, x, y)

    def phase_motion_multi_clip(self, states, frames, rois):
        return pm.multi(self.be, states, frames, rois)

    def pca_reduce(self, motion):
        return self.emu.pca_reduce(motion)

    def pca_reduce_windows(self, motion, first, window):
        from tests.test_emu_flow_clip import pca_windows
        return pca_windows(self.emu, motion, first, window)

    def pca_reduce_windows_multi(self, rows_list, firsts, window):
        from tests.flow_multi_cases import EmuApi
        return EmuApi(self.emu).pca_multi(rows_list, firsts, window)


class _Buffered(_EmuBackend):
    def alloc_buffer(self, T, H, W, dtype):
        return np.zeros((1, 1, 1))


@pytest.fixture(scope="module")
def factories(emu, be):
    from respmon_amd.base import RespiratoryMonitor
    from respmon_amd.subjects import SubjectTracker

    def make_monitor(frames, roi, phase_params=None, **attrs):
        mon = RespiratoryMonitor(capture_target=synth.FakeCapture(frames[:1], fps=10), visualize=None, save_all_data=True,
                                 motion_extraction_method='phase', run_on_init=False, backend=_Buffered(emu, be), phase_params=phase_params)
        for k, v in attrs.items():
            setattr(mon, k, v)
        mon.skip_calibration(*roi)
        return mon

    def make_tracker(rois, **kw):
        return SubjectTracker(rois, 10, save_all_data=True, backend=_EmuBackend(emu, be), motion_extraction_method='phase', **kw)
    return make_monitor, make_tracker


def test_emu_phase_monitor_clips_equal_the_step_loop(factories):
    pm.check_monitor(factories[0])


def test_emu_phase_tracker_equals_monitors(factories):
    pm.check_tracker(factories[1], factories[0])


def test_unknown_method_is_still_refused():
    from respmon_amd.base import RespiratoryMonitor
    from respmon_amd.subjects import SubjectTracker
    with pytest.raises(AssertionError):
        RespiratoryMonitor(capture_target=synth.FakeCapture(np.zeros((1, 8, 8), np.uint8)), visualize=None, motion_extraction_method='phases',
                           run_on_init=False, backend=object())
    with pytest.raises(AssertionError):
        SubjectTracker([(0, 0, 4, 4)], 10, backend=object(), motion_extraction_method='Phase')
