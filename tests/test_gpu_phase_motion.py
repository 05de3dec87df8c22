"""The 'phase' motion signal (include/respmon_hip.h rm_phase_motion_*, RespiratoryMonitor / SubjectTracker with
motion_extraction_method='phase') on the MI355X: the cases of tests/phase_motion_cases.py on the shipped kernels -- every case against
the numpy restatement within (n - 1) 2^-53 sum |term| + 64 D, zeros and constants, every cut and every grouping of the subjects bit
for bit, the purpose, the refusals -- and the Python layer.  The host-emulated twin is tests/test_emu_phase_motion.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi, synth
from tests import phase_motion_cases as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device

    class B:
        lib = _capi.load()
        ctx = device.ctx()
        stream = staticmethod(device.stream_ptr)
        dev = staticmethod(lambda a: torch.from_numpy(np.array(a, order="C")).cuda())      # (a copy: the shared clips are read-only arrays)
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        debug_set = staticmethod(device.debug_set)
    return B


@pytest.mark.parametrize("name", list(pm.CASES))
def test_phase_motion_against_reference(be, name):
    pm.check_reference_case(be, name)


def test_phase_motion_zeros_constants_and_first_frames(be):
    pm.check_zeros_and_constants(be)


def test_phase_motion_does_not_depend_on_the_cut(be):
    pm.check_cuts(be)


def test_phase_motion_dtypes_equal_their_widened_forms(be):
    pm.check_dtypes_equal_their_widened_forms(be)


def test_phase_motion_multi_equals_singles(be):
    pm.check_multi_equals_singles(be)


def test_phase_motion_purpose(be):
    pm.check_purpose(be)


def test_phase_motion_refusals(be):
    pm.check_refusals(be)


def test_phase_motion_is_declared(be):
    pm.check_declared(be.lib)


def test_phase_motion_is_refused_while_a_submission_is_in_flight_on_another_stream(be):
    """the rule of every entry point that uses the context's workspace (rm_stream_push): RM_E_BUSY, nothing written, state untouched"""
    import torch
    side = ctypes.c_void_p(torch.cuda.Stream().cuda_stream)
    x, y, w, h = pm.ROI
    f = be.dev(pm.clip()[:4])
    frames = be.dev(synth.synth_breathing(33, 40, 64, seed=2))
    with pm.Session(be, w, h, 1) as s, pm.Session(be, w, h, 1) as s2:
        one, two = np.full((4, 3), pm.SENTINEL), np.full((4, 2, 3), pm.SENTINEL)
        rois = np.array([pm.ROI, pm.ROI], np.int32)
        hs = (ctypes.c_void_p * 2)(s.handle.value, s2.handle.value)
        tk, xywh = ctypes.c_int(-1), np.zeros(4, np.int32)
        _capi.check(be.lib, be.lib.rm_locate_submit(be.ctx, be.p(frames), _capi.RM_U8, 33, 40, 64, 10.0, 0.1, 1.0, 500.0, 4, 2, 0.7, 20, 0, be.stream(),
                                                    ctypes.byref(tk)), "rm_locate_submit")
        rc1 = be.lib.rm_phase_motion_clip(be.ctx, s.handle, be.p(f), _capi.RM_U8, 4, pm.H, pm.W, x, y, ctypes.c_void_p(one.ctypes.data), side)
        msg1 = be.lib.rm_last_error_string()
        rc2 = be.lib.rm_phase_motion_multi_clip(be.ctx, hs, be.p(f), _capi.RM_U8, 4, pm.H, pm.W, ctypes.c_void_p(rois.ctypes.data), 2,
                                                ctypes.c_void_p(two.ctypes.data), side)
        msg2 = be.lib.rm_last_error_string()
        _capi.check(be.lib, be.lib.rm_locate_result(be.ctx, tk.value, ctypes.c_void_p(xywh.ctypes.data)), "rm_locate_result")
        assert rc1 == _capi.RM_E_BUSY and b"in flight" in msg1 and rc2 == _capi.RM_E_BUSY and b"in flight" in msg2
        assert s.info()[0] == 0 and s2.info()[0] == 0
        assert np.array_equal(one, np.full((4, 3), pm.SENTINEL)) and np.array_equal(two, np.full((4, 2, 3), pm.SENTINEL))
        assert be.lib.rm_phase_motion_clip(be.ctx, s.handle, be.p(f), _capi.RM_U8, 4, pm.H, pm.W, x, y, ctypes.c_void_p(one.ctypes.data),
                                           be.stream()) == _capi.RM_OK and s.info()[0] == 4


# ---- case 7: the Python layer -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def factories(be):
    from respmon_amd.base import RespiratoryMonitor
    from respmon_amd.subjects import SubjectTracker

    def make_monitor(frames, roi, phase_params=None, **attrs):
        mon = RespiratoryMonitor(capture_target=synth.FakeCapture(frames[:1], fps=10), visualize=None, save_all_data=True,
                                 motion_extraction_method='phase', run_on_init=False, phase_params=phase_params)
        for k, v in attrs.items():
            setattr(mon, k, v)
        mon.skip_calibration(*roi)
        return mon

    def make_tracker(rois, **kw):
        return SubjectTracker(rois, 10, save_all_data=True, motion_extraction_method='phase', **kw)
    return make_monitor, make_tracker


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("clips", ["tensor", "numpy"])
def test_phase_monitor_clips_equal_the_step_loop(factories, clips):
    pm.check_monitor(factories[0], wrap=_cuda if clips == "tensor" else (lambda a: a), frame_wrap=_cuda)


@pytest.mark.parametrize("clips", ["tensor", "numpy"])
def test_phase_tracker_equals_monitors(factories, clips):
    pm.check_tracker(factories[1], factories[0], wrap=_cuda if clips == "tensor" else (lambda a: a))


def test_phase_monitor_equals_the_c_abi(be, factories):
    """the monitor's rows are float32(v) of the library's sums, its values rm_pca_reduce of them"""
    from respmon_amd.base import _Backend
    f = np.array(pm.clip()[:12])
    mon = factories[0](f, pm.ROI)
    mon.step_clip(_cuda(f))
    with pm.Session(be, pm.ROI[2], pm.ROI[3], 1) as s:
        sums = s.clip(f, pm.ROI[0], pm.ROI[1])
    rows = np.array([[r[1] / r[0], r[2] / r[0]] for r in sums[1:]], np.float32)
    assert np.array_equal(np.array(mon.motion_data, np.float32), rows)
    assert mon.data[0] == 0.0 and mon.data[1] == 0.0 and mon.data[-1] == _Backend().pca_reduce(rows)


def test_phase_run_reaches_measure_through_the_capture(be):
    """run() with a 'phase' monitor on a capture: next_frame() -> step(), the per-frame call on device frames"""
    from respmon_amd.base import RespiratoryMonitor
    f = np.array(pm.clip()[:14])
    mon = RespiratoryMonitor(capture_target=synth.FakeCapture(f, fps=10), visualize=None, save_all_data=True, motion_extraction_method='phase',
                             run_on_init=False, phase_params=dict(level=1))
    mon.sync_to_fps = lambda: None
    mon.skip_calibration(*pm.ROI)
    mon.run()
    other = factories_monitor(f)
    other.step_clip(f)
    pm.assert_same_signal(mon, other, "run() against step_clip")
    clips = RespiratoryMonitor(capture_target=synth.FakeCapture(f, fps=10), visualize=None, save_all_data=True, motion_extraction_method='phase',
                               run_on_init=False)
    clips.sync_to_fps = lambda: None
    clips.measure_clip_length = 5
    clips.skip_calibration(*pm.ROI)
    clips.run()
    pm.assert_same_signal(clips, other, "run() with measure_clip_length = 5")


def factories_monitor(f):
    from respmon_amd.base import RespiratoryMonitor
    mon = RespiratoryMonitor(capture_target=synth.FakeCapture(f[:1], fps=10), visualize=None, save_all_data=True, motion_extraction_method='phase',
                             run_on_init=False)
    mon.skip_calibration(*pm.ROI)
    return mon


def test_unknown_method_is_still_refused_on_the_device_backend():
    from respmon_amd.subjects import SubjectTracker
    with pytest.raises(AssertionError):
        SubjectTracker([(0, 0, 4, 4)], 10, motion_extraction_method='phases')
