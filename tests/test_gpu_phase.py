"""Phase-based magnification (include/respmon_hip.h rm_phase_*, respmon_amd.live.PhaseMagnifier) on the MI355X: the cases of
tests/phase_cases.py on the shipped kernels -- every clip against the numpy restatement within 64 D, the integer outputs, the first
frame and the unprocessed pyramid bit for bit, every cut of the sequence bit for bit, the bars clip, the refusals -- and the Python
layer.  The host-emulated twin is tests/test_emu_phase.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import phase_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device
    TD = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32,
          np.dtype(np.float64): torch.float64}

    class B:
        lib = _capi.load()
        ctx = device.ctx()
        stream = staticmethod(device.stream_ptr)
        dev = staticmethod(lambda a: torch.from_numpy(np.array(a, order="C")).cuda())      # (a copy: the shared clips are read-only arrays)
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        full = staticmethod(lambda shape, dtype, value: torch.full(tuple(shape), value, dtype=TD[np.dtype(dtype)], device="cuda"))
        np = staticmethod(lambda t: t.cpu().numpy())
    return B


@pytest.mark.parametrize("name", pc.REFERENCE_CASES)
def test_phase_against_reference(be, name):
    pc.check_reference_case(be, name)


@pytest.mark.parametrize("name", pc.INTEGER_CASES)
def test_phase_uint8_out(be, name):
    pc.check_integer_case(be, name)


def test_phase_uint16_and_float32_out(be):
    pc.check_u16_out(be)


def test_phase_first_frame_is_its_own_collapse(be, oracle):
    pc.check_first_frame(be, oracle)


def test_phase_degenerate_regions(be):
    pc.check_degenerate(be)


def test_phase_does_not_depend_on_the_cut(be):
    pc.check_chunk_invariance(be, internal=True)


def test_phase_nothing_processed(be, oracle):
    pc.check_nothing_processed(be, oracle)


def test_phase_purpose_bars(be):
    pc.check_purpose(be)


def test_phase_argument_errors(be):
    pc.check_argument_errors(be)


def test_phase_is_declared(be):
    pc.check_declared(be.lib)


def test_phase_push_is_refused_while_a_submission_is_in_flight_on_another_stream(be):
    """the rule of every entry point that uses the context's workspace (rm_stream_push): RM_E_BUSY, nothing written, state untouched"""
    import torch
    from respmon_amd import synth
    side = torch.cuda.Stream()
    v = pc.moving(4, 8, 9, "f64")
    frames = be.dev(synth.synth_breathing(33, 40, 64, seed=2))
    with pc.Phase(be, 8, 9, 3, 0, pc.butter_sos(1), 10.0) as ph:
        d, out = be.dev(v), be.full(v.shape, np.float64, -7.0)
        tk, xywh = ctypes.c_int(-1), np.zeros(4, np.int32)
        _capi.check(be.lib, be.lib.rm_locate_submit(be.ctx, be.p(frames), _capi.RM_U8, 33, 40, 64, 10.0, 0.1, 1.0, 500.0, 4, 2, 0.7, 20, 0, be.stream(),
                                                    ctypes.byref(tk)), "rm_locate_submit")
        rc = be.lib.rm_phase_push(be.ctx, ph.h, be.p(d), _capi.RM_F64, 4, be.p(out), _capi.RM_F64, ctypes.c_void_p(side.cuda_stream))
        msg = be.lib.rm_last_error_string()
        _capi.check(be.lib, be.lib.rm_locate_result(be.ctx, tk.value, ctypes.c_void_p(xywh.ctypes.data)), "rm_locate_result")
        assert rc == _capi.RM_E_BUSY and b"in flight" in msg
        assert ph.info()[0] == 0 and np.array_equal(be.np(out), np.full(v.shape, -7.0))
        assert ph.push_rc(d, _capi.RM_F64, 4, out, _capi.RM_F64) == _capi.RM_OK and ph.info()[0] == 4


# ---- case 10: the Python layer -------------------------------------------------------------------------------------------------
PY = dict(fps=pc.FPS, freq_min=pc.BAND[0], freq_max=pc.BAND[1], amplification=20, pyramid_levels=4, skip_levels_at_top=0, order=3)


def test_phase_magnifier_numpy_and_tensor_round_trip(be):
    import torch
    from respmon_amd.live import PhaseMagnifier
    name = "moving_37x45_skip0_nsec3_u8"
    v = pc.video_of(pc.CASES[name])
    ref, D = pc.reference(name)
    with PhaseMagnifier(37, 45, out_dtype='float64', **PY) as pm:
        assert pm.frames_seen == 0 and pm.state_bytes == 8 * (5 + 4 * 3) * pc.processed_pixels(37, 45, 4, 0)
        whole = pm.push(np.array(v))
        assert isinstance(whole, np.ndarray) and whole.dtype == np.float64 and pm.frames_seen == len(v)
        pc.check_float(whole, ref, D, name + " PhaseMagnifier")
        pm.reset()
        parts = [pm.push(np.array(v[0]))] + [pm.push(np.array(v[k:k + 4])) for k in range(1, len(v), 4)]      # one [H,W] frame, then chunks
        assert parts[0].shape == (37, 45)
        assert np.array_equal(np.concatenate([parts[0][None]] + parts[1:]), whole)
    with PhaseMagnifier(37, 45, **PY) as pm:                        # uint8 in -> uint8 out
        whole8 = pm.push(np.array(v))
        assert isinstance(whole8, np.ndarray) and whole8.dtype == np.uint8 and whole8.shape == v.shape
        pc.check_integer(whole8, ref, D, 255, name + " PhaseMagnifier uint8")
        pm.reset()
        d = torch.from_numpy(np.array(v)).cuda()
        outs = [pm.push(d[k:k + n]) for k, n in ((0, 1), (1, 2), (3, 7), (10, 2))]
        assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in outs)
        assert torch.equal(torch.cat(outs), torch.from_numpy(whole8).cuda())
        assert pm.frames_seen == len(v)
    with PhaseMagnifier(37, 45, out_dtype=np.float32, blur=False, **PY) as pm:
        assert pm.push(np.array(v[:3])).dtype == np.float32
    with PhaseMagnifier(37, 45, **PY) as pm, pytest.raises(ValueError):
        pm.push(np.zeros((2, 38, 45), np.uint8))
    with PhaseMagnifier(37, 45, **PY) as pm, pytest.raises(ValueError):
        pm.push(np.zeros((2, 37, 45, 3), np.uint8))
    with pytest.raises(TypeError):
        PhaseMagnifier(37, 45, out_dtype='int8', **PY)


def test_phase_magnification_video_is_one_push(be):
    import torch
    from respmon_amd import transforms
    from respmon_amd.live import PhaseMagnifier
    v = np.array(pc.moving(12, 37, 45, "u16"))
    got = transforms.phase_magnification_video(v, PY["fps"], PY["freq_min"], PY["freq_max"], 20, pyramid_levels=4, order=3)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint16
    with PhaseMagnifier(37, 45, **PY) as pm:
        assert np.array_equal(got, pm.push(v))
    dev = transforms.phase_magnification_video(torch.from_numpy(v).cuda(), PY["fps"], PY["freq_min"], PY["freq_max"], 20, pyramid_levels=4, order=3,
                                               out_dtype='float64')
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float64
    ref, D = pc.reference("moving_37x45_skip0_nsec3_u16")
    pc.check_float(dev.cpu().numpy(), ref, D, "moving_37x45_skip0_nsec3_u16 phase_magnification_video")


def test_magnified_calibration_video_methods(be):
    import torch
    from respmon_amd import transforms
    from respmon_amd.base import RespiratoryMonitor
    v = np.array(pc.moving(12, 37, 45, "u8"))
    mon = RespiratoryMonitor.__new__(RespiratoryMonitor)
    mon.calibration_buffer = torch.from_numpy(v).cuda()
    mon.fps, mon.freq_min, mon.freq_max = 10.0, 0.2, 0.8
    today = transforms.eulerian_magnification_video(mon.calibration_buffer, 10.0, 0.2, 0.8, 500, pyramid_levels=9, skip_levels_at_top=4)
    assert torch.equal(mon.magnified_calibration_video(), today)
    assert torch.equal(mon.magnified_calibration_video(method='linear'), today)
    ph = mon.magnified_calibration_video(method='phase')
    assert isinstance(ph, torch.Tensor) and ph.is_cuda and ph.dtype == torch.uint8 and tuple(ph.shape) == v.shape
    assert torch.equal(ph, transforms.phase_magnification_video(mon.calibration_buffer, 10.0, 0.2, 0.8, 10))
    assert torch.equal(ph[0], mon.calibration_buffer[0]) or int((ph[0].int() - mon.calibration_buffer[0].int()).abs().max()) <= 1
    assert mon.magnified_calibration_video(method='phase', out_dtype='float64', amplification=5).dtype == torch.float64
    with pytest.raises(ValueError):
        mon.magnified_calibration_video(method='cubic')
    with pytest.raises(ValueError):
        mon.magnified_calibration_video(method='phase', color=True)


def test_capi_declares_the_five_entries():
    names = ("rm_phase_create", "rm_phase_destroy", "rm_phase_reset", "rm_phase_info", "rm_phase_push")
    assert all(n in _capi.SIGNATURES for n in names)
