"""rm_sosfilt, rm_stream_* and respmon_amd.live.LiveMagnifier on the MI355X: the cases of tests/stream_cases.py on the shipped kernels --
the filter against its definition, the stream against the reference's operation order bit for bit in every chunking, state hygiene,
refusals -- and the Python surface.  The host-emulated twin is tests/test_emu_stream.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device
    lib = _capi.load()
    side = torch.cuda.Stream()
    TD = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}

    class B:
        ctx = device.ctx()
        stream = staticmethod(device.stream_ptr)
        other_stream = staticmethod(lambda: ctypes.c_void_p(side.cuda_stream))
        dev = staticmethod(lambda a: torch.from_numpy(np.array(a, order="C")).cuda())      # (a copy: the shared videos are read-only arrays)
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        empty = staticmethod(lambda shape, dtype: torch.zeros(tuple(shape), dtype=TD[np.dtype(dtype)], device="cuda"))
        np = staticmethod(lambda t: t.cpu().numpy())

        @staticmethod
        def new_ctx(dev_index=0):
            if dev_index >= torch.cuda.device_count():
                return None
            h = ctypes.c_void_p()
            return h if lib.rm_ctx_create(dev_index, ctypes.byref(h)) == _capi.RM_OK else None

        free_ctx = staticmethod(lib.rm_ctx_destroy)
    B.lib = lib
    assert side.cuda_stream != (device.stream_ptr().value or 0)
    return B


LOC = (sc.FPS, 0.1, 1.0, 500.0, 4, 2, 0.7, 20, 0)      # fps, band, amplification, levels, skip, temporal threshold, threshold, flags


def _locate(be, v):
    d = be.dev(v)
    xywh = np.zeros(4, np.int32)
    _capi.check(be.lib, be.lib.rm_locate(be.ctx, be.p(d), _capi.RM_U8, *v.shape, *LOC, ctypes.c_void_p(xywh.ctypes.data), be.stream()), "rm_locate")


def _magnify(be, v):
    d, out = be.dev(v), be.empty(v.shape, np.uint8)
    _capi.check(be.lib, be.lib.rm_magnify(be.ctx, be.p(d), _capi.RM_U8, *v.shape, 10.0, 0.1, 1.0, 500.0, 4, 2, be.p(out), _capi.RM_U8, be.stream()), "rm_magnify")


def _submit(be, v):
    d = be.dev(v)
    tk = ctypes.c_int(-1)
    _capi.check(be.lib, be.lib.rm_locate_submit(be.ctx, be.p(d), _capi.RM_U8, *v.shape, *LOC, be.stream(), ctypes.byref(tk)), "rm_locate_submit")
    return tk.value, d


def _result(be, ticket):
    xywh = np.zeros(4, np.int32)
    _capi.check(be.lib, be.lib.rm_locate_result(be.ctx, ticket[0], ctypes.c_void_p(xywh.ctypes.data)), "rm_locate_result")


def _lfilter(be, b, a, x):
    d, out = be.dev(x), be.empty(x.shape, np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64); a = np.ascontiguousarray(a, dtype=np.float64)
    _capi.check(be.lib, be.lib.rm_lfilter(be.ctx, be.p(d), x.shape[0], x[0].size, ctypes.c_void_p(b.ctypes.data), ctypes.c_void_p(a.ctypes.data), len(b),
                                          1.0, be.p(out), be.stream()), "rm_lfilter")
    return be.np(out)


@pytest.mark.parametrize("rate", sc.SOS_RATES, ids=lambda r: "fps%g_%g-%g" % r)
@pytest.mark.parametrize("order", sc.SOS_ORDERS)
def test_sosfilt_equals_its_definition_bit_for_bit(be, order, rate):
    sc.check_sosfilt(be, order, rate)


def test_sosfilt_refusals(be):
    sc.check_sosfilt_refusals(be)


def test_sections_are_stable_where_the_ba_form_is_not(be):
    sc.check_why_sos(be, lambda b, a, x: _lfilter(be, b, a, x))


@pytest.mark.parametrize("with_zi", [False, True], ids=["rest", "zi"])
@pytest.mark.parametrize("case", sc.STREAM_CASES, ids=sc.case_id)
def test_stream_is_its_definition_however_it_is_cut(be, case, with_zi):
    sc.check_stream_case(be, case, with_zi)


def test_stream_steady_start_is_quiet(be):
    sc.check_steady_start_is_quiet(be)


def test_stream_state_hygiene(be):
    sc.check_state_hygiene(be, lambda v: _locate(be, v), lambda v: _magnify(be, v))


def test_stream_refusals(be):
    sc.check_stream_refusals(be, lambda v: _submit(be, v), lambda tk: _result(be, tk))


@pytest.mark.parametrize("case", sc.REFERENCE_CASES, ids=sc.case_id)
def test_stream_means_what_the_reference_means(be, oracle, case):
    sc.check_means_what_the_reference_means(be, oracle, case)


def test_stream_is_declared_everywhere(be):
    sc.check_bookkeeping(be.lib)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
PY = dict(fps=sc.FPS, freq_min=sc.BAND[0], freq_max=sc.BAND[1], amplification=sc.AMP, pyramid_levels=4, skip_levels_at_top=2)


def test_live_magnifier_rest_is_the_sos_composition_plus_the_frame():
    from respmon_amd import transforms
    from respmon_amd.live import LiveMagnifier
    v = sc.video(40, 70, np.uint8)
    f = v * (1.0 / 255)
    raw = transforms.eulerian_magnification_bandpass(f, sc.FPS, sc.BAND[0], sc.BAND[1], sc.AMP, pyramid_levels=4, skip_levels_at_top=2,
                                                     temporal_filter_function=transforms.temporal_bandpass_filter_sos)[1]
    assert np.abs(raw).max() > 1e-3
    with LiveMagnifier(40, 70, start='rest', out_dtype='float64', **PY) as lm:
        assert lm.frames_seen == 0 and lm.state_bytes == 16 * 6 * sc.filtered_np(40, 70, 4, 2)
        whole = lm.push(v)
        assert isinstance(whole, np.ndarray) and whole.dtype == np.float64 and lm.frames_seen == len(v)
        assert np.array_equal(whole, f + raw)
        lm.reset()
        parts = [lm.push(v[0])] + [lm.push(v[k:k + 6]) for k in range(1, len(v), 6)]       # one [H,W] frame, then chunks
        assert parts[0].shape == (40, 70)
        assert np.array_equal(np.concatenate([parts[0][None]] + parts[1:]), whole)


def test_live_magnifier_numpy_and_tensor_round_trip():
    import torch
    from respmon_amd.live import LiveMagnifier
    v = sc.video(40, 70, np.uint8)
    with LiveMagnifier(40, 70, **PY) as lm:                      # steady start, uint8 in -> uint8 out
        whole = lm.push(v)
        assert isinstance(whole, np.ndarray) and whole.dtype == np.uint8 and whole.shape == v.shape
        lm.reset()
        d = torch.from_numpy(np.array(v)).cuda()
        outs = [lm.push(d[k:k + n]) for k, n in ((0, 1), (1, 2), (3, 7), (10, 9), (19, 1))]
        assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in outs)
        assert torch.equal(torch.cat(outs), torch.from_numpy(whole).cuda())
        assert lm.frames_seen == len(v)
    with LiveMagnifier(40, 70, out_dtype=np.float32, **PY) as lm:
        assert lm.push(v[:3]).dtype == np.float32
    with pytest.raises(ValueError):
        LiveMagnifier(40, 70, start='warm', **PY)
    with LiveMagnifier(40, 70, **PY) as lm, pytest.raises(ValueError):
        lm.push(np.zeros((2, 41, 70), np.uint8))


def test_live_magnifier_in_colour():
    from respmon_amd.live import LiveMagnifier
    v = sc.video(40, 70, "bgr")
    with LiveMagnifier(40, 70, color=True, **PY) as lm:
        whole = lm.push(v)
        assert whole.shape == v.shape and whole.dtype == np.uint8
        lm.reset()
        one = lm.push(v[0])
        assert one.shape == (40, 70, 3)
        rest = lm.push(v[1:])
        assert np.array_equal(np.concatenate([one[None], rest]), whole)
    from respmon_amd import transforms
    raw = transforms.eulerian_magnification_bandpass(v, sc.FPS, sc.BAND[0], sc.BAND[1], sc.AMP, pyramid_levels=4, skip_levels_at_top=2,
                                                     temporal_filter_function=transforms.temporal_bandpass_filter_sos)[1]
    with LiveMagnifier(40, 70, color=True, start='rest', **PY) as c:
        assert np.array_equal(c.push(v), sc.to_u8(v * (1.0 / 255) + raw[..., None]))      # the same raw onto the three channels
    with LiveMagnifier(40, 70, color=True, **PY) as lm, pytest.raises(ValueError):
        lm.push(sc.video(40, 70, np.uint8))
    with pytest.raises(TypeError):
        LiveMagnifier(40, 70, color=True, out_dtype='float64', **PY)


def test_temporal_bandpass_filter_sos_on_a_host_signal_goes_to_scipy():
    import scipy.signal
    from respmon_amd import transforms
    x = np.random.default_rng(5).random(300)
    sos = transforms.butter_bandpass_sos(0.1, 0.5, 30.0)
    assert sos.shape == (6, 6) and np.array_equal(sos, sc.butter_sos(6, 30.0, 0.1, 0.5))
    y = transforms.temporal_bandpass_filter_sos(x, 30.0, freq_min=0.1, freq_max=0.5, amplification_factor=50)
    assert isinstance(y, np.ndarray) and np.array_equal(y, scipy.signal.sosfilt(sos, x) * 50)
    x2 = np.random.default_rng(6).random((40, 5, 7))
    y2 = transforms.temporal_bandpass_filter_sos(x2, 30.0, freq_min=0.1, freq_max=0.5, amplification_factor=50)     # a video: the device
    assert isinstance(y2, np.ndarray) and np.array_equal(y2, sc.sos_restated(sos, x2, scale=50.0)[0])
    y3 = transforms.temporal_bandpass_filter_sos(x2, 30.0, freq_min=0.1, freq_max=0.5, amplification_factor=50, axis=2)
    assert np.array_equal(y3, scipy.signal.sosfilt(sos, x2, axis=2) * 50)
