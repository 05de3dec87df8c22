"""rm_magnify on the MI355X: the magnified video (frames + band-passed motion, respmon_amd/csrc/rm_magnify.h) against its definition
m[t] = f[t] + raw[t] -- raw from rm_eulerian_magnification_bandpass, bit for bit --, its output conversions, the reference's meaning
(transforms.py:170, 181 with the oracle), its argument checks and the Python surface.  Small shapes as in tests/test_emu_magnify.py plus
1080p x 64 and 720p x 32."""
import ctypes

import numpy as np
import pytest

from tests.test_emu_magnify import CASES, as_read, reference_magnified, video

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from respmon_amd import _capi
    return _capi.load()  # raises if the HIP extension is missing: no fallback


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(hip, vid, fps, fmin, fmax, amp, L, S):
    """raw_bandpassed_data of rm_eulerian_magnification_bandpass for a device frame buffer (no masked output)."""
    import torch
    from respmon_amd import _capi, device
    T, H, W = device.buffer_shape(vid)
    raw = torch.empty((T, H, W), dtype=torch.float64, device=vid.device)
    _capi.check(hip, hip.rm_eulerian_magnification_bandpass(device.ctx(), device.ptr(vid), device.buffer_dtype_code(vid), T, H, W, fps, fmin, fmax, amp,
                                                            L, S, 0.7, None, device.ptr(raw), None, device.stream_ptr()), "bandpass")
    return raw


def _magnify(hip, vid, fps, fmin, fmax, amp, L, S, out_dtype):
    import torch
    from respmon_amd import _capi, device
    T, H, W = device.buffer_shape(vid)
    code = {torch.uint8: _capi.RM_U8, torch.float32: _capi.RM_F32, torch.float64: _capi.RM_F64}[out_dtype]
    out = torch.empty((T, H, W), dtype=out_dtype, device=vid.device)
    _capi.check(hip, hip.rm_magnify(device.ctx(), device.ptr(vid), device.buffer_dtype_code(vid), T, H, W, fps, fmin, fmax, amp, L, S,
                                    device.ptr(out), code, device.stream_ptr()), "rm_magnify")
    return out


def _f(vid):
    """f: the frame buffer as the calibration reads it (device, float64)."""
    import torch
    from respmon_amd import transforms
    if vid.dim() == 4:
        vid = transforms.bgr_buffer_to_gray(vid)
    if vid.dtype == torch.uint8:
        return vid.double() * (1.0 / 255)
    return vid.double()


def _to_u8(m):
    from respmon_amd import transforms
    return transforms.float_to_uint8(m.clamp(0.0, 1.0))   # (torch.clamp keeps NaN)


def _check(hip, vid, L, S, fps=10.0, fmin=0.1, fmax=1.0, amp=500.0, equal_nan=False):
    import torch
    want = _f(vid) + _raw(hip, vid, fps, fmin, fmax, amp, L, S)
    m = _magnify(hip, vid, fps, fmin, fmax, amp, L, S, torch.float64)
    if equal_nan:
        assert bool(((m == want) | (m.isnan() & want.isnan())).all())
    else:
        assert torch.equal(m, want), float((m - want).abs().max())
    f32 = _magnify(hip, vid, fps, fmin, fmax, amp, L, S, torch.float32)
    w32 = want.float()
    assert bool(((f32 == w32) | (f32.isnan() & w32.isnan())).all())
    assert torch.equal(_magnify(hip, vid, fps, fmin, fmax, amp, L, S, torch.uint8), _to_u8(want))
    return m, want


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d_%dx%d_L%dS%d_%s_%s" % (c[0], c[1], c[2], c[3], c[4], getattr(c[5], "__name__", c[5]), c[6]))
def test_magnify_equals_its_definition_bit_for_bit(hip, case):
    import torch
    from respmon_amd import transforms
    T, H, W, L, S, dt, path = case
    vid = _dev(video(T, H, W, dt, seed=T + H))
    m, want = _check(hip, vid, L, S)
    if path == "zero":
        assert torch.equal(m, _f(vid))
    if dt == "bgr":
        assert torch.equal(_magnify(hip, transforms.bgr_buffer_to_gray(vid), 10.0, 0.1, 1.0, 500.0, L, S, torch.float64), m)


@pytest.mark.parametrize("shape", [(64, 1080, 1920, 9, 4), (32, 720, 1280, 4, 2)], ids=["1080p_x64_L9S4", "720p_x32_L4S2"])
def test_magnify_full_frames(hip, shape):
    import torch
    from respmon_amd import synth
    T, H, W, L, S = shape
    vid = _dev(synth.synth_breathing(T, H, W, seed=5))
    _check(hip, vid, L, S)
    if T == 32:   # every input dtype at 720p
        for dt in (torch.float16, torch.float32, torch.float64):
            _check(hip, (vid.double() * (1.0 / 255)).to(dt), L, S)
        _check(hip, vid.unsqueeze(-1).expand(-1, -1, -1, 3).contiguous(), L, S)


def test_magnify_without_a_full_size_float64_buffer(hip):
    """Peak extra device memory of the fused path is the calibration workspace plus the output: on a fresh context the workspace after a
    1080p x 64 call is far below one [T,H,W] float64 array, and neither materialised raw buffer exists."""
    import torch
    from respmon_amd import _capi, device, synth
    T, H, W = 64, 1080, 1920
    vid = _dev(synth.synth_breathing(T, H, W, seed=6))
    out = torch.empty((T, H, W), dtype=torch.uint8, device="cuda")
    ctx = ctypes.c_void_p()
    _capi.check(hip, hip.rm_ctx_create(torch.cuda.current_device(), ctypes.byref(ctx)), "ctx_create")
    try:
        _capi.check(hip, hip.rm_magnify(ctx, device.ptr(vid), _capi.RM_U8, T, H, W, 10.0, 0.1, 1.0, 500.0, 9, 4, device.ptr(out), _capi.RM_U8,
                                        device.stream_ptr()), "rm_magnify")
        torch.cuda.synchronize()
        assert hip.rm_ctx_workspace_bytes(ctx) < T * H * W   # an eighth of one [T,H,W] float64 array
        probe = np.empty(1)
        for name in (b"magnify_raw", b"raw_full"):
            assert hip.rm_debug_workspace(ctx, name, ctypes.c_void_p(probe.ctypes.data), 8, device.stream_ptr()) == _capi.RM_E_BADARG
        assert torch.equal(out, _magnify(hip, vid, 10.0, 0.1, 1.0, 500.0, 9, 4, torch.uint8))
    finally:
        hip.rm_ctx_destroy(ctx)


def test_magnify_non_finite_frames(hip):
    for S, L, shape in [(2, 4, (8, 40, 70)), (0, 3, (6, 20, 30)), (4, 6, (8, 80, 128))]:
        v = video(*shape, np.float64, seed=9)
        v[2, 5:9, 7:30] = np.nan
        v[3, 20:, :10] = np.inf
        v[5, :3, -4:] = -np.inf
        m, _ = _check(hip, _dev(v), L, S, equal_nan=True)
        assert bool(m.isnan().any())


def test_magnify_output_conversions_at_the_edges(hip):
    import torch
    special = np.array([-0.5, -1e-300, -0.0, 0.0, 1e-300, 0.5, 1.0 / 255, np.nextafter(1.0 / 255, 0), np.nextafter(1.0, 0), 1.0, np.nextafter(1.0, 2), 1.5,
                        254.0 / 255, 255.0 / 255, 2.0 ** -1074, 3e9, -3e9, 128.5 / 255])
    T, H, W = 4, 16, 64
    v = np.resize(special, (T, H, W)).astype(np.float64)
    for levels, skip, amp in [(3, 1, 0.0), (3, 2, 500.0), (5, 3, 0.0)]:   # raw is an exact zero: the values reach the converters unchanged
        vid = _dev(v)
        assert torch.equal(_magnify(hip, vid, 10.0, 0.1, 1.0, amp, levels, skip, torch.float64), vid)
        u8 = _magnify(hip, vid, 10.0, 0.1, 1.0, amp, levels, skip, torch.uint8).cpu().numpy()
        assert np.array_equal(u8, (np.clip(v, 0, 1) * 255).astype(np.uint8))     # transforms.py:26-29 on the clamped value
        assert np.array_equal(u8, _to_u8(vid).cpu().numpy())
        assert set(np.unique(u8)) >= {0, 127, 254, 255}
        assert torch.equal(_magnify(hip, vid, 10.0, 0.1, 1.0, amp, levels, skip, torch.float32), vid.float())
    vn = v.copy()
    vn[1, 3, 5] = np.nan
    u8 = _magnify(hip, _dev(vn), 10.0, 0.1, 1.0, 500.0, 3, 2, torch.uint8)
    assert int(u8[1, 3, 5]) == 0 and torch.equal(u8, _to_u8(_dev(vn)))


def test_magnify_means_what_the_reference_means(hip, oracle):
    """m against collapse(vid_pyramid) of the reference (transforms.py:170, 181), computed with the oracle alone.  d0 = max|ref - (f +
    raw_oracle)| / max|ref|, the cost of adding at full resolution instead of level by level, measured with the oracle on these inputs:
    3.8e-16, 6.5e-16, 3.4e-16.  Bound: 4 d0 + the 1e-11 * max|raw| tests/test_gpu_calibration.py allows between the device's raw and the
    oracle's, rescaled to max|ref|."""
    import torch
    from respmon_amd import synth
    for T, H, W, L, S in [(12, 48, 80, 4, 2), (10, 70, 100, 6, 4), (9, 40, 70, 3, 1)]:
        f = oracle.uint8_to_float(synth.synth_breathing(T, H, W, seed=L))
        ref = reference_magnified(oracle, f, 10.0, 0.1, 1.0, 500.0, L, S)
        raw_o = oracle.eulerian_magnification_bandpass(f.copy(), 10.0, 0.1, 1.0, 500.0, pyramid_levels=L, skip_levels_at_top=S)[1]
        scale = np.abs(ref).max()
        d0 = np.abs(ref - (f + raw_o)).max() / scale
        e_raw = 1e-11 * np.abs(raw_o).max() / scale
        m = _magnify(hip, _dev(f), 10.0, 0.1, 1.0, 500.0, L, S, torch.float64).cpu().numpy()
        err = np.abs(m - ref).max() / scale
        print("magnify vs reference: T%d %dx%d L%d S%d d0=%.3g e_raw=%.3g err=%.3g" % (T, H, W, L, S, d0, e_raw, err))
        assert 0 < d0 < 1e-14
        assert err <= 4 * d0 + e_raw, (T, H, W, L, S, err, d0, e_raw)


def test_magnify_arguments(hip):
    import torch
    from respmon_amd import _capi, device
    vid = _dev(video(4, 16, 64, np.uint8, seed=1))
    out = torch.zeros((4, 16, 64), dtype=torch.uint8, device="cuda")
    E = _capi.RM_E_BADARG
    c = device.ctx()

    def call(frames=device.ptr(vid), dtype=_capi.RM_U8, T=4, H=16, W=64, o=device.ptr(out), od=_capi.RM_U8, ctx=c, fps=10.0, levels=3, skip=1):
        return hip.rm_magnify(ctx, frames, dtype, T, H, W, fps, 0.1, 1.0, 500.0, levels, skip, o, od, device.stream_ptr())

    assert call() == _capi.RM_OK
    good = out.clone()
    for od in (_capi.RM_F16, _capi.RM_BGR8, 7, -1):
        assert call(od=od) == E
    assert call(o=device.ptr(vid)) == E
    assert b"overlap" in hip.rm_last_error_string()
    both = torch.zeros(2 * vid.numel(), dtype=torch.uint8, device="cuda")
    both[:vid.numel()] = vid.reshape(-1)
    assert call(frames=device.ptr(both), o=ctypes.c_void_p(both.data_ptr() + vid.numel() - 1)) == E
    assert call(frames=device.ptr(both), o=ctypes.c_void_p(both.data_ptr() + vid.numel())) == _capi.RM_OK
    assert torch.equal(both[vid.numel():].reshape(vid.shape), good)
    assert call(T=0) == E and call(T=-3) == E and call(H=0) == E and call(W=0) == E
    assert call(frames=None) == E and call(o=None) == E and call(ctx=None) == E
    assert call(dtype=9) == E and call(fps=0.0) == E and call(levels=0) == E and call(skip=-1) == E
    assert call(T=4097) == _capi.RM_E_UNSUPPORTED
    out.zero_()
    assert call() == _capi.RM_OK and torch.equal(out, good)   # the context still works
    assert hip.rm_abi_version() == 1


def test_python_surface(hip):
    import torch
    from respmon_amd import transforms
    v8 = video(9, 48, 128, np.uint8, seed=2)
    vid = _dev(v8)
    want8 = _magnify(hip, vid, 10.0, 0.1, 1.0, 500.0, 4, 2, torch.uint8)
    want64 = _magnify(hip, vid, 10.0, 0.1, 1.0, 500.0, 4, 2, torch.float64)
    got = transforms.eulerian_magnification_video(v8, 10.0, 0.1, 1.0, 500.0)                       # numpy in -> numpy out, uint8 by default
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want8.cpu().numpy())
    got = transforms.eulerian_magnification_video(vid, 10.0, 0.1, 1.0, 500.0, out_dtype="float64")   # tensor in -> tensor out
    assert isinstance(got, torch.Tensor) and got.is_cuda and torch.equal(got, want64)
    for od, td in [(np.float32, torch.float32), (torch.float64, torch.float64), (np.dtype("uint8"), torch.uint8), ("float32", torch.float32)]:
        got = transforms.eulerian_magnification_video(vid, 10.0, 0.1, 1.0, 500.0, out_dtype=od)
        assert got.dtype == td and torch.equal(got, _magnify(hip, vid, 10.0, 0.1, 1.0, 500.0, 4, 2, td))
    f64 = vid.double() * (1.0 / 255)
    got = transforms.eulerian_magnification_video(f64, 10.0, 0.1, 1.0, 500.0, pyramid_levels=5, skip_levels_at_top=3)   # float64 by default
    assert got.dtype == torch.float64 and torch.equal(got, _magnify(hip, f64, 10.0, 0.1, 1.0, 500.0, 5, 3, torch.float64))
    bgr = _dev(video(6, 40, 70, "bgr", seed=4))
    got = transforms.eulerian_magnification_video(bgr, 10.0, 0.1, 1.0, 500.0)
    assert got.dtype == torch.uint8 and torch.equal(got, _magnify(hip, transforms.bgr_buffer_to_gray(bgr), 10.0, 0.1, 1.0, 500.0, 4, 2, torch.uint8))
    with pytest.raises(TypeError):
        transforms.eulerian_magnification_video(vid, 10.0, 0.1, 1.0, 500.0, out_dtype="float16")


def test_monitor_magnified_calibration_video(hip):
    """A monitor whose buffer was filled through store_frame: the method is the function on that buffer with locate()'s defaults."""
    import torch
    from respmon_amd import transforms
    from respmon_amd.base import RespiratoryMonitor, _Backend
    frames = video(12, 144, 128, np.uint8, seed=7)
    be = _Backend()
    for dt in (torch.float64, torch.uint8):
        mon = RespiratoryMonitor.__new__(RespiratoryMonitor)   # (no capture device: only the fields the method reads)
        mon.fps, mon.freq_min, mon.freq_max = 10.0, 0.1, 1.0
        mon.calibration_buffer = torch.zeros(frames.shape, dtype=dt, device="cuda")
        for i, fr in enumerate(frames):
            be.store_frame(mon.calibration_buffer, i, _dev(fr))
        got = mon.magnified_calibration_video()
        want = transforms.eulerian_magnification_video(mon.calibration_buffer, 10.0, 0.1, 1.0, 500, pyramid_levels=9, skip_levels_at_top=4)
        assert got.dtype == dt and torch.equal(got, want)
        assert torch.equal(mon.magnified_calibration_video(out_dtype="float32"),
                           _magnify(hip, mon.calibration_buffer, 10.0, 0.1, 1.0, 500.0, 9, 4, torch.float32))
