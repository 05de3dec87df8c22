"""rm_magnify_bgr on the MI355X: the magnified video in colour (BGR frames in, BGR video out, respmon_amd/csrc/rm_magnify.h) against the
composition it replaces, formed on the device: raw of rm_eulerian_magnification_bandpass on the same RM_BGR8 buffer, then torch float64
arithmetic in the order of the definition -- `* (1./255)`, `+ raw`, clamp to [0, 1] -- and the library's own rm_float_to_uint8 for the
`* 255` and the truncation.  Small shapes as in tests/test_emu_magnify_bgr.py plus 1080p x 32, 720p x 16 and 1078 x 1918; unaligned
buffers, equal channels, the clamp, the workspace, the argument checks and the Python surface."""
import ctypes

import numpy as np
import pytest

from tests.test_emu_magnify import video
from tests.test_emu_magnify_bgr import CASES

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


def _big_video(T, H, W, seed):
    """The recipe of video(..., "bgr", seed) with the noise drawn on the device: a breathing gray clip, every channel moved by up to 20."""
    import torch
    from respmon_amd import synth
    gray = _dev(synth.synth_breathing(T, H, W, seed=seed))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    noise = torch.randint(-20, 21, (T, H, W, 3), device="cuda", generator=gen, dtype=torch.int16)
    return (gray.unsqueeze(-1).to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8).contiguous()


def _raw(hip, vid, L, S, amp=500.0):
    import torch
    from respmon_amd import _capi, device
    T, H, W = device.buffer_shape(vid)
    raw = torch.empty((T, H, W), dtype=torch.float64, device=vid.device)
    _capi.check(hip, hip.rm_eulerian_magnification_bandpass(device.ctx(), device.ptr(vid), _capi.RM_BGR8, T, H, W, 10.0, 0.1, 1.0, amp, L, S, 0.7, None,
                                                            device.ptr(raw), None, device.stream_ptr()), "bandpass")
    return raw


def _rc(hip, vid, out, L, S, amp=500.0, ctx=None):
    from respmon_amd import device
    T, H, W = device.buffer_shape(vid)
    return hip.rm_magnify_bgr(ctx or device.ctx(), device.ptr(vid), T, H, W, 10.0, 0.1, 1.0, amp, L, S, device.ptr(out), device.stream_ptr())


def _magnify_bgr(hip, vid, L, S, amp=500.0):
    import torch
    from respmon_amd import _capi
    out = torch.empty_like(vid)
    _capi.check(hip, _rc(hip, vid, out, L, S, amp), "rm_magnify_bgr")
    return out


def _definition(hip, vid, L, S, amp=500.0):
    """(want, the sum before the clamp) on the device."""
    from respmon_amd import transforms
    pre = vid.double() * (1.0 / 255) + _raw(hip, vid, L, S, amp).unsqueeze(-1)
    return transforms.float_to_uint8(pre.clamp(0.0, 1.0)), pre


def _check(hip, vid, L, S, amp=500.0):
    import torch
    want, pre = _definition(hip, vid, L, S, amp)
    got = _magnify_bgr(hip, vid, L, S, amp)
    assert got.shape == vid.shape and got.dtype == torch.uint8
    assert torch.equal(got, want), int((got.int() - want.int()).abs().max())
    return got, pre


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d_%dx%d_L%dS%d_%s" % c)
def test_magnify_bgr_equals_its_definition_bit_for_bit(hip, case):
    import torch
    T, H, W, L, S, path = case
    vid = _dev(video(T, H, W, "bgr", seed=T + H))
    got, pre = _check(hip, vid, L, S)
    if path == "zero":
        assert torch.equal(pre, vid.double() * (1.0 / 255))


@pytest.mark.parametrize("shape", [(32, 1080, 1920, 9, 4), (32, 1080, 1920, 4, 2), (16, 720, 1280, 9, 4), (16, 720, 1280, 4, 2), (12, 1078, 1918, 9, 4),
                                   (12, 1078, 1918, 4, 2)],
                         ids=["1080p_x32_L9S4", "1080p_x32_L4S2", "720p_x16_L9S4", "720p_x16_L4S2", "1078x1918_x12_L9S4", "1078x1918_x12_L4S2"])
def test_magnify_bgr_full_frames(hip, shape):
    """Checks 1-4 at full size: the definition, an unaligned output and frame buffer, equal channels, the clamp."""
    import torch
    from respmon_amd import _capi, device
    T, H, W, L, S = shape
    vid = _big_video(T, H, W, seed=5)
    assert bool((vid[..., 0] != vid[..., 1]).any()) and bool((vid[..., 1] != vid[..., 2]).any())
    got, _ = _check(hip, vid, L, S)
    # 2: the same buffers 1 and 8 bytes off a 16-byte boundary
    n = vid.numel()
    store_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    store_out = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    for off_in, off_out in [(1, 8), (8, 0), (0, 1)]:
        a_in = (-store_in.data_ptr()) % 16 + off_in
        a_out = (-store_out.data_ptr()) % 16 + off_out
        fin = store_in[a_in:a_in + n].view(vid.shape)
        fin.copy_(vid)
        store_out.zero_()
        fout = store_out[a_out:a_out + n].view(vid.shape)
        assert fin.data_ptr() % 16 == off_in and fout.data_ptr() % 16 == off_out
        _capi.check(hip, _rc(hip, fin, fout, L, S), "rm_magnify_bgr")
        assert torch.equal(fout, got), (off_in, off_out)
        assert not bool(store_out[:a_out].any()) and not bool(store_out[a_out + n:].any())
    del store_in, store_out, fin, fout
    # 3: equal channels are the gray video
    eq = vid[..., 1:2].expand(-1, -1, -1, 3).contiguous()
    g8 = torch.empty((T, H, W), dtype=torch.uint8, device="cuda")
    _capi.check(hip, hip.rm_magnify(device.ctx(), device.ptr(eq), _capi.RM_BGR8, T, H, W, 10.0, 0.1, 1.0, 500.0, L, S, device.ptr(g8), _capi.RM_U8,
                                    device.stream_ptr()), "rm_magnify")
    ge = _magnify_bgr(hip, eq, L, S)
    for c in range(3):
        assert torch.equal(ge[..., c], g8), c
    del eq, ge, g8
    # 4: the clamp, on both sides
    amp = 50000.0
    gc, pre = _check(hip, vid, L, S, amp=amp)
    assert float(pre.min()) < 0.0 and float(pre.max()) > 1.0   # not vacuous
    assert bool((gc == 0).any()) and bool((gc == 255).any())
    assert bool((gc[pre < 0] == 0).all()) and bool((gc[pre > 1] == 255).all())


def test_magnify_bgr_small_unaligned_equal_channels_and_clamp(hip):
    import torch
    from respmon_amd import _capi, device, synth
    T, H, W, L, S = 5, 32, 64, 4, 2
    vid = _dev(video(T, H, W, "bgr", seed=3))
    got, _ = _check(hip, vid, L, S)
    n = vid.numel()
    store_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    store_out = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    for off_in, off_out in [(0, 0), (1, 0), (0, 1), (8, 0), (0, 8), (1, 8), (8, 8)]:
        a_in = (-store_in.data_ptr()) % 16 + off_in
        a_out = (-store_out.data_ptr()) % 16 + off_out
        fin = store_in[a_in:a_in + n].view(vid.shape)
        fin.copy_(vid)
        store_out.zero_()
        fout = store_out[a_out:a_out + n].view(vid.shape)
        _capi.check(hip, _rc(hip, fin, fout, L, S), "rm_magnify_bgr")
        assert torch.equal(fout, got), (off_in, off_out)
        assert not bool(store_out[:a_out].any()) and not bool(store_out[a_out + n:].any())
    for Te, He, We, Le, Se in [(9, 48, 128, 4, 2), (6, 40, 70, 3, 1), (5, 20, 30, 3, 0), (5, 20, 30, 3, 2)]:
        eq = _dev(synth.synth_breathing(Te, He, We, seed=5)[..., None].repeat(3, -1))
        g8 = torch.empty((Te, He, We), dtype=torch.uint8, device="cuda")
        _capi.check(hip, hip.rm_magnify(device.ctx(), device.ptr(eq), _capi.RM_BGR8, Te, He, We, 10.0, 0.1, 1.0, 500.0, Le, Se, device.ptr(g8),
                                        _capi.RM_U8, device.stream_ptr()), "rm_magnify")
        ge = _magnify_bgr(hip, eq, Le, Se)
        for c in range(3):
            assert torch.equal(ge[..., c], g8), (Te, He, We, c)
    for Tc, Hc, Wc, Lc, Sc in [(9, 48, 128, 4, 2), (6, 40, 70, 4, 2), (5, 20, 30, 3, 0)]:
        v = _dev(video(Tc, Hc, Wc, "bgr", seed=8))
        gc, pre = _check(hip, v, Lc, Sc, amp=50000.0)
        assert float(pre.min()) < 0.0 and float(pre.max()) > 1.0
        assert bool((gc == 0).any()) and bool((gc == 255).any())


def test_magnify_bgr_nothing_filtered_is_not_an_identity_copy(hip):
    """skip >= levels - 1: float_to_uint8(uint8_to_float(k)) per byte, k - 1 on 24 of the 256 levels."""
    import torch
    from respmon_amd import transforms
    T, H, W = 3, 16, 64
    v = (np.arange(T * H * W * 3, dtype=np.int64) * 7 % 256).astype(np.uint8).reshape(T, H, W, 3)
    vid = _dev(v)
    got = _magnify_bgr(hip, vid, 3, 2)
    assert torch.equal(got, transforms.float_to_uint8(vid.double() * (1.0 / 255)))
    diff = v.astype(int) - got.cpu().numpy()
    assert set(np.unique(diff)) == {0, 1} and len(np.unique(v[diff == 1])) == 24


def test_magnify_bgr_without_a_full_size_float64_buffer(hip):
    """On a fresh context after a fused 1080p x 32 call the workspace is far below one [T,H,W] float64 array and neither materialised raw
    buffer exists; after a plain-path call behind S >= 1, magnify_raw does."""
    import torch
    from respmon_amd import _capi, device
    T, H, W = 32, 1080, 1920
    vid = _big_video(T, H, W, seed=6)
    out = torch.empty_like(vid)
    probe = np.empty(1)

    def has(ctx, name):
        rc = hip.rm_debug_workspace(ctx, name, ctypes.c_void_p(probe.ctypes.data), 8, device.stream_ptr())
        assert rc in (_capi.RM_OK, _capi.RM_E_BADARG)
        return rc == _capi.RM_OK

    ctx = ctypes.c_void_p()
    _capi.check(hip, hip.rm_ctx_create(torch.cuda.current_device(), ctypes.byref(ctx)), "ctx_create")
    try:
        _capi.check(hip, _rc(hip, vid, out, 9, 4, ctx=ctx), "rm_magnify_bgr")
        torch.cuda.synchronize()
        assert hip.rm_ctx_workspace_bytes(ctx) < T * H * W   # an eighth of one [T,H,W] float64 array
        assert not has(ctx, b"magnify_raw") and not has(ctx, b"raw_full")
        assert torch.equal(out, _magnify_bgr(hip, vid, 9, 4))
    finally:
        hip.rm_ctx_destroy(ctx)
    ctx = ctypes.c_void_p()
    _capi.check(hip, hip.rm_ctx_create(torch.cuda.current_device(), ctypes.byref(ctx)), "ctx_create")
    try:
        small = _dev(video(4, 70, 70, "bgr", seed=2))
        _capi.check(hip, _rc(hip, small, torch.empty_like(small), 7, 5, ctx=ctx), "rm_magnify_bgr")
        torch.cuda.synchronize()
        assert has(ctx, b"magnify_raw")
    finally:
        hip.rm_ctx_destroy(ctx)


def test_magnify_bgr_arguments(hip):
    import torch
    from respmon_amd import _capi, device
    vid = _dev(video(4, 16, 64, "bgr", seed=1))
    out = torch.zeros_like(vid)
    E = _capi.RM_E_BADARG
    c = device.ctx()

    def call(frames=device.ptr(vid), T=4, H=16, W=64, o=device.ptr(out), ctx=c, fps=10.0, levels=3, skip=1):
        return hip.rm_magnify_bgr(ctx, frames, T, H, W, fps, 0.1, 1.0, 500.0, levels, skip, o, device.stream_ptr())

    assert call() == _capi.RM_OK
    good = out.clone()
    assert torch.equal(good, _definition(hip, vid, 3, 1)[0])
    assert call(frames=None) == E and call(o=None) == E and call(ctx=None) == E
    assert call(T=0) == E and call(T=-3) == E and call(H=0) == E and call(W=0) == E
    assert call(levels=0) == E and call(skip=-1) == E and call(fps=0.0) == E and call(fps=float("nan")) == E
    assert call(T=4097) == _capi.RM_E_UNSUPPORTED
    n = vid.numel()
    assert call(o=device.ptr(vid)) == E
    assert b"overlap" in hip.rm_last_error_string()
    three = torch.zeros(3 * n, dtype=torch.uint8, device="cuda")
    three[n:2 * n] = vid.reshape(-1)
    base = three.data_ptr()
    mid = ctypes.c_void_p(base + n)
    assert call(frames=mid, o=ctypes.c_void_p(base + 2 * n - 1)) == E
    assert call(frames=mid, o=ctypes.c_void_p(base + 1)) == E
    assert call(frames=mid, o=ctypes.c_void_p(base + n + n // 3)) == E
    assert call(frames=mid, o=ctypes.c_void_p(base + 2 * n)) == _capi.RM_OK   # immediately after the frame buffer
    assert call(frames=mid, o=ctypes.c_void_p(base)) == _capi.RM_OK           # immediately before it
    assert torch.equal(three[2 * n:].view(vid.shape), good) and torch.equal(three[:n].view(vid.shape), good)
    assert torch.equal(three[n:2 * n].view(vid.shape), vid)
    g = torch.empty((4, 16, 64), dtype=torch.uint8, device="cuda")
    assert hip.rm_magnify(c, device.ptr(vid), _capi.RM_BGR8, 4, 16, 64, 10.0, 0.1, 1.0, 500.0, 3, 1, device.ptr(g), _capi.RM_BGR8, device.stream_ptr()) == E
    out.zero_()
    assert call() == _capi.RM_OK and torch.equal(out, good)   # the context still works
    assert hip.rm_abi_version() == 1


def test_python_surface_color(hip):
    import torch
    from respmon_amd import transforms
    v = video(9, 48, 128, "bgr", seed=2)
    vid = _dev(v)
    want = _magnify_bgr(hip, vid, 4, 2)
    got = transforms.eulerian_magnification_video(v, 10.0, 0.1, 1.0, 500.0, color=True)              # numpy in -> numpy out
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == v.shape and np.array_equal(got, want.cpu().numpy())
    got = transforms.eulerian_magnification_video(vid, 10.0, 0.1, 1.0, 500.0, color=True)            # tensor in -> tensor out
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, want)
    for od in ("uint8", np.uint8, torch.uint8, np.dtype("uint8")):
        assert torch.equal(transforms.eulerian_magnification_video(vid, 10.0, 0.1, 1.0, 500.0, out_dtype=od, color=True), want)
    got = transforms.eulerian_magnification_video(vid, 10.0, 0.1, 1.0, 500.0, pyramid_levels=6, skip_levels_at_top=3, color=True)
    assert torch.equal(got, _magnify_bgr(hip, vid, 6, 3))
    for od in ("float32", np.float64, torch.float32, "float16"):
        with pytest.raises(TypeError):
            transforms.eulerian_magnification_video(vid, 10.0, 0.1, 1.0, 500.0, out_dtype=od, color=True)
    gray = transforms.bgr_buffer_to_gray(vid)
    for bad in (gray, gray.double() * (1.0 / 255), vid[..., :2].contiguous(), gray.cpu().numpy()):
        with pytest.raises(ValueError):
            transforms.eulerian_magnification_video(bad, 10.0, 0.1, 1.0, 500.0, color=True)
    # the default is unchanged: the gray video, also for BGR input
    g8 = transforms.eulerian_magnification_video(vid, 10.0, 0.1, 1.0, 500.0)
    assert g8.shape == (9, 48, 128) and g8.dtype == torch.uint8
    assert torch.equal(g8, transforms.eulerian_magnification_video(gray, 10.0, 0.1, 1.0, 500.0))
    assert torch.equal(g8, transforms.eulerian_magnification_video(vid, 10.0, 0.1, 1.0, 500.0, color=False))


def test_monitor_magnified_calibration_video_color(hip):
    """A 'bgr8' monitor whose buffer was filled through store_frame: the method is the direct call on that buffer with locate()'s defaults;
    a gray buffer refuses color=True and names its dtype."""
    import torch
    from respmon_amd import transforms
    from respmon_amd.base import RespiratoryMonitor, _Backend
    frames = video(12, 144, 128, "bgr", seed=7)
    be = _Backend()

    def monitor(buffer_dtype, buf):
        mon = RespiratoryMonitor.__new__(RespiratoryMonitor)   # (no capture device: only the fields the method reads)
        mon.fps, mon.freq_min, mon.freq_max, mon.buffer_dtype = 10.0, 0.1, 1.0, buffer_dtype
        mon.calibration_buffer = buf
        return mon

    mon = monitor("bgr8", torch.zeros(frames.shape, dtype=torch.uint8, device="cuda"))
    for i, fr in enumerate(frames):
        bgr = _dev(fr)
        be.store_frame(mon.calibration_buffer, i, transforms.bgr_buffer_to_gray(bgr.unsqueeze(0))[0], bgr=bgr)
    assert torch.equal(mon.calibration_buffer, _dev(frames))
    got = mon.magnified_calibration_video(color=True)
    assert got.shape == frames.shape and got.dtype == torch.uint8
    assert torch.equal(got, _magnify_bgr(hip, mon.calibration_buffer, 9, 4))
    assert torch.equal(got, transforms.eulerian_magnification_video(mon.calibration_buffer, 10.0, 0.1, 1.0, 500, pyramid_levels=9, skip_levels_at_top=4,
                                                                    color=True))
    assert torch.equal(mon.magnified_calibration_video(out_dtype="uint8", color=True), got)
    with pytest.raises(TypeError):
        mon.magnified_calibration_video(out_dtype="float32", color=True)
    gray_video = mon.magnified_calibration_video()   # the default stays the gray video
    assert gray_video.shape == frames.shape[:3] and gray_video.dtype == torch.uint8
    for name, dt in (("uint8", torch.uint8), ("float64", torch.float64)):
        m = monitor(name, torch.zeros(frames.shape[:3], dtype=dt, device="cuda"))
        with pytest.raises(ValueError, match=name):
            m.magnified_calibration_video(color=True)
        assert m.magnified_calibration_video().dtype == dt
