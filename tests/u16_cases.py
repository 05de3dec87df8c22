"""Shared by tests/test_emu_u16.py and tests/test_gpu_u16.py (not a test module): uint16 frame buffers (RM_U16, include/respmon_hip.h)
through the C-ABI on raw pointers.  A backend `be` hides where the memory lives, as in tests/window_cases.py:
    be.lib, be.ctx, be.stream()          the bound library, a context, the stream argument
    be.dev(ndarray) -> buffer            an array where the library reads / writes it (numpy itself on the host-emulated build, a tensor
                                         on the GPU);  be.p(buffer) -> c_void_p its address;  be.np(buffer) -> ndarray its host copy

The contract under test: every entry point given an RM_U16 buffer returns, bit for bit, what the same call returns on the RM_F64 buffer
that holds k * (1./65535).  Every comparison is exact, so there is no tolerance anywhere in this file."""
import ctypes

import numpy as np

from respmon_amd import _capi, synth

SCALE = 1. / 65535
KW = dict(fps=10.0, fmin=0.1, fmax=1.0, amp=500.0, thr=0.7, threshold=20)
U16, F64, U8, F32 = _capi.RM_U16, _capi.RM_F64, _capi.RM_U8, _capi.RM_F32
CODE = {np.dtype(np.uint16): U16, np.dtype(np.float64): F64, np.dtype(np.uint8): U8, np.dtype(np.float32): F32}
NP_OF = {U16: np.uint16, F64: np.float64, U8: np.uint8, F32: np.float32}


def widen(v):
    """uint16_to_float with numpy: the float64 buffer the contract compares against"""
    assert v.dtype == np.uint16
    return v.astype(np.float64) * SCALE


def hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def ck(be, rc, what):
    return _capi.check(be.lib, rc, what)


_VIDEOS = {}


def random_u16(T, H, W, seed):
    """full-range random uint16 (made once per shape, read-only)"""
    key = ("rand", T, H, W, seed)
    if key not in _VIDEOS:
        v = np.random.default_rng(seed).integers(0, 65536, size=(T, H, W), dtype=np.uint16)
        v.setflags(write=False)
        _VIDEOS[key] = v
    return _VIDEOS[key]


def every_level():
    """one 256 x 256 frame that holds each of the 65 536 levels once, shuffled"""
    if "levels" not in _VIDEOS:
        v = np.random.default_rng(16).permutation(65536).astype(np.uint16).reshape(1, 256, 256)
        v.setflags(write=False)
        _VIDEOS["levels"] = v
    return _VIDEOS["levels"]


def breathing16(T, H, W, bits=16, seed=7):
    key = ("breath", T, H, W, bits, seed)
    if key not in _VIDEOS:
        v = synth.synth_breathing16(T, H, W, seed=seed, bits=bits)
        v.setflags(write=False)
        _VIDEOS[key] = v
    return _VIDEOS[key]


# ---- thin callers ---------------------------------------------------------------------------------------------------------------
def calibrate(be, frames, L, S, flags=0):
    """rm_calibrate -> (heat [H,W], (min, max))"""
    T, H, W = frames.shape
    d = be.dev(frames)
    heat = be.dev(np.full((H, W), np.nan))
    mm = np.full(2, np.nan)
    ck(be, be.lib.rm_calibrate(be.ctx, be.p(d), CODE[frames.dtype], T, H, W, KW["fps"], KW["fmin"], KW["fmax"], KW["amp"], L, S, KW["thr"],
                               flags, be.p(heat), hp(mm), be.stream()), "rm_calibrate")
    return be.np(heat), mm


def front_rows(be, frames, L, S, flags=0):
    """rm_shard_pyramid: the rows the front half hands to the temporal filter (G_S, or the Laplacian levels) -- the direct output of the
    kernels that read the frame buffer"""
    T, H, W = frames.shape
    n = ctypes.c_size_t()
    ck(be, be.lib.rm_shard_layout_flags(H, W, L, S, flags, ctypes.byref(n)), "rm_shard_layout_flags")
    NP = int(n.value)
    if NP == 0:
        return np.zeros((T, 0))
    d = be.dev(frames)
    lap = be.dev(np.full((T, NP), np.nan))
    ck(be, be.lib.rm_shard_pyramid(be.ctx, be.p(d), CODE[frames.dtype], T, H, W, L, S, flags, be.p(lap), be.stream()), "rm_shard_pyramid")
    return be.np(lap)


def locate(be, frames, L, S, flags=0):
    T, H, W = frames.shape
    d = be.dev(frames)
    xywh = np.zeros(4, np.int32)
    rc = ck(be, be.lib.rm_locate(be.ctx, be.p(d), CODE[frames.dtype], T, H, W, KW["fps"], KW["fmin"], KW["fmax"], KW["amp"], L, S, KW["thr"],
                                 KW["threshold"], flags, hp(xywh), be.stream()), "rm_locate")
    return None if rc == _capi.RM_NO_CONTOUR else tuple(int(v) for v in xywh)


def magnify_rc(be, frames, L, S, out_code, amp=20.0):
    T, H, W = frames.shape[:3]
    d = be.dev(frames)
    out = be.dev(np.zeros((T, H, W), NP_OF[out_code]))
    rc = be.lib.rm_magnify(be.ctx, be.p(d), _capi.RM_BGR8 if frames.ndim == 4 else CODE[frames.dtype], T, H, W, KW["fps"], KW["fmin"],
                           KW["fmax"], amp, L, S, be.p(out), out_code, be.stream())
    return rc, out


def magnify(be, frames, L, S, out_code, amp=20.0):
    rc, out = magnify_rc(be, frames, L, S, out_code, amp)
    ck(be, rc, "rm_magnify")
    return be.np(out)


def u16_of(m):
    """rm_magnify's RM_U16 output of the float64 output m: the clamp to [0, 1], then the C truncation of m * 65535"""
    return (np.clip(m, 0.0, 1.0) * 65535).astype(np.int64).astype(np.uint16)


class Stream:
    def __init__(self, be, H, W, L, S, amp=20.0):
        self.be = be
        sos = _sos()
        self.h = ctypes.c_void_p()
        ck(be, be.lib.rm_stream_create(be.ctx, H, W, L, S, hp(sos), sos.shape[0], None, amp, ctypes.byref(self.h)), "rm_stream_create")

    def push(self, frames, out_code):
        n, H, W = frames.shape
        d = self.be.dev(frames)
        out = self.be.dev(np.zeros((n, H, W), NP_OF[out_code]))
        ck(self.be, self.be.lib.rm_stream_push(self.be.ctx, self.h, self.be.p(d), CODE[frames.dtype], n, self.be.p(out), out_code,
                                               self.be.stream()), "rm_stream_push")
        return self.be.np(out)

    def close(self):
        self.be.lib.rm_stream_destroy(self.h)


def _sos():
    import scipy.signal
    nyq = KW["fps"] / 2
    return np.ascontiguousarray(scipy.signal.butter(6, [KW["fmin"] / nyq, KW["fmax"] / nyq], btype='band', output='sos'))


# ---- 1. conversions -------------------------------------------------------------------------------------------------------------
def check_conversions(be):
    k = np.arange(65536, dtype=np.uint16)
    want = k.astype(np.float64) * SCALE
    out, dk = be.dev(np.full(65536, np.nan)), be.dev(k)
    ck(be, be.lib.rm_uint16_to_float(be.ctx, be.p(dk), be.p(out), k.size, be.stream()), "rm_uint16_to_float")
    got = be.np(out)
    assert np.array_equal(got, want)
    # why no kernel may take a float32 shortcut: all but two of these values (0 and 1) change when they pass through a float
    assert int(np.count_nonzero(want.astype(np.float32).astype(np.float64) != want)) == 65534
    # the way back: v * 65535, C truncation, low 16 bits; NaN and products outside int32 give 0
    v = np.concatenate([want, [0.0, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), -0.0, 0.5, 1.5, -0.25, 2.0, np.nan, 1e12, -1e12,
                               32767.9 / 65535, 40000.0, -40000.0]])
    prod = v * 65535
    ok = np.isfinite(prod) & (prod < 2147483648.0) & (prod > -2147483649.0)
    ref = np.where(ok, np.where(ok, prod, 0.0).astype(np.int64) & 65535, 0).astype(np.uint16)
    back, dv = be.dev(np.full(v.size, 0xdead, np.uint16)), be.dev(v)
    ck(be, be.lib.rm_float_to_uint16(be.ctx, be.p(dv), be.p(back), v.size, be.stream()), "rm_float_to_uint16")
    assert np.array_equal(be.np(back), ref)
    assert int(ref[65536]) == 0 and int(ref[65537]) == 65535 and int(ref[65536 + 9]) == 0 and int(ref[65536 + 10]) == 0 and int(ref[65536 + 11]) == 0
    return be.np(back)[:65536]    # u16(k * (1./65535) * 65535) per level: what an unfiltered uint16 -> uint16 magnification must give


# ---- 2. calibration -------------------------------------------------------------------------------------------------------------
def check_calibration(be, T, H, W, L, S, flags=0, frames=None):
    """heat map, min / max and (skip >= 1) the front half's rows of the RM_U16 buffer against those of the RM_F64 buffer of k * (1./65535)"""
    v = random_u16(T, H, W, seed=1000 * L + S) if frames is None else frames
    f = widen(v)
    if S >= 1:
        rows16, rows64 = front_rows(be, v, L, S, flags), front_rows(be, f, L, S, flags)
        assert rows64.size == 0 or (np.isfinite(rows64).all() and np.ptp(rows64) > 0)
        assert np.array_equal(rows16, rows64), (T, H, W, L, S, flags)
    heat16, mm16 = calibrate(be, v, L, S, flags)
    heat64, mm64 = calibrate(be, f, L, S, flags)
    assert np.array_equal(heat16, heat64, equal_nan=True), (T, H, W, L, S, flags)
    assert np.array_equal(mm16, mm64, equal_nan=True), (T, H, W, L, S, flags)
    return heat16


def check_flags_against_one_another(be, T, H, W, L, S):
    """the flag relations tests/test_gpu_calibration.py states for the other dtypes, on a uint16 buffer"""
    v = random_u16(T, H, W, seed=1000 * L + S)
    per_level = calibrate(be, v, L, S, 2)[0]
    assert np.array_equal(per_level, calibrate(be, widen(v), L, S, 2)[0], equal_nan=True)
    for fl in (64, 64 | 8, 16):
        assert np.array_equal(calibrate(be, v, L, S, fl)[0], per_level, equal_nan=True), (fl, T, H, W, L, S)
    ff = calibrate(be, v, L, S, 0)[0]
    assert np.array_equal(calibrate(be, v, L, S, 1)[0], ff, equal_nan=True)      # pruning never changes a bit
    assert np.array_equal(calibrate(be, v, L, S, 8)[0], ff, equal_nan=True)      # nor does the strip geometry
    scale = np.abs(per_level).max()
    assert np.abs(ff - per_level).max() <= 1e-9 * scale      # (the same linear map in another order: tests/test_gpu_calibration.py _close)


# ---- 3. the two-call form against the CPU oracle ----------------------------------------------------------------------------------
def check_locate_oracle(be, T, H, W, L, S, seed=7):
    from oracle import respmon_oracle as oracle
    v16 = breathing16(T, H, W, 16, seed)
    ref = oracle.locate(widen(v16), KW["fps"], pyramid_levels=L, skip_levels_at_top=S)
    assert ref is not None
    assert locate(be, v16, L, S) == tuple(ref)
    # a 12-bit camera, samples right-aligned or shifted left by 4: the same ROI, and a heat map scaled by 2^4 bit for bit
    v12 = breathing16(T, H, W, 12, seed)
    v12s = (v12 << np.uint16(4)).astype(np.uint16)
    ref12 = oracle.locate(widen(v12), KW["fps"], pyramid_levels=L, skip_levels_at_top=S)
    assert ref12 is not None
    assert locate(be, v12, L, S) == tuple(ref12) == locate(be, v12s, L, S)
    h12, hs = calibrate(be, v12, L, S)[0], calibrate(be, v12s, L, S)[0]
    assert np.ptp(h12) > 0 and np.array_equal(hs, 16.0 * h12)
    return tuple(ref)


# ---- 4. motion ------------------------------------------------------------------------------------------------------------------
def motion_rois(H, W):
    """odd offsets and sizes, a rectangle that touches the right and bottom edges, the 1 x 1 rectangle, the whole frame"""
    return [(3, 5, 17, 11), (W - 9, H - 7, 9, 7), (W // 2, H // 3, 1, 1), (0, 0, W, H), (1, 1, W - 2, 1)]


def roi_means(be, frames, roi):
    """(rm_roi_mean of every frame, rm_roi_mean_clip, rm_roi_mean_multi_clip with that one rectangle)"""
    N, H, W = frames.shape
    x, y, w, h = roi
    d = be.dev(frames)
    code, esz = CODE[frames.dtype], frames.dtype.itemsize
    single = np.full(N, np.nan)
    for i in range(N):
        o = ctypes.c_double(np.nan)
        fp = ctypes.c_void_p(be.p(d).value + i * H * W * esz)
        ck(be, be.lib.rm_roi_mean(be.ctx, fp, code, H, W, x, y, w, h, ctypes.byref(o), be.stream()), "rm_roi_mean")
        single[i] = o.value
    clip = np.full(N, np.nan)
    ck(be, be.lib.rm_roi_mean_clip(be.ctx, be.p(d), code, N, H, W, x, y, w, h, hp(clip), be.stream()), "rm_roi_mean_clip")
    multi = np.full((N, 2), np.nan)
    rois = np.array([roi, (0, 0, W, H)], np.int32)
    ck(be, be.lib.rm_roi_mean_multi_clip(be.ctx, be.p(d), code, N, H, W, hp(rois), 2, hp(multi), be.stream()), "rm_roi_mean_multi_clip")
    return single, clip, multi


def roi_crop_u8(be, frame, roi):
    H, W = frame.shape
    x, y, w, h = roi
    dst, d = be.dev(np.zeros((h, w), np.uint8)), be.dev(frame)
    ck(be, be.lib.rm_roi_to_uint8(be.ctx, be.p(d), CODE[frame.dtype], H, W, x, y, w, h, be.p(dst), be.stream()), "rm_roi_to_uint8")
    return be.np(dst)


def check_motion(be, H=45, W=67):
    from oracle import respmon_oracle as oracle
    v = random_u16(3, H, W, seed=44)
    f = widen(v)
    for roi in motion_rois(H, W):
        a, b = roi_means(be, v, roi), roi_means(be, f, roi)
        for got, want in zip(a, b):
            assert np.isfinite(want).all() and np.array_equal(got, want), roi
        x, y, w, h = roi
        assert np.array_equal(roi_crop_u8(be, v[0], roi), oracle.float_to_uint8(f[0, y:y + h, x:x + w])), roi
        assert np.array_equal(roi_crop_u8(be, v[0], roi), roi_crop_u8(be, f[0], roi)), roi


def flow_run(be, frames, roi, split=None):
    """rm_flow_begin on frame 0, rm_flow_clip over the rest (in two calls when `split`) -> (corners, means, good counts, end points)"""
    N, H, W = frames.shape
    x, y, w, h = roi
    d = be.dev(frames)
    code, esz = CODE[frames.dtype], frames.dtype.itemsize
    st = ctypes.c_void_p()
    ck(be, be.lib.rm_flow_state_create(be.ctx, ctypes.byref(st)), "rm_flow_state_create")
    try:
        pts = np.zeros((100, 2), np.float32)
        n = ctypes.c_int()
        ck(be, be.lib.rm_flow_begin(be.ctx, st, be.p(d), code, H, W, x, y, w, h, 100, 0.3, 7.0, 7, hp(pts), ctypes.byref(n), be.stream()), "rm_flow_begin")
        mean = np.full((N - 1, 2), np.nan, np.float32)
        good = np.full(N - 1, -1, np.int32)
        cuts = [1, N] if not split else [1, split, N]
        for a, b in zip(cuts, cuts[1:]):
            fp = ctypes.c_void_p(be.p(d).value + a * H * W * esz)
            ck(be, be.lib.rm_flow_clip(be.ctx, st, fp, code, b - a, H, W, x, y, w, h, 15, 15, 2, 10, 0.03, hp(mean[a - 1:]), hp(good[a - 1:]), be.stream()),
               "rm_flow_clip")
        end = np.zeros((100, 2), np.float32)
        m = ctypes.c_int()
        ck(be, be.lib.rm_flow_points(be.ctx, st, hp(end), 100, ctypes.byref(m), be.stream()), "rm_flow_points")
        # one more single step on the last frame: the state the clip left is usable by rm_flow_step
        sm = np.full(2, np.nan, np.float32)
        sg = ctypes.c_int(-1)
        fp = ctypes.c_void_p(be.p(d).value + (N - 1) * H * W * esz)
        ck(be, be.lib.rm_flow_step(be.ctx, st, fp, code, H, W, x, y, w, h, 15, 15, 2, 10, 0.03, hp(sm), ctypes.byref(sg), be.stream()), "rm_flow_step")
        return pts[:n.value].copy(), mean, good, end[:min(m.value, 100)].copy(), sm, sg.value
    finally:
        be.lib.rm_flow_state_destroy(st)


def flow_clip_video(N=5, H=96, W=128):
    """a textured 16-bit clip that drifts by a fraction of a pixel per frame: corners to find and to follow"""
    if "flow" not in _VIDEOS:
        render = synth.synth_texture(H, W, seed=5)
        hi = np.stack([render(0.4 * i, 0.25 * i) for i in range(N)]).astype(np.uint16)
        lo = np.random.default_rng(6).integers(0, 256, size=hi.shape, dtype=np.uint16)
        v = (hi << np.uint16(8)) | lo
        v.setflags(write=False)
        _VIDEOS["flow"] = v
    return _VIDEOS["flow"]


def check_flow_clip(be):
    v = flow_clip_video()
    roi = (21, 13, 80, 64)
    a, b = flow_run(be, v, roi), flow_run(be, widen(v), roi)
    assert len(a[0]) >= 4 and (a[2] > 0).all()
    for got, want in zip(a, b):
        assert np.array_equal(got, want)
    for got, want in zip(flow_run(be, v, roi, split=3), a):
        assert np.array_equal(got, want)


# ---- 5. magnify and stream ------------------------------------------------------------------------------------------------------
def check_magnify(be, T, H, W, L, S, identity):
    v = breathing16(T, H, W, 16, seed=21)
    m16, m64 = magnify(be, v, L, S, F64), magnify(be, widen(v), L, S, F64)
    assert np.isfinite(m64).all() and np.array_equal(m16, m64)
    out = magnify(be, v, L, S, U16)
    assert out.dtype == np.uint16 and np.array_equal(out, u16_of(m64))
    assert np.array_equal(magnify(be, widen(v), L, S, U16), out)          # RM_U16 output from another input dtype
    assert np.array_equal(magnify(be, v, L, S, F32), m64.astype(np.float32))
    # nothing filtered (skip >= levels - 1): the rule per level, which the caller computed with rm_float_to_uint16 and numpy
    plain = magnify(be, v, S + 1, S, U16)
    assert np.array_equal(plain, identity[v])
    assert np.array_equal(plain, u16_of(widen(v)))


def check_magnify_clamp(be):
    """a strong amplification drives pixels out of [0, 1]: the uint16 output clamps instead of wrapping around"""
    v = breathing16(8, 40, 80, 16, seed=21)
    m64 = magnify(be, widen(v), 5, 3, F64, amp=4000.0)
    assert (m64 > 1.0).any() and (m64 < 0.0).any()
    out = magnify(be, v, 5, 3, U16, amp=4000.0)
    assert np.array_equal(out, u16_of(m64)) and (out == 65535).any() and (out == 0).any()


def check_stream(be, H=40, W=80, L=5, S=3):
    v = breathing16(11, H, W, 16, seed=23)
    runs = {}
    for name, frames, out_code, cuts in (("u16 one", v, F64, [0, 11]), ("u16 two", v, F64, [0, 4, 11]), ("f64 one", widen(v), F64, [0, 11]),
                                         ("u16 out", v, U16, [0, 7, 11])):
        st = Stream(be, H, W, L, S)
        try:
            runs[name] = np.concatenate([st.push(np.ascontiguousarray(frames[a:b]), out_code) for a, b in zip(cuts, cuts[1:])])
        finally:
            st.close()
    assert np.isfinite(runs["f64 one"]).all() and np.ptp(runs["f64 one"] - widen(v)) > 0
    assert np.array_equal(runs["u16 one"], runs["f64 one"]) and np.array_equal(runs["u16 two"], runs["u16 one"])
    assert np.array_equal(runs["u16 out"], u16_of(runs["f64 one"]))


# ---- 6. arguments ---------------------------------------------------------------------------------------------------------------
def check_arguments(be):
    """RM_U16 is refused nowhere a gray dtype is taken; the colour forms stay uint8-only; 5, 7 and 9 are still no dtype"""
    lib, ctx, s = be.lib, be.ctx, be.stream()
    assert lib.rm_abi_version() == 1 and _capi.RM_U16 == 6
    T, H, W, L, S = 4, 32, 48, 3, 1
    v = random_u16(T, H, W, seed=9)
    d = be.dev(v)
    NPIX = H * W
    keep = []     # every buffer a call is handed stays alive until the checks are over

    def f64(*shape, dtype=np.float64):
        keep.append(be.dev(np.zeros(shape, dtype)))
        return keep[-1]
    heat, mm, xywh, n = f64(H, W), np.zeros(2), np.zeros(8, np.int32), ctypes.c_int()
    area = np.zeros(2)
    kw = (KW["fps"], KW["fmin"], KW["fmax"], KW["amp"])

    def calls(code):
        """every gray entry point with dtype `code` on the same 2-byte buffer -> {name: return code}"""
        r = {}
        r["rm_pyr_down"] = lib.rm_pyr_down(ctx, be.p(d), code, T, H, W, be.p(f64(T, (H + 1) // 2, (W + 1) // 2)), s)
        lv = [f64(T, (H + (1 << k) - 1) >> k, (W + (1 << k) - 1) >> k) for k in range(L)]
        ptrs = (ctypes.c_void_p * L)(*[be.p(a).value for a in lv])
        r["rm_create_laplacian_video_pyramid"] = lib.rm_create_laplacian_video_pyramid(ctx, be.p(d), code, T, H, W, L, ptrs, s)
        r["rm_time_average"] = lib.rm_time_average(ctx, be.p(d), code, T, NPIX, be.p(f64(H, W)), s)
        r["rm_calibrate"] = lib.rm_calibrate(ctx, be.p(d), code, T, H, W, *kw, L, S, 0.7, 0, be.p(heat), hp(mm), s)
        r["rm_locate"] = lib.rm_locate(ctx, be.p(d), code, T, H, W, *kw, L, S, 0.7, 20, 0, hp(xywh), s)
        tk = ctypes.c_int(-1)
        rc = lib.rm_locate_submit(ctx, be.p(d), code, T, H, W, *kw, L, S, 0.7, 20, 0, s, ctypes.byref(tk))
        if rc >= 0:
            rc = lib.rm_locate_result(ctx, tk.value, hp(xywh))
        r["rm_locate_submit"] = rc
        r["rm_locate_multi"] = lib.rm_locate_multi(ctx, be.p(d), code, T, H, W, *kw, L, S, 0.7, 20, 0, 2, 0.0, hp(xywh), hp(area), ctypes.byref(n), s)
        r["rm_eulerian_magnification_bandpass"] = lib.rm_eulerian_magnification_bandpass(ctx, be.p(d), code, T, H, W, *kw, L, S, 0.7, be.p(f64(T, H, W)),
                                                                                         be.p(f64(T, H, W)), hp(mm), s)
        r["rm_magnify"] = lib.rm_magnify(ctx, be.p(d), code, T, H, W, *kw, L, S, be.p(f64(T, H, W)), F64, s)
        sz = ctypes.c_size_t()
        lib.rm_shard_layout_flags(H, W, L, S, 0, ctypes.byref(sz))
        r["rm_shard_pyramid"] = lib.rm_shard_pyramid(ctx, be.p(d), code, T, H, W, L, S, 0, be.p(f64(T, sz.value)), s)
        ex = ctypes.c_int()
        if getattr(be, "comm", True):
            r["rm_locate_streams"] = lib.rm_locate_streams(ctx, be.p(d), code, T, H, W, *kw, L, S, 0.7, 20, 0, be.p(heat), hp(xywh), ctypes.byref(ex), s)
            r["rm_locate_sharded"] = lib.rm_locate_sharded(ctx, be.p(d), code, T, H, W, *kw, L, S, 0.7, 20, 0, be.p(heat), hp(xywh), ctypes.byref(ex), s)
        win = ctypes.c_void_p()
        ck(be, lib.rm_window_create(ctx, T, H, W, L, S, 0, ctypes.byref(win)), "rm_window_create")
        r["rm_window_push"] = lib.rm_window_push(ctx, win, be.p(d), code, T, s)
        lib.rm_window_destroy(win)
        st = Stream(be, H, W, L, S)
        r["rm_stream_push"] = lib.rm_stream_push(ctx, st.h, be.p(d), code, T, be.p(f64(T, H, W)), F64, s)
        st.close()
        h1, w1 = (H + 1) // 2, (W + 1) // 2
        r["rm_rate_map"] = lib.rm_rate_map(ctx, be.p(d), code, T, H, W, 1, KW["fps"], KW["fmin"], KW["fmax"], 16, be.p(f64(h1, w1)), be.p(f64(h1, w1)),
                                           be.p(f64(h1, w1)), be.p(f64(h1, w1, dtype=np.int32)), s)
        o = ctypes.c_double()
        r["rm_roi_mean"] = lib.rm_roi_mean(ctx, be.p(d), code, H, W, 1, 1, 5, 5, ctypes.byref(o), s)
        r["rm_roi_mean_clip"] = lib.rm_roi_mean_clip(ctx, be.p(d), code, T, H, W, 1, 1, 5, 5, hp(np.zeros(T)), s)
        roi = np.array([[1, 1, 5, 5]], np.int32)
        r["rm_roi_mean_multi_clip"] = lib.rm_roi_mean_multi_clip(ctx, be.p(d), code, T, H, W, hp(roi), 1, hp(np.zeros(T)), s)
        r["rm_roi_to_uint8"] = lib.rm_roi_to_uint8(ctx, be.p(d), code, H, W, 1, 1, 5, 5, be.p(f64(5, 5, dtype=np.uint8)), s)
        fs = ctypes.c_void_p()
        ck(be, lib.rm_flow_state_create(ctx, ctypes.byref(fs)), "rm_flow_state_create")
        pts, mean, good = np.zeros((100, 2), np.float32), np.zeros((T, 2), np.float32), np.zeros(T, np.int32)
        roi2 = np.array([[0, 0, W, H]], np.int32)
        r["rm_flow_begin"] = lib.rm_flow_begin(ctx, fs, be.p(d), code, H, W, 0, 0, W, H, 100, 0.3, 7.0, 7, hp(pts), ctypes.byref(n), s)
        if code != U16:    # the refusals below are about the dtype: give them a session that has begun
            ck(be, lib.rm_flow_begin(ctx, fs, be.p(d), U16, H, W, 0, 0, W, H, 100, 0.3, 7.0, 7, hp(pts), ctypes.byref(n), s), "rm_flow_begin")
        r["rm_flow_step"] = lib.rm_flow_step(ctx, fs, be.p(d), code, H, W, 0, 0, W, H, 15, 15, 2, 10, 0.03, hp(mean), ctypes.byref(n), s)
        r["rm_flow_clip"] = lib.rm_flow_clip(ctx, fs, be.p(d), code, T, H, W, 0, 0, W, H, 15, 15, 2, 10, 0.03, hp(mean), hp(good), s)
        states = (ctypes.c_void_p * 1)(fs.value)
        r["rm_flow_multi_clip"] = lib.rm_flow_multi_clip(ctx, states, be.p(d), code, T, H, W, hp(roi2), 1, 15, 15, 2, 10, 0.03, hp(mean), hp(good), s)
        lib.rm_flow_state_destroy(fs)
        return r

    got = calls(U16)
    assert all(rc >= 0 for rc in got.values()), {k: rc for k, rc in got.items() if rc < 0}
    assert len(got) >= 21
    for bad in (5, 7, 9):
        refused = calls(bad)
        assert all(rc == _capi.RM_E_BADARG for rc in refused.values()), (bad, {k: rc for k, rc in refused.items() if rc != _capi.RM_E_BADARG})
    # output dtypes: rm_magnify and the gray stream write RM_U16; 5 / 7 / 9 are no output dtype; colour stays uint8
    assert magnify_rc(be, v, L, S, U16)[0] == _capi.RM_OK
    for bad in (5, 7, 9, _capi.RM_F16, _capi.RM_BGR8):
        assert lib.rm_magnify(ctx, be.p(d), U16, T, H, W, *kw, L, S, be.p(f64(T, H, W)), bad, s) == _capi.RM_E_BADARG, bad
    bgr = be.dev(np.random.default_rng(2).integers(0, 256, size=(T, H, W, 3), dtype=np.uint8))
    st = Stream(be, H, W, L, S)
    try:
        out16 = be.dev(np.zeros((T, H, W, 3), np.uint16))
        assert lib.rm_stream_push(ctx, st.h, be.p(d), U16, T, be.p(out16), _capi.RM_BGR8, s) == _capi.RM_E_BADARG     # colour out needs BGR frames in
        assert lib.rm_stream_push(ctx, st.h, be.p(bgr), U16 + 1, T, be.p(out16), _capi.RM_BGR8, s) == _capi.RM_E_BADARG
        assert lib.rm_stream_push(ctx, st.h, be.p(d), U16, T, be.p(out16), 7, s) == _capi.RM_E_BADARG
        # the gray video of a BGR stream may be 16 bits wide; the colour video is [n,H,W,3] uint8 whatever else is asked for
        assert lib.rm_stream_push(ctx, st.h, be.p(bgr), _capi.RM_BGR8, T, be.p(out16), U16, s) == _capi.RM_OK
    finally:
        st.close()
    # rm_magnify_bgr has no dtype argument at all: uint8 in, uint8 out; rm_bgr_to_gray is what it was
    gray = be.dev(np.zeros((T, H, W), np.uint8))
    ck(be, lib.rm_bgr_to_gray(ctx, be.p(bgr), T * NPIX, be.p(gray), s), "rm_bgr_to_gray")
    b = be.np(bgr).astype(np.int64)
    assert np.array_equal(be.np(gray), ((b[..., 0] * 1868 + b[..., 1] * 9617 + b[..., 2] * 4899 + 8192) >> 14).astype(np.uint8))
    assert "rm_magnify_bgr" in _capi.SIGNATURES and len(_capi.SIGNATURES["rm_magnify_bgr"][1]) == 13
