"""Shared by tests/test_emu_stream.py and tests/test_gpu_stream.py (not a test module): the case tables, thin callers of rm_sosfilt and
rm_stream_* on raw pointers, the numpy restatement of scipy's sosfilt recurrence, and the checks both builds run.  A backend `be` hides
where the memory lives:
    be.lib, be.ctx, be.stream()          the bound library, a context, the stream argument
    be.other_stream()                    a stream argument that is not be.stream()
    be.dev(ndarray) -> buffer            an array where the library reads it (numpy itself on the host-emulated build, a tensor on the GPU)
    be.p(buffer) -> c_void_p             its address;  buffer[a:b] slices frames
    be.empty(shape, dtype) -> buffer, be.np(buffer) -> ndarray      a result area and its host copy
    be.new_ctx(device=0) -> ctx or None, be.free_ctx(ctx)

Definition under test (include/respmon_hip.h): out[t] = convert(f[t] + raw[t]), raw = collapse(sosfilt * amp of the Laplacian levels
skip .. levels-2 along time), in that operation order, however the stream is cut into pushes.  The comparisons are exact."""
import ctypes
import os

import numpy as np

from respmon_amd import _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {np.dtype(np.uint8): _capi.RM_U8, np.dtype(np.uint16): _capi.RM_U16, np.dtype(np.float16): _capi.RM_F16, np.dtype(np.float32): _capi.RM_F32,
      np.dtype(np.float64): _capi.RM_F64}
OUT_NP = {_capi.RM_U8: np.uint8, _capi.RM_U16: np.uint16, _capi.RM_F32: np.float32, _capi.RM_F64: np.float64}

# ---- the filter ---------------------------------------------------------------------------------------------------------------
SOS_ORDERS = (1, 2, 6, 8)
SOS_RATES = ((10.0, 0.1, 1.0), (30.0, 0.1, 0.5), (60.0, 0.1, 0.5))     # (fps, band)
SOS_T = (1, 2, 13, 40)
SOS_NP = (1, 63, 64, 65, 257)
SOS_SCALES = (1.0, 500.0)


def butter_sos(order, fps, fmin, fmax):
    import scipy.signal
    return np.ascontiguousarray(scipy.signal.butter(order, [fmin / (fps / 2), fmax / (fps / 2)], btype='band', output='sos'))


def sosfilt_zi(sos):
    import scipy.signal
    return np.ascontiguousarray(scipy.signal.sosfilt_zi(sos))


def sos_restated(sos, x, z=None, scale=1.0):
    """scipy.signal.sosfilt(sos, x, axis=0, zi=z) * scale written out: x [n, ...], z [nsec, 2, ...] (None: rest).  Every line is one
    rounded float64 operation per element, in the order of scipy's loop.  -> (y, the state after the last sample)"""
    x = np.asarray(x, dtype=np.float64)
    nsec = sos.shape[0]
    z = np.zeros((nsec, 2) + x.shape[1:]) if z is None else np.array(z, dtype=np.float64)
    y = np.empty_like(x)
    for t in range(x.shape[0]):
        cur = x[t]
        for s in range(nsec):
            b0, b1, b2, _, a1, a2 = sos[s]
            new = b0 * cur + z[s, 0]
            z[s, 0] = (b1 * cur - a1 * new) + z[s, 1]
            z[s, 1] = b2 * cur - a2 * new
            cur = new
        y[t] = cur * scale
    return y, z


def steady_state(zi, x0):
    """z[s][k] = zi[s][k] * x[0]: one multiplication per element"""
    return zi.reshape(zi.shape + (1,) * np.ndim(x0)) * np.asarray(x0, dtype=np.float64)[None, None]


def sosfilt_rc(be, sos, x, zi=None, scale=1.0, out=None, nsec=None):
    """the raw rm_sosfilt call -> (return code, out buffer)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    d = be.dev(x)
    o = be.empty(x.shape, np.float64) if out is None else out
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    z = None if zi is None else np.ascontiguousarray(zi, dtype=np.float64)
    rc = be.lib.rm_sosfilt(be.ctx, be.p(d) if out is None else be.p(out), x.shape[0], x[0].size, ctypes.c_void_p(sos.ctypes.data),
                           sos.shape[0] if nsec is None else nsec, None if z is None else ctypes.c_void_p(z.ctypes.data), float(scale), be.p(o), be.stream())
    return rc, o


def sosfilt(be, sos, x, zi=None, scale=1.0):
    rc, o = sosfilt_rc(be, sos, x, zi, scale)
    _capi.check(be.lib, rc, "rm_sosfilt")
    return be.np(o)


def check_sosfilt(be, order, rate):
    import scipy.signal
    fps, fmin, fmax = rate
    sos = butter_sos(order, fps, fmin, fmax)
    assert sos.shape == (order, 6) and np.all(sos[:, 3] == 1.0)
    zi = sosfilt_zi(sos)
    rng = np.random.default_rng(100 * order + int(fps))
    for T in SOS_T:
        for NP in SOS_NP:
            x = rng.random((T, NP))
            for scale in SOS_SCALES:
                got = sosfilt(be, sos, x, scale=scale)
                want, _ = sos_restated(sos, x, scale=scale)
                assert np.array_equal(got, want), (order, rate, T, NP, scale, np.abs(got - want).max())
                assert np.abs(got - scipy.signal.sosfilt(sos, x, axis=0) * scale).max() <= 1e-12
                z0 = steady_state(zi, x[0])
                got = sosfilt(be, sos, x, zi=zi, scale=scale)
                want, _ = sos_restated(sos, x, z=z0, scale=scale)
                assert np.array_equal(got, want), (order, rate, T, NP, scale, "zi", np.abs(got - want).max())
                assert np.abs(got - scipy.signal.sosfilt(sos, x, axis=0, zi=z0)[0] * scale).max() <= 1e-12


# the section counts no integer-order design of SOS_ORDERS gives: a low-pass design followed by a band-pass one, so that every section
# has coefficients of its own and the low-pass sections (DC gain != 0) have a steady state that is not zero
SOS_MIXED = {3: (2, 2), 4: (4, 2), 5: (4, 3), 7: (6, 4)}        # sections -> (low-pass order: order / 2 sections, band-pass order)


def mixed_sos(nsec, fps, fmin, fmax):
    import scipy.signal
    lo, bp = SOS_MIXED[nsec]
    sos = np.concatenate([scipy.signal.butter(lo, 2.5 * fmax / (fps / 2), btype='low', output='sos'), butter_sos(bp, fps, fmin, fmax)])
    assert sos.shape == (nsec, 6) and np.all(sos[:, 3] == 1.0) and len({tuple(r) for r in sos}) == nsec
    return np.ascontiguousarray(sos)


def check_sosfilt_sections(be, nsec, rate, Ts=SOS_T, NPs=SOS_NP):
    """check_sosfilt for a table of `nsec` sections that is not one design: from rest and from zi, bit for bit"""
    import scipy.signal
    sos = mixed_sos(nsec, *rate)
    zi = sosfilt_zi(sos)
    assert np.abs(zi[:SOS_MIXED[nsec][0] // 2 + 1]).min() > 0        # the steady state reaches past the low-pass sections
    rng = np.random.default_rng(100 * nsec + int(rate[0]))
    for T in Ts:
        for NP in NPs:
            x = rng.random((T, NP))
            for scale in SOS_SCALES:
                got = sosfilt(be, sos, x, scale=scale)
                want, _ = sos_restated(sos, x, scale=scale)
                assert np.array_equal(got, want), (nsec, rate, T, NP, scale, np.abs(got - want).max())
                assert np.abs(got - scipy.signal.sosfilt(sos, x, axis=0) * scale).max() <= 1e-12
                z0 = steady_state(zi, x[0])
                got = sosfilt(be, sos, x, zi=zi, scale=scale)
                want, _ = sos_restated(sos, x, z=z0, scale=scale)
                assert np.array_equal(got, want), (nsec, rate, T, NP, scale, "zi", np.abs(got - want).max())
                assert np.abs(got - scipy.signal.sosfilt(sos, x, axis=0, zi=z0)[0] * scale).max() <= 1e-12


def check_sosfilt_refusals(be):
    sos = butter_sos(2, 10.0, 0.1, 1.0)
    x = np.random.default_rng(3).random((4, 5))
    E, U = _capi.RM_E_BADARG, _capi.RM_E_UNSUPPORTED
    nine = np.ascontiguousarray(np.tile(sos[:1], (9, 1)))
    assert sosfilt_rc(be, nine, x)[0] == U
    assert sosfilt_rc(be, nine[:8], x)[0] == _capi.RM_OK
    assert sosfilt_rc(be, sos, x, nsec=0)[0] == E and sosfilt_rc(be, sos, x, nsec=-1)[0] == E
    bad = sos.copy()
    bad[1, 3] = 2.0
    assert sosfilt_rc(be, bad, x)[0] == E
    assert b"a0" in be.lib.rm_last_error_string()
    d = be.dev(x)
    assert sosfilt_rc(be, sos, x, out=d)[0] == E                 # data == out
    assert b"in-place" in be.lib.rm_last_error_string()
    assert np.array_equal(sosfilt(be, sos, x), sos_restated(sos, x)[0])      # the context still works


def check_why_sos(be, lfilter):
    """fps 30, 0.1-0.5 Hz, 2 000 samples x 64 elements of uniform noise: the sections stay small (scipy on the CPU: 0.22), the `ba` form of
    the same design, through rm_lfilter, explodes (scipy on the CPU: 1.7e19) -- the reason the stream filters in sections.
    lfilter(b, a, x) -> ndarray: rm_lfilter of this backend."""
    import scipy.signal
    x = np.random.default_rng(2024).random((2000, 64))
    wn = [0.1 / 15.0, 0.5 / 15.0]
    sos = np.ascontiguousarray(scipy.signal.butter(6, wn, btype='band', output='sos'))
    y = sosfilt(be, sos, x)
    print("why sos: max|sosfilt| = %.3g" % np.abs(y).max())
    assert np.isfinite(y).all() and np.abs(y).max() < 10
    b, a = scipy.signal.butter(6, wn, btype='band', output='ba')
    with np.errstate(all="ignore"):
        yb = lfilter(b, a, x)
        big = np.nanmax(np.abs(yb))
    print("why sos: max|lfilter ba| = %.3g" % big)
    assert big > 1e6


# ---- the stream ---------------------------------------------------------------------------------------------------------------
FPS, BAND, AMP, ORDER = 30.0, (0.1, 1.0), 50.0, 6
NFRAMES = 20
CHUNKS = (1, 2, 7, 9, 1)           # 9 = MAG_FC + 1: two frame groups of the fused sum kernel in one push
# (H, W, levels, skip, input dtype, BGR output as well)
STREAM_CASES = [
    (40, 70, 3, 1, np.uint8),        # element-wise accesses
    (48, 128, 4, 2, np.float64),     # whole tiles, 16-byte accesses
    (40, 72, 5, 3, np.float32),
    (70, 152, 6, 4, np.float16),
    (9, 20, 3, 1, np.uint8),         # smaller than a tile
    (16, 64, 3, 1, np.uint8),        # exactly one tile
    (40, 70, 4, 2, "bgr"),           # gray and BGR output
    (20, 30, 3, 0, np.float64),      # skip 0: the plain sum behind a materialised raw
    (70, 70, 7, 5, np.uint8),        # skip 5: plain
    (2, 2, 3, 1, np.float64),        # TileEval does not apply
    (20, 30, 3, 2, np.uint8),        # nothing filtered
]
REFERENCE_CASES = [STREAM_CASES[1], STREAM_CASES[3], STREAM_CASES[0]]


def case_id(c):
    return "%dx%d_L%dS%d_%s" % (c[0], c[1], c[2], c[3], getattr(c[4], "__name__", c[4]))


_VIDEOS = {}


def video(H, W, dt, T=NFRAMES):
    """the frames of a case (made once, read-only)"""
    key = (T, H, W, getattr(dt, "__name__", dt))
    if key not in _VIDEOS:
        u8 = synth.synth_breathing(T, H, W, seed=H + W, fps=FPS)
        if isinstance(dt, str):
            rng = np.random.default_rng(H)
            v = np.clip(u8[..., None].astype(np.int32) + rng.integers(-20, 21, (T, H, W, 3)), 0, 255).astype(np.uint8)
        elif dt == np.uint8:
            v = u8
        else:
            v = (u8 * (1.0 / 255)).astype(dt)
        v = np.ascontiguousarray(v)
        v.setflags(write=False)
        _VIDEOS[key] = v
    return _VIDEOS[key]


def code_of(a):
    return _capi.RM_BGR8 if a.ndim == 4 else DT[np.dtype(a.dtype)]


def design(zi=False):
    sos = butter_sos(ORDER, FPS, *BAND)
    return sos, (sosfilt_zi(sos) if zi else None)


def as_read(be, frames):
    """f: the frames as the calibration reads them, float64 (BGR: cvtColor on the device first)"""
    if frames.ndim == 4:
        src = be.dev(frames)
        gray = be.empty(frames.shape[:3], np.uint8)
        _capi.check(be.lib, be.lib.rm_bgr_to_gray(be.ctx, be.p(src), gray_size(frames), be.p(gray), be.stream()), "rm_bgr_to_gray")
        frames = be.np(gray)
    if frames.dtype == np.uint8:
        return frames * (1.0 / 255)
    return frames.astype(np.float64)


def gray_size(frames):
    return int(np.prod(frames.shape[:3]))


def level_shapes(T, H, W, L):
    shapes = [(T, H, W)]
    for _ in range(1, L):
        shapes.append((T, (shapes[-1][1] + 1) // 2, (shapes[-1][2] + 1) // 2))
    return shapes


def composition(be, f, L, S, sos, zi, amp):
    """raw of the definition: rm_create_laplacian_video_pyramid, the numpy restatement * amp on levels S .. L-2 (zi: started from
    zi * the first frame's level), rm_collapse_laplacian_video_pyramid"""
    T, H, W = f.shape
    src = be.dev(np.ascontiguousarray(f))
    levels = [be.empty(s, np.float64) for s in level_shapes(T, H, W, L)]
    ptrs = (ctypes.c_void_p * L)(*[be.p(lv).value for lv in levels])
    _capi.check(be.lib, be.lib.rm_create_laplacian_video_pyramid(be.ctx, be.p(src), _capi.RM_F64, T, H, W, L, ptrs, be.stream()), "create pyramid")
    bp = []
    for i, lv in enumerate(levels):
        x = be.np(lv)
        if i < S or i >= L - 1:
            bp.append(be.dev(np.zeros(x.shape)))
            continue
        z0 = None if zi is None else steady_state(zi, x[0])
        bp.append(be.dev(np.ascontiguousarray(sos_restated(sos, x, z=z0, scale=amp)[0])))
    ptrs = (ctypes.c_void_p * L)(*[be.p(lv).value for lv in bp])
    out = be.empty((T, H, W), np.float64)
    _capi.check(be.lib, be.lib.rm_collapse_laplacian_video_pyramid(be.ctx, ptrs, T, H, W, L, be.p(out), be.stream()), "collapse pyramid")
    return be.np(out)


def to_u8(m):
    """the clamp to [0, 1], then transforms.py:26-29 (the C truncation of m * 255)"""
    return (np.clip(m, 0.0, 1.0) * 255).astype(np.uint8)


class Stream:
    def __init__(self, be, H, W, L, S, sos, zi=None, amp=AMP, ctx=None):
        self.be, self.H, self.W, self.ctx = be, H, W, (ctx if ctx is not None else be.ctx)
        self.h = ctypes.c_void_p()
        sos = np.ascontiguousarray(sos, dtype=np.float64)
        z = None if zi is None else np.ascontiguousarray(zi, dtype=np.float64)
        _capi.check(be.lib, be.lib.rm_stream_create(self.ctx, H, W, L, S, ctypes.c_void_p(sos.ctypes.data), sos.shape[0],
                                                    None if z is None else ctypes.c_void_p(z.ctypes.data), float(amp), ctypes.byref(self.h)), "rm_stream_create")

    def close(self):
        if self.h:
            self.be.lib.rm_stream_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def push_rc(self, buf, code, n, out, out_code, ctx=None, stream=None):
        return self.be.lib.rm_stream_push(ctx if ctx is not None else self.ctx, self.h, self.be.p(buf), code, n, self.be.p(out), out_code,
                                          self.be.stream() if stream is None else stream)

    def push(self, frames, out_code):
        """frames: ndarray -> the magnified frames as ndarray"""
        frames = np.ascontiguousarray(frames)
        shape = frames.shape if out_code == _capi.RM_BGR8 else frames.shape[:3]
        out = self.be.empty(shape, np.uint8 if out_code == _capi.RM_BGR8 else OUT_NP[out_code])
        _capi.check(self.be.lib, self.push_rc(self.be.dev(frames), code_of(frames), len(frames), out, out_code), "rm_stream_push")
        return self.be.np(out)

    def run(self, frames, out_code, chunks=None):
        """the whole of `frames` in pushes of `chunks` frames (cycled; None: one push)"""
        if chunks is None:
            return self.push(frames, out_code)
        outs, k, i = [], 0, 0
        while k < len(frames):
            n = chunks[i % len(chunks)]
            outs.append(self.push(frames[k:k + n], out_code))
            k += n
            i += 1
        return np.concatenate(outs)

    def reset(self):
        _capi.check(self.be.lib, self.be.lib.rm_stream_reset(self.ctx, self.h), "rm_stream_reset")

    def info(self):
        seen, n, b = ctypes.c_longlong(-1), ctypes.c_size_t(), ctypes.c_size_t()
        _capi.check(self.be.lib, self.be.lib.rm_stream_info(self.h, ctypes.byref(seen), ctypes.byref(n), ctypes.byref(b)), "rm_stream_info")
        return int(seen.value), int(n.value), int(b.value)


def filtered_np(H, W, L, S):
    if S >= L - 1:
        return 0
    return sum(h * w for _, h, w in level_shapes(1, H, W, L)[S:L - 1])


def check_stream_case(be, case, with_zi):
    H, W, L, S, dt = case
    v = video(H, W, dt)
    T = len(v)
    sos, zi = design(with_zi)
    f = as_read(be, v)
    raw = composition(be, f, L, S, sos, zi, AMP)
    want = f + raw
    if S >= L - 1:
        assert not raw.any()
    elif min(H, W) > 2:                          # (2 x 2: the only filtered level is one pixel, G_1 - pyrUp(G_2) with G_2 == G_1)
        assert np.abs(raw).max() > 1e-3          # the motion is there: the comparison is not between zeros
    with Stream(be, H, W, L, S, sos, zi) as st:
        assert st.info() == (0, filtered_np(H, W, L, S), 16 * ORDER * filtered_np(H, W, L, S))
        whole = st.run(v, _capi.RM_F64)
        assert st.info()[0] == T
        assert np.array_equal(whole, want), np.abs(whole - want).max()
        st.reset()
        assert st.info()[0] == 0
        assert np.array_equal(st.run(v, _capi.RM_F64, (1,)), want)
        st.reset()
        assert np.array_equal(st.run(v, _capi.RM_F64, CHUNKS), want)
        assert st.info()[0] == T
        # the other output dtypes are the conversions of the same sum, in a chunking of their own
        st.reset()
        assert np.array_equal(st.run(v, _capi.RM_F32, CHUNKS), want.astype(np.float32))
        st.reset()
        assert np.array_equal(st.run(v, _capi.RM_U8, (7, 1)), to_u8(want))
        if v.ndim == 4:
            col = to_u8(v * (1.0 / 255) + raw[..., None])
            for chunks in (None, (1,), CHUNKS):
                st.reset()
                assert np.array_equal(st.run(v, _capi.RM_BGR8, chunks), col), chunks
        # the internal split of a large push (two frames per chunk here) changes nothing
        _capi.check(be.lib, be.lib.rm_debug_set(be.ctx, b"stream_frames", 2), "rm_debug_set")
        try:
            st.reset()
            assert np.array_equal(st.run(v, _capi.RM_F64), want)
        finally:
            _capi.check(be.lib, be.lib.rm_debug_set(be.ctx, b"stream_frames", 0), "rm_debug_set")


def check_stream_sections(be, nsec, with_zi, case=STREAM_CASES[0]):
    """rm_stream_push with a table of `nsec` sections (mixed_sos), cut three ways, bit for bit against the composition whose filter is
    sos_restated: the state planes of that section count are stored and reloaded at every cut"""
    H, W, L, S, dt = case
    v = video(H, W, dt)
    sos = mixed_sos(nsec, FPS, *BAND)
    zi = sosfilt_zi(sos) if with_zi else None
    f = as_read(be, v)
    raw = composition(be, f, L, S, sos, zi, AMP)
    want = f + raw
    assert np.abs(raw).max() > 1e-3
    with Stream(be, H, W, L, S, sos, zi) as st:
        assert st.info() == (0, filtered_np(H, W, L, S), 16 * nsec * filtered_np(H, W, L, S))
        for chunks in (None, (1,), CHUNKS):
            got = st.run(v, _capi.RM_F64, chunks)
            assert st.info()[0] == len(v)
            assert np.array_equal(got, want), (nsec, with_zi, chunks, np.abs(got - want).max())
            st.reset()


def check_steady_start_is_quiet(be):
    """the point of zi: a still scene gives (nearly) the scene back from the first frame on, where the start from rest rings"""
    H, W, L, S = 40, 70, 4, 2
    v = np.ascontiguousarray(np.broadcast_to(video(H, W, np.uint8)[:1], (NFRAMES, H, W)))
    f = v * (1.0 / 255)
    sos, zi = design(True)
    with Stream(be, H, W, L, S, sos, zi) as st:
        quiet = np.abs(st.run(v, _capi.RM_F64, CHUNKS) - f).max()
    with Stream(be, H, W, L, S, sos, None) as st:
        ringing = np.abs(st.run(v, _capi.RM_F64, CHUNKS) - f).max()
    print("steady start: max|out - f| = %.3g, from rest %.3g" % (quiet, ringing))
    assert quiet < 1e-6 and ringing > 1e3 * quiet


def check_state_hygiene(be, locate, magnify):
    """two streams of different geometry pushed alternately on one context, with an rm_locate and an rm_magnify on that context between
    the pushes (locate(frames_u8), magnify(frames_u8): this backend's calls, results ignored)"""
    ga, gb = (40, 70, 4, 2, np.uint8), (48, 128, 5, 3, np.float32)
    va, vb = video(*ga[:2], ga[4]), video(*gb[:2], gb[4])
    sos, zi = design(True)
    other = video(33, 64, np.uint8)
    with Stream(be, *ga[:4], sos, zi) as a, Stream(be, *gb[:4], sos, None) as b:
        alone_a = a.run(va, _capi.RM_F64)
        alone_b = b.run(vb, _capi.RM_F64)
        a.reset(); b.reset()
        outs_a, outs_b = [], []
        for k in range(0, NFRAMES, 5):
            outs_a.append(a.push(va[k:k + 5], _capi.RM_F64))
            locate(other)
            outs_b.append(b.push(vb[k:k + 5], _capi.RM_F64))
            magnify(other)
            assert a.info()[0] == k + 5 and b.info()[0] == k + 5
        assert np.array_equal(np.concatenate(outs_a), alone_a)
        assert np.array_equal(np.concatenate(outs_b), alone_b)
        a.reset()
        assert a.info()[0] == 0
        assert np.array_equal(a.run(va, _capi.RM_F64, (3,)), alone_a)      # the same frames after a reset: the first run again
        assert a.info()[0] == NFRAMES


def check_stream_refusals(be, submit, result):
    """submit(frames_u8) -> ticket, result(ticket): rm_locate_submit / rm_locate_result on be.ctx and be.stream()"""
    lib = be.lib
    E, U = _capi.RM_E_BADARG, _capi.RM_E_UNSUPPORTED
    H, W, L, S = 40, 70, 4, 2
    sos, zi = design(True)
    sp, zp = ctypes.c_void_p(sos.ctypes.data), ctypes.c_void_p(zi.ctypes.data)
    h = ctypes.c_void_p(1)
    assert lib.rm_stream_create(be.ctx, 0, W, L, S, sp, ORDER, zp, AMP, ctypes.byref(h)) == E and not h.value
    assert lib.rm_stream_create(be.ctx, H, W, 0, S, sp, ORDER, zp, AMP, ctypes.byref(h)) == E
    assert lib.rm_stream_create(be.ctx, H, W, L, -1, sp, ORDER, zp, AMP, ctypes.byref(h)) == E
    assert lib.rm_stream_create(be.ctx, H, W, L, S, None, ORDER, zp, AMP, ctypes.byref(h)) == E
    assert lib.rm_stream_create(be.ctx, H, W, L, S, sp, 0, zp, AMP, ctypes.byref(h)) == E
    assert lib.rm_stream_create(be.ctx, H, W, L, S, sp, 9, zp, AMP, ctypes.byref(h)) == U
    assert lib.rm_stream_create(None, H, W, L, S, sp, ORDER, zp, AMP, ctypes.byref(h)) == E
    assert lib.rm_stream_create(be.ctx, H, W, L, S, sp, ORDER, zp, AMP, None) == E
    bad = sos.copy()
    bad[0, 3] = 0.5
    assert lib.rm_stream_create(be.ctx, H, W, L, S, ctypes.c_void_p(bad.ctypes.data), ORDER, zp, AMP, ctypes.byref(h)) == E
    assert lib.rm_stream_destroy(None) == _capi.RM_OK
    assert lib.rm_stream_info(None, None, None, None) == E
    v = video(H, W, np.uint8)
    vc = video(H, W, "bgr")
    with Stream(be, H, W, L, S, sos, zi) as st:
        assert lib.rm_stream_info(st.h, None, None, None) == _capi.RM_OK
        assert lib.rm_stream_reset(be.ctx, None) == E and lib.rm_stream_reset(None, st.h) == E
        want = st.run(v, _capi.RM_U8)
        st.reset()
        buf, out = be.dev(v), be.empty(v.shape, np.uint8)
        for n in (0, -1):
            assert st.push_rc(buf, _capi.RM_U8, n, out, _capi.RM_U8) == E
        assert lib.rm_stream_push(be.ctx, st.h, None, _capi.RM_U8, 1, be.p(out), _capi.RM_U8, be.stream()) == E
        assert lib.rm_stream_push(be.ctx, st.h, be.p(buf), _capi.RM_U8, 1, None, _capi.RM_U8, be.stream()) == E
        assert lib.rm_stream_push(be.ctx, None, be.p(buf), _capi.RM_U8, 1, be.p(out), _capi.RM_U8, be.stream()) == E
        assert lib.rm_stream_push(None, st.h, be.p(buf), _capi.RM_U8, 1, be.p(out), _capi.RM_U8, be.stream()) == E
        for code in (-1, 5, 99):
            assert st.push_rc(buf, code, 1, out, _capi.RM_U8) == E
        for oc in (_capi.RM_F16, 7, -1):
            assert st.push_rc(buf, _capi.RM_U8, 1, out, oc) == E
        assert b"out_dtype" in lib.rm_last_error_string()
        assert st.push_rc(buf, _capi.RM_U8, 1, be.empty(vc.shape, np.uint8), _capi.RM_BGR8) == E       # BGR out from gray in
        assert b"RM_BGR8" in lib.rm_last_error_string()
        assert st.push_rc(buf, _capi.RM_U8, 2, buf, _capi.RM_U8) == E                                  # in place
        assert b"overlap" in lib.rm_last_error_string()
        both = be.empty((2 * NFRAMES, H, W), np.uint8)
        last = ctypes.c_void_p(be.p(both).value + 2 * H * W - 1)
        assert lib.rm_stream_push(be.ctx, st.h, be.p(both), _capi.RM_U8, 2, last, _capi.RM_U8, be.stream()) == E   # the last byte of the frames
        other_dev = be.new_ctx(1)
        if other_dev is not None:
            assert st.push_rc(buf, _capi.RM_U8, 1, out, _capi.RM_U8, ctx=other_dev) == E               # wrong device
            assert b"device" in lib.rm_last_error_string()
            be.free_ctx(other_dev)
        # a submission in flight on the context's stream: a push on another stream is refused, not run on shared workspace
        tk = submit(video(33, 64, np.uint8))
        assert st.push_rc(buf, _capi.RM_U8, 1, out, _capi.RM_U8, stream=be.other_stream()) == _capi.RM_E_BUSY
        assert b"in flight" in lib.rm_last_error_string()
        result(tk)
        assert st.info()[0] == 0                                     # every refused push left the stream as it was
        _capi.check(lib, st.push_rc(buf, _capi.RM_U8, NFRAMES, out, _capi.RM_U8), "rm_stream_push")
        assert np.array_equal(be.np(out), want)


def check_means_what_the_reference_means(be, oracle, case):
    """Against the reference's own sequence with scipy's sosfilt * amp as its temporal_filter_function, formed the reference's way
    (transforms.py:170, 181): the band-passed levels added into the video pyramid, then the collapse.  Bound and procedure of
    tests/test_emu_magnify.py test_emu_magnify_means_what_the_reference_means: d0 = max|ref - (f + raw_oracle)| / max|ref| is the cost of
    the reordering, measured with the oracle alone; err <= 4 d0 + 1e-12 max|raw| / max|ref|."""
    import scipy.signal
    H, W, L, S, dt = case
    v = video(H, W, dt)
    f = as_read(be, v)
    sos, _ = design(False)

    def filt(x, fps, freq_min, freq_max, amplification_factor, axis=0):
        assert (fps, freq_min, freq_max) == (FPS,) + BAND
        return scipy.signal.sosfilt(sos, np.asarray(x, dtype=np.float64), axis=axis) * amplification_factor

    pyr = oracle.create_laplacian_video_pyramid(f, L)
    for i in range(len(pyr)):
        if i < S or i >= len(pyr) - 1:
            continue
        pyr[i] = pyr[i] + filt(pyr[i], FPS, BAND[0], BAND[1], AMP)
    ref = oracle.collapse_laplacian_video_pyramid(pyr)
    raw_o = oracle.eulerian_magnification_bandpass(f.copy(), FPS, BAND[0], BAND[1], AMP, pyramid_levels=L, skip_levels_at_top=S,
                                                   temporal_filter_function=filt)[1]
    scale = np.abs(ref).max()
    d0 = np.abs(ref - (f + raw_o)).max() / scale
    e_raw = 1e-12 * np.abs(raw_o).max() / scale
    with Stream(be, H, W, L, S, sos, None) as st:
        m = st.run(v, _capi.RM_F64, CHUNKS)
    err = np.abs(m - ref).max() / scale
    print("stream vs reference: %s d0=%.3g e_raw=%.3g err=%.3g" % (case_id(case), d0, e_raw, err))
    assert 0 < d0 < 1e-14
    assert err <= 4 * d0 + e_raw, (case, err, d0, e_raw)


def check_bookkeeping(lib):
    import hashlib
    import json
    names = ("rm_sosfilt", "rm_stream_create", "rm_stream_destroy", "rm_stream_reset", "rm_stream_info", "rm_stream_push")
    hdr = open(os.path.join(ROOT, "include", "respmon_hip.h")).read()
    for n in names:
        assert n in _capi.SIGNATURES and ("int %s(" % n) in hdr, n
        getattr(lib, n)
    assert "out[t] = convert(f[t] + raw[t])" in hdr and "temporal_bandpass_filter_sos" in hdr
    assert lib.rm_abi_version() == 1
    csrc = os.path.join(ROOT, "respmon_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "rm_stream" in [ln for ln in mk.splitlines() if ln.startswith("UNITS")][0].split()
    assert '#include "rm_stream.hip"' in open(os.path.join(csrc, "rm_unity.hip")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("STAMP_SRCS")][0].split("=", 1)[1].split()
    assert not any("stream" in s or "magnify" in s for s in srcs)
    sha = hashlib.sha256(b"".join(open(os.path.join(csrc, s), "rb").read() for s in srcs)).hexdigest()[:16]
    committed = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
    stamps = {e["kernel_source_sha"] for e in (committed.values() if isinstance(committed, dict) else committed)
              if isinstance(e, dict) and "kernel_source_sha" in e}
    assert stamps == {sha}, (stamps, sha)
