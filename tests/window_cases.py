"""Shared by tests/test_emu_window.py and tests/test_gpu_window.py (not a test module): the moving-blob stream, thin callers of the
rm_window_* C-ABI on raw pointers, and the checks both builds run.  A backend `be` hides where the memory lives:
    be.lib, be.ctx, be.stream()          the bound library, a context, the stream argument
    be.dev(ndarray) -> buffer            frames where the library reads them (numpy itself on the host-emulated build, a tensor on the GPU)
    be.p(buffer) -> c_void_p             its address;  buffer[a:b] slices frames
    be.out(shape) -> buffer, be.np(buffer) -> ndarray      a float64 result area and its host copy

Every comparison is exact: the claim under test is "the same arithmetic on the same values" as the contiguous-buffer calls."""
import ctypes

import numpy as np

from respmon_amd import _capi, synth

# fps / band chosen so that T = 9, 10 and 16 all keep a few non-DC bins (0.25-0.9 Hz at 2.5 fps; the blob breathes at 0.5 Hz)
KW = dict(fps=2.5, fmin=0.25, fmax=0.9, amp=500.0, thr=0.7, threshold=20)
GEOMS = [(70, 90, 4, 1), (70, 90, 4, 2), (33, 47, 3, 1)]      # (H, W, levels, skip); the last: odd sizes at every level
SMALL = (33, 47, 3, 1)
TS = (16, 10, 9)                                               # MFMA with a K-split / even, no multiple of 4 / odd: the VALU form
CENTRES = ((0.30, 0.28), (0.52, 0.66), (0.72, 0.36))


def knob_cases(T):
    """the default choice, and for even T the two other forms through the debug switches"""
    return [{}] + ([{"temporal_wide": 1}, {"temporal_valu": 1}] if T % 2 == 0 else [])


_STREAMS = {}


def stream(T, H, W):
    """uint8 [3T,H,W]: synth_breathing in three segments of T frames whose blob sits somewhere else each time (made once, never modified)"""
    key = (T, H, W)
    if key not in _STREAMS:
        segs = [synth.synth_breathing(T, H, W, seed=40 + i, fps=KW["fps"], breath_hz=0.5, amplitude=0.3, center=c, sigma=(0.13, 0.11))
                for i, c in enumerate(CENTRES)]
        v = np.concatenate(segs)
        v.setflags(write=False)
        _STREAMS[key] = v
    return _STREAMS[key]


DT = {np.dtype(np.uint8): _capi.RM_U8, np.dtype(np.float16): _capi.RM_F16, np.dtype(np.float32): _capi.RM_F32, np.dtype(np.float64): _capi.RM_F64}


def code_of(a):
    return _capi.RM_BGR8 if a.ndim == 4 else DT[np.dtype(a.dtype)]


class Knobs:
    def __init__(self, be, knobs):
        self.be, self.knobs = be, knobs

    def _set(self, k, v):
        _capi.check(self.be.lib, self.be.lib.rm_debug_set(self.be.ctx, k.encode(), v), "rm_debug_set")

    def __enter__(self):
        for k, v in self.knobs.items():
            self._set(k, v)

    def __exit__(self, *exc):
        for k in self.knobs:
            self._set(k, -1 if k == "temporal_wide" else 0)


class Window:
    def __init__(self, be, T, H, W, levels, skip, flags=0):
        self.be, self.T, self.H, self.W = be, T, H, W
        self.h = ctypes.c_void_p()
        _capi.check(be.lib, be.lib.rm_window_create(be.ctx, T, H, W, levels, skip, flags, ctypes.byref(self.h)), "rm_window_create")

    def close(self):
        if self.h:
            self.be.lib.rm_window_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def push(self, buf, code, n):
        _capi.check(self.be.lib, self.be.lib.rm_window_push(self.be.ctx, self.h, self.be.p(buf), code, n, self.be.stream()), "rm_window_push")

    def push_np(self, frames):
        frames = np.ascontiguousarray(frames)
        self.push(self.be.dev(frames), code_of(frames), len(frames))

    def reset(self):
        _capi.check(self.be.lib, self.be.lib.rm_window_reset(self.be.ctx, self.h), "rm_window_reset")

    def info(self):
        c, h, n, b = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(), ctypes.c_size_t()
        _capi.check(self.be.lib, self.be.lib.rm_window_info(self.h, ctypes.byref(c), ctypes.byref(h), ctypes.byref(n), ctypes.byref(b)), "rm_window_info")
        return c.value, h.value, int(n.value), int(b.value)

    def rows(self):
        _, _, NP, _ = self.info()
        out = np.full((self.T, NP), np.nan)
        _capi.check(self.be.lib, self.be.lib.rm_debug_window_rows(self.be.ctx, self.h, 0, self.T, ctypes.c_void_p(out.ctypes.data), self.be.stream()),
                    "rm_debug_window_rows")
        return out

    def calibrate_rc(self, kw=KW):
        heat = self.be.out((self.H, self.W))
        rc = self.be.lib.rm_window_calibrate(self.be.ctx, self.h, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], kw["thr"], self.be.p(heat),
                                             self.be.stream())
        return rc, heat

    def calibrate(self, kw=KW):
        rc, heat = self.calibrate_rc(kw)
        _capi.check(self.be.lib, rc, "rm_window_calibrate")
        return self.be.np(heat)

    def locate(self, kw=KW):
        """-> (rc, roi or None)"""
        xywh = np.full(4, -7, np.int32)
        rc = self.be.lib.rm_window_locate(self.be.ctx, self.h, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], kw["thr"], kw["threshold"],
                                          ctypes.c_void_p(xywh.ctypes.data), self.be.stream())
        return rc, (tuple(int(v) for v in xywh) if rc == _capi.RM_OK else None)

    def locate_multi(self, K, min_area=0.0, kw=KW):
        xywh = np.full((max(K, 1), 4), -7, np.int32)
        area = np.full(max(K, 1), -7.0)
        n = ctypes.c_int(-7)
        rc = self.be.lib.rm_window_locate_multi(self.be.ctx, self.h, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], kw["thr"], kw["threshold"], K,
                                                float(min_area), ctypes.c_void_p(xywh.ctypes.data), ctypes.c_void_p(area.ctypes.data), ctypes.byref(n),
                                                self.be.stream())
        m = max(n.value, 0)
        return rc, [tuple(int(v) for v in r) for r in xywh[:m]], [float(a) for a in area[:m]]


def contiguous(be, frames, levels, skip, flags=0, kw=KW):
    """rm_calibrate and rm_locate on a contiguous buffer -> (heat ndarray, rc of rm_locate, roi or None)"""
    frames = np.ascontiguousarray(frames)
    m, H, W = frames.shape[:3]
    code = code_of(frames)
    buf = be.dev(frames)
    heat = be.out((H, W))
    _capi.check(be.lib, be.lib.rm_calibrate(be.ctx, be.p(buf), code, m, H, W, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], levels, skip, kw["thr"],
                                            flags, be.p(heat), None, be.stream()), "rm_calibrate")
    xywh = np.full(4, -7, np.int32)
    rc = _capi.check(be.lib, be.lib.rm_locate(be.ctx, be.p(buf), code, m, H, W, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], levels, skip, kw["thr"],
                                              kw["threshold"], flags, ctypes.c_void_p(xywh.ctypes.data), be.stream()), "rm_locate")
    return be.np(heat), rc, (tuple(int(v) for v in xywh) if rc == _capi.RM_OK else None)


def shard_rows(be, frames, levels, skip, flags=0):
    """rm_shard_pyramid of the frames -> [n, NP] ndarray"""
    frames = np.ascontiguousarray(frames)
    n, H, W = frames.shape[:3]
    NP = ctypes.c_size_t()
    _capi.check(be.lib, be.lib.rm_shard_layout_flags(H, W, levels, skip, flags, ctypes.byref(NP)), "rm_shard_layout_flags")
    out = be.out((n, int(NP.value)))
    _capi.check(be.lib, be.lib.rm_shard_pyramid(be.ctx, be.p(be.dev(frames)), code_of(frames), n, H, W, levels, skip, flags, be.p(out), be.stream()),
                "rm_shard_pyramid")
    return be.np(out)


def same(win, frames, levels, skip, flags=0, tag=None):
    """the window's heatmap, return code and ROI equal those of the contiguous calls on `frames`; -> (rc, roi)"""
    want_heat, want_rc, want_roi = contiguous(win.be, frames, levels, skip, flags)
    got_heat = win.calibrate()
    assert np.array_equal(got_heat, want_heat, equal_nan=True), (tag, float(np.abs(got_heat - want_heat).max()))
    rc, roi = win.locate()
    assert (rc, roi) == (want_rc, want_roi), (tag, rc, roi, want_rc, want_roi)
    return rc, roi


# ---- case 1 -------------------------------------------------------------------------------------------------------------------
def check_every_head(be, geom, T, knobs):
    """Frame-by-frame pushes; after each, from count = 1 to 2T + 3, calibrate and locate against the contiguous last min(count, T)
    frames: the partly filled ring and every head position twice."""
    H, W, L, S = geom
    v = stream(T, H, W)
    full = []
    with Knobs(be, knobs), Window(be, T, H, W, L, S) as win:
        for k in range(1, 2 * T + 4):
            win.push_np(v[k - 1:k])
            m = min(k, T)
            assert win.info()[:2] == (m, k % T if k >= T else 0), (k, win.info())
            rc, roi = same(win, v[k - m:k], L, S, tag=(geom, T, knobs, k))
            if k >= T:
                full.append((rc, roi))
    # the stream does its job: over the full windows the blob has moved, and every one of them has a contour
    assert all(rc == _capi.RM_OK for rc, _ in full), full
    assert len({roi for _, roi in full}) > 1, full


# ---- case 2 -------------------------------------------------------------------------------------------------------------------
def check_granularity(be, geom, T):
    """n = 1, n = 3 (wraps mid-call), n = T and one n = T + 5 call, each followed by the same short tail: identical info, heatmap and ring;
    the ring is rm_shard_pyramid of the frames it holds, row by row."""
    H, W, L, S = geom
    v = stream(T, H, W)
    total = 2 * T + 5                     # T + 5 frames in the big call, then T more: every variant ends on the same frame
    results = []
    for how in ("ones", "threes", "Ts", "big"):
        with Window(be, T, H, W, L, S) as win:
            if how == "big":
                win.push_np(v[:T + 5])
                win.push_np(v[T + 5:total])
            else:
                n = {"ones": 1, "threes": 3, "Ts": T}[how]
                for a in range(0, total, n):
                    win.push_np(v[a:min(a + n, total)])
            results.append((how, win.info(), win.calibrate(), win.rows()))
    _, info0, heat0, rows0 = results[0]
    assert info0[:2] == (T, total % T)
    assert info0[3] == T * info0[2] * 8
    for how, info, heat, rows in results[1:]:
        assert info == info0, (how, info, info0)
        assert np.array_equal(heat, heat0), how
        assert np.array_equal(rows, rows0), how
    want = shard_rows(be, v[total - T:total], L, S)            # chronological; frame j of the stream sits in row j mod T
    for i in range(T):
        assert np.array_equal(rows0[(total - T + i) % T], want[i]), i
    with Window(be, T, H, W, L, S) as win:                     # and the one big call alone: its last T frames, nothing else
        win.push_np(v[:T + 5])
        assert win.info()[:2] == (T, 5 % T)
        same(win, v[5:T + 5], L, S, tag="n = T + 5")


# ---- case 3 -------------------------------------------------------------------------------------------------------------------
def check_dtypes(be, geom, T):
    H, W, L, S = geom
    v = stream(T, H, W)[:T + 3]
    for dt in (np.uint8, np.float16, np.float32, np.float64):
        frames = v if dt == np.uint8 else (v * (1. / 255)).astype(dt)
        with Window(be, T, H, W, L, S) as win:
            for a in range(0, T + 3, 2):
                win.push_np(frames[a:a + 2])
            n = T + 3
            same(win, frames[n - T:n], L, S, tag=np.dtype(dt).name)
    rng = np.random.default_rng(5)
    bgr = np.ascontiguousarray(np.clip(v[..., None].astype(np.int16) + rng.integers(-20, 21, v.shape + (3,)), 0, 255).astype(np.uint8))
    with Window(be, T, H, W, L, S) as win:
        for a in range(0, T + 3, 3):
            win.push_np(bgr[a:a + 3])
        n = T + 3
        same(win, bgr[n - T:n], L, S, tag="bgr8")
    # pushes that alternate uint8 and the float64 copies k * (1. / 255): the ring is float64 either way
    with Window(be, T, H, W, L, S) as a, Window(be, T, H, W, L, S) as b:
        for k in range(T + 3):
            a.push_np(v[k:k + 1])
            b.push_np(v[k:k + 1] if k % 2 == 0 else v[k:k + 1] * (1. / 255))
        assert np.array_equal(a.rows(), b.rows())
        assert np.array_equal(a.calibrate(), b.calibrate())
        assert a.locate() == b.locate()


# ---- case 4 -------------------------------------------------------------------------------------------------------------------
FLAGS = (_capi.RM_FLAG_FILTER_LAPLACIANS, _capi.RM_FLAG_UNFUSED_SMALL, _capi.RM_FLAG_NO_PRUNE, _capi.RM_FLAG_DENSE_SUM)


def check_flag(be, geom, T, flag):
    H, W, L, S = geom
    v = stream(T, H, W)
    n = T + T // 2 + 1
    with Window(be, T, H, W, L, S, flags=flag) as win:
        for a in range(0, n, 3):
            win.push_np(v[a:min(a + 3, n)])
        assert win.info()[1] == n % T != 0
        same(win, v[n - T:n], L, S, flags=flag, tag=flag)


# ---- case 7 -------------------------------------------------------------------------------------------------------------------
def check_argument_errors(be):
    lib, ctx = be.lib, be.ctx
    H, W, L, S = SMALL
    T = 10
    h = ctypes.c_void_p(1)
    assert lib.rm_window_create(ctx, T, H, W, L, 0, 0, ctypes.byref(h)) == _capi.RM_E_BADARG and not h.value
    assert lib.rm_window_create(ctx, 4097, H, W, L, S, 0, ctypes.byref(h)) == _capi.RM_E_UNSUPPORTED and not h.value
    assert lib.rm_window_create(ctx, 0, H, W, L, S, 0, ctypes.byref(h)) == _capi.RM_E_BADARG
    assert lib.rm_window_create(None, T, H, W, L, S, 0, ctypes.byref(h)) == _capi.RM_E_BADARG
    assert lib.rm_window_create(ctx, T, H, W, L, S, 0, None) == _capi.RM_E_BADARG
    assert lib.rm_window_destroy(None) == _capi.RM_OK
    v = stream(T, H, W)
    buf = be.dev(np.ascontiguousarray(v[:2]))
    with Window(be, T, H, W, L, S) as win:
        heat = be.out((H, W))
        xywh = np.zeros(4, np.int32)
        xp = ctypes.c_void_p(xywh.ctypes.data)
        a = (KW["fps"], KW["fmin"], KW["fmax"], KW["amp"], KW["thr"])
        # nothing held yet
        assert lib.rm_window_calibrate(ctx, win.h, *a, be.p(heat), be.stream()) == _capi.RM_E_BADARG
        assert lib.rm_window_locate(ctx, win.h, *a, 20, xp, be.stream()) == _capi.RM_E_BADARG
        assert win.locate_multi(4)[0] == _capi.RM_E_BADARG
        for n in (0, -1):
            assert lib.rm_window_push(ctx, win.h, be.p(buf), _capi.RM_U8, n, be.stream()) == _capi.RM_E_BADARG
        assert lib.rm_window_push(ctx, win.h, None, _capi.RM_U8, 1, be.stream()) == _capi.RM_E_BADARG
        assert lib.rm_window_push(ctx, None, be.p(buf), _capi.RM_U8, 1, be.stream()) == _capi.RM_E_BADARG
        assert lib.rm_window_push(None, win.h, be.p(buf), _capi.RM_U8, 1, be.stream()) == _capi.RM_E_BADARG
        for bad in (-1, 5, 99):
            assert lib.rm_window_push(ctx, win.h, be.p(buf), bad, 1, be.stream()) == _capi.RM_E_BADARG
        assert win.info()[:2] == (0, 0)                      # a refused push leaves the window as it was
        win.push(buf, _capi.RM_U8, 2)
        assert lib.rm_window_calibrate(ctx, win.h, *a, None, be.stream()) == _capi.RM_E_BADARG
        assert lib.rm_window_calibrate(ctx, None, *a, be.p(heat), be.stream()) == _capi.RM_E_BADARG
        assert lib.rm_window_calibrate(None, win.h, *a, be.p(heat), be.stream()) == _capi.RM_E_BADARG
        assert lib.rm_window_calibrate(ctx, win.h, 0.0, *a[1:], be.p(heat), be.stream()) == _capi.RM_E_BADARG
        assert lib.rm_window_locate(ctx, win.h, *a, 20, None, be.stream()) == _capi.RM_E_BADARG
        for kw in (dict(K=0), dict(K=_capi.RM_MAX_ROIS + 1), dict(K=4, min_area=-1.0), dict(K=4, min_area=float("nan"))):
            assert win.locate_multi(**kw)[0] == _capi.RM_E_BADARG, kw
        assert lib.rm_window_info(None, None, None, None, None) == _capi.RM_E_BADARG
        assert lib.rm_window_info(win.h, None, None, None, None) == _capi.RM_OK
        assert lib.rm_window_reset(ctx, None) == _capi.RM_E_BADARG and lib.rm_window_reset(None, win.h) == _capi.RM_E_BADARG
        assert win.calibrate_rc()[0] == _capi.RM_OK
    # nothing filtered (skip >= levels - 1): no ring, a zero heatmap, and the return code of rm_locate on the same frames
    with Window(be, T, H, W, 3, 2) as win:
        assert win.info()[2:] == (0, 0)
        win.push_np(v[:T + 2])
        assert win.info()[:2] == (T, 2)
        want_heat, want_rc, want_roi = contiguous(be, v[2:T + 2], 3, 2)
        assert want_rc == _capi.RM_NO_CONTOUR and not want_heat.any()
        got = win.calibrate()
        assert np.array_equal(got, want_heat)
        assert win.locate() == (want_rc, want_roi)
