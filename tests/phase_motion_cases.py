"""Shared by tests/test_emu_phase_motion.py and tests/test_gpu_phase_motion.py (not a test module): the clips, thin callers of
rm_phase_motion_* on raw pointers and the checks both builds run against tests/phase_motion_reference.py.  A backend `be` hides where
the memory lives (as in tests/phase_cases.py):
    be.lib, be.ctx, be.stream()                 the bound library, a context, the stream argument
    be.dev(ndarray) -> buffer                   an array where the library reads it (numpy itself on the host-emulated build)
    be.p(buffer) -> c_void_p                    its address
    be.debug_set(key, value)                    rm_debug_set on the context

Tolerance (derived, not chosen).  The per-pixel terms are reproducible bit for bit except for atan2.  The reference value of a sum is
math.fsum of the unperturbed terms; a build must agree within (n - 1) 2^-53 sum |term| + 64 D, n the pixels of the level: the first
term bounds ANY summation order of n terms (on the main case numpy's pairwise sum lands at 0.0015 of it, a plain left-to-right sum at 0.019),
D is the largest deviation, over the frames of the case, of the fsum of three perturbed reference runs (seeds 11, 12, 13; every inexact
atan2 times 1 + k 2^-52, k in -4 .. 4) from the unperturbed one, and 64 is the factor argued in tests/phase_cases.py.  A wrong tap,
sign or weight shows at 1e-3 of the sums.

D as measured on the CPU (numpy 2, glibc), (Sw, Sc, Ss), for the record -- the tests compute it afresh:"""
import ctypes
import functools
import os

import numpy as np

from respmon_amd import _capi, synth
from tests import phase_motion_reference as pmr

RECORDED_D = {
    "roi_l0": (0, 2.8e-17, 1.1e-16), "roi_l1": (0, 1.4e-17, 2.8e-17), "roi_l2": (0, 3.3e-19, 8.7e-19), "whole_l0": (0, 0, 0),
    "edge_l2": (0, 3.3e-19, 6.5e-19), "tiny_l1": (0, 2.7e-19, 3.3e-19), "tiny_l2": (0, 0, 0), "one_px": (0, 0, 0), "row_9x1": (0, 4.3e-19, 0),
    "col_1x9": (0, 0, 2.7e-19), "roi_l1_N1": (0, 0, 0), "roi_l1_N2": (0, 1.4e-17, 2.8e-17), "roi_l1_u16": (0, 1.4e-17, 2.8e-17),
    "roi_l1_f16": (0, 1.4e-17, 2.8e-17), "roi_l1_f32": (0, 1.4e-17, 2.8e-17), "roi_l1_f64": (0, 1.4e-17, 2.8e-17),
}

DT = {np.dtype(np.uint8): _capi.RM_U8, np.dtype(np.uint16): _capi.RM_U16, np.dtype(np.float16): _capi.RM_F16,
      np.dtype(np.float32): _capi.RM_F32, np.dtype(np.float64): _capi.RM_F64}
FPS, T, H, W = 10.0, 48, 96, 128
ROI = (20, 16, 64, 48)
FACTOR = 64
SENTINEL = -7.0


# ---- the clips -------------------------------------------------------------------------------------------------------------------
def displacement():
    t = np.arange(T)
    return 0.15 * np.sin(2 * np.pi * 0.4 * t / FPS), 0.4 * np.sin(2 * np.pi * 0.4 * t / FPS)


@functools.lru_cache(maxsize=None)
def _clip_u8():
    render = synth.synth_texture(H, W)
    dx, dy = displacement()
    k = np.stack([render(dx[t], dy[t]) for t in range(T)])
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def clip(kind="u8"):
    """synth_texture(96, 128) moving by (dx, dy), 48 frames: uint8, uint16 (256 k + 77), float64 ((k + 0.37) / 255), that as float32 / float16"""
    k = _clip_u8()
    if kind == "u8":
        return k
    if kind == "u16":
        v = (k.astype(np.uint16) * 256 + 77).astype(np.uint16)
    else:
        v = (k + 0.37) / 255
        if kind != "f64":
            v = v.astype({"f32": np.float32, "f16": np.float16}[kind])
    v.setflags(write=False)
    return v


# name -> (kind, frames, roi, level)
CASES = {
    "roi_l0": ("u8", T, ROI, 0), "roi_l1": ("u8", T, ROI, 1), "roi_l2": ("u8", T, ROI, 2),
    "whole_l0": ("u8", 6, (0, 0, W, H), 0),               # 2 x 24 tiles, wider than a wave
    "edge_l2": ("u8", 12, (91, 67, 37, 29), 2),           # odd sizes, touching the right and bottom frame edges: level 10 x 8
    "tiny_l1": ("u8", 12, (3, 5, 5, 7), 1),               # level 3 x 4
    "tiny_l2": ("u8", 12, (3, 5, 5, 7), 2),               # level 2 x 2, G_3 is 1 x 1
    "one_px": ("u8", 12, (77, 31, 1, 1), 0),
    "row_9x1": ("u8", 12, (60, 40, 9, 1), 1),
    "col_1x9": ("u8", 12, (60, 40, 1, 9), 0),
    "roi_l1_N1": ("u8", 1, ROI, 1), "roi_l1_N2": ("u8", 2, ROI, 1),
    "roi_l1_u16": ("u16", 12, ROI, 1), "roi_l1_f16": ("f16", 12, ROI, 1), "roi_l1_f32": ("f32", 12, ROI, 1), "roi_l1_f64": ("f64", 12, ROI, 1),
}


def frames_of(name):
    kind, n, roi, level = CASES[name]
    return clip(kind)[:n], roi, level


@functools.lru_cache(maxsize=None)
def reference(name):
    """(ref [n,3]: the fsum of the unperturbed terms, tol [n,3], D [3], pixels of the level)"""
    f, roi, level = frames_of(name)
    tr = pmr.terms(f, roi, level)
    ref = pmr.fsums(tr)
    D = np.zeros(3)
    for seed in (11, 12, 13):
        D = np.maximum(D, np.abs(pmr.fsums(pmr.terms(f, roi, level, perturb_seed=seed)) - ref).max(axis=0))
    n = tr[0][0].size
    tol = (n - 1) * 2.0 ** -53 * pmr.abs_sums(tr) + FACTOR * D[None, :]
    ref.setflags(write=False)
    return ref, tol, D, n


# ---- thin callers ---------------------------------------------------------------------------------------------------------------
class Session:
    def __init__(self, be, w, h, level):
        self.be, self.w, self.h, self.level = be, w, h, level
        self.handle = ctypes.c_void_p()
        _capi.check(be.lib, be.lib.rm_phase_motion_create(be.ctx, w, h, level, ctypes.byref(self.handle)), "rm_phase_motion_create")

    def info(self):
        seen, lh, lw, b = ctypes.c_longlong(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t()
        _capi.check(self.be.lib, self.be.lib.rm_phase_motion_info(self.handle, ctypes.byref(seen), ctypes.byref(lh), ctypes.byref(lw), ctypes.byref(b)),
                    "rm_phase_motion_info")
        return seen.value, lh.value, lw.value, b.value

    def reset(self):
        _capi.check(self.be.lib, self.be.lib.rm_phase_motion_reset(self.be.ctx, self.handle), "rm_phase_motion_reset")

    def clip_rc(self, frames, x, y, n=None, dtype=None, null=(), ctx="be"):
        """the raw return code of rm_phase_motion_clip with the output prefilled by a sentinel; `null`: arguments passed as NULL"""
        be = self.be
        f = np.ascontiguousarray(frames)
        N, Hf, Wf = f.shape
        d = be.dev(f)
        n = N if n is None else n
        out = np.full((max(min(n, N), 1), 3), SENTINEL)
        rc = be.lib.rm_phase_motion_clip(be.ctx if ctx == "be" else ctx, None if "state" in null else self.handle, None if "frames" in null else be.p(d),
                                         DT[f.dtype] if dtype is None else dtype, n, Hf, Wf, x, y,
                                         None if "sums" in null else ctypes.c_void_p(out.ctypes.data), be.stream())
        return rc, out

    def clip(self, frames, x, y):
        rc, out = self.clip_rc(frames, x, y)
        _capi.check(self.be.lib, rc, "rm_phase_motion_clip")
        return out

    def close(self):
        if self.handle:
            self.be.lib.rm_phase_motion_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def multi_rc(be, handles, frames, rois, n=None, k=None, dtype=None, null=()):
    f = np.ascontiguousarray(frames)
    N, Hf, Wf = f.shape
    d = be.dev(f)
    r = np.ascontiguousarray(rois, np.int32).reshape(-1, 4)
    n = N if n is None else n
    K = len(r) if k is None else k
    hs = (ctypes.c_void_p * max(len(handles), 1))(*[getattr(h, "value", h) for h in handles])
    out = np.full((max(min(n, N), 1), max(min(K, len(r)), 1), 3), SENTINEL)
    rc = be.lib.rm_phase_motion_multi_clip(be.ctx, None if "states" in null else hs, None if "frames" in null else be.p(d),
                                           DT[f.dtype] if dtype is None else dtype, n, Hf, Wf, None if "rois" in null else ctypes.c_void_p(r.ctypes.data), K,
                                           None if "sums" in null else ctypes.c_void_p(out.ctypes.data), be.stream())
    return rc, out


def multi(be, sessions, frames, rois):
    rc, out = multi_rc(be, [s.handle for s in sessions], frames, rois)
    _capi.check(be.lib, rc, "rm_phase_motion_multi_clip")
    return out


def level_size(w, h, level):
    for _ in range(level):
        w, h = (w + 1) // 2, (h + 1) // 2
    return h, w


def run_case(be, name):
    f, roi, level = frames_of(name)
    with Session(be, roi[2], roi[3], level) as s:
        lh, lw = level_size(roi[2], roi[3], level)
        info = s.info()
        assert info[:3] == (0, lh, lw) and 8 * lh * lw <= info[3] <= 32 * lh * lw, info
        got = s.clip(f, roi[0], roi[1])
        assert s.info()[0] == len(f)
    return got


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_reference_case(be, name):
    """case 1: every sum of every frame within (n - 1) 2^-53 sum |term| + 64 D of the reference's fsum"""
    ref, tol, D, n = reference(name)
    got = run_case(be, name)
    assert got.shape == ref.shape and np.isfinite(got).all(), name
    err = np.abs(got - ref)
    worst = float((err / np.where(tol > 0, tol, 1.0)).max())
    print("%s: %d pixels, max |error| (Sw, Sc, Ss) %s, D %s (recorded %s), largest error / bound %.3g"
          % (name, n, err.max(axis=0), D, RECORDED_D.get(name), worst))
    assert np.array_equal(got[0], np.zeros(3)), name                       # the first frame after create
    assert (got[:, 0] >= 0).all()
    assert (err <= tol).all(), (name, err.max(axis=0), tol.max(axis=0))
    if name == "one_px":
        assert np.array_equal(got[:, 1:], np.zeros((len(got), 2)))         # a 1 x 1 level: R1 = R2 = 0, Sc = Ss = 0 exactly
    if len(ref) > 2 and name != "one_px":
        assert (np.abs(ref[1:, 0]) > 0).all()                              # the case is not vacuous


def check_reference_sees_a_wrong_tap():
    """what the bound is for: a changed weight moves the sums by far more than it allows"""
    ref, tol, D, n = reference("roi_l1")
    f, roi, level = frames_of("roi_l1")
    tw, tc, ts = pmr.terms(f, roi, level)
    lvl = pmr.level_of(f, roi, level)
    wrong = pmr.fsums((tw, tc * (1 + 1e-3), ts))
    assert (np.abs(wrong[1:, 1] - ref[1:, 1]) > 100 * tol[1:, 1]).all() and lvl.shape[1:] == level_size(roi[2], roi[3], level)
    assert (D[1:] < 1e-15).all() and D[0] == 0.0


def check_zeros_and_constants(be):
    """case 2"""
    x, y, w, h = ROI
    with Session(be, w, h, 1) as s:
        got = s.clip(np.zeros((6, H, W), np.uint8), x, y)
        assert np.array_equal(got, np.zeros((6, 3)))                       # all-zero frames: exactly (0, 0, 0), +0.0
        assert not np.signbit(got).any()
        s.reset()
        got = s.clip(np.full((6, H, W), 100, np.uint8), x, y)
        assert np.array_equal(got[:, 1:], np.zeros((6, 2))) and np.array_equal(got[0], np.zeros(3))
        assert (got[1:, 0] >= 0).all()
        # the first frame after create and after reset gives zeros, whatever came before
        f = clip()[:5]
        a = s.clip(f, x, y)
        assert s.info()[0] == 11 and (a[:, 0] > 0).all()
        s.reset()
        assert s.info()[0] == 0
        b = s.clip(f, x, y)
        assert np.array_equal(b[0], np.zeros(3)) and (b[1:, 0] > 0).all() and np.array_equal(b[1:], a[1:])
    with Session(be, w, h, 1) as s2:
        assert np.array_equal(s2.clip(f, x, y), b)


CUTS = ((48,), (1, 47), (5, 7, 36), (1,) * 48)


def _in_cuts(s, f, x, y, cut):
    parts, k = [], 0
    for n in cut:
        parts.append(s.clip(f[k:k + n], x, y))
        k += n
        assert s.info()[0] == k
    return np.concatenate(parts)


def check_cuts(be):
    """case 3: every cut of one sequence gives the bits of one call, the library's own chunks included, and leaves the same state"""
    x, y, w, h = ROI
    f, more = clip(), clip()[::-1][:9]
    with Session(be, w, h, 1) as s:
        whole = _in_cuts(s, f, x, y, CUTS[0])
        after = s.clip(more, x, y)
        for cut in CUTS[1:]:
            s.reset()
            assert np.array_equal(_in_cuts(s, f, x, y, cut), whole), cut
            assert np.array_equal(s.clip(more, x, y), after), cut
        for chunk in (5, 7, 1):                                            # 10, 7 and 48 internal chunks: both parities of the state's planes
            s.reset()
            be.debug_set("phase_motion_frames", chunk)
            try:
                assert np.array_equal(s.clip(f, x, y), whole), chunk
            finally:
                be.debug_set("phase_motion_frames", 0)
            assert s.info()[0] == T and np.array_equal(s.clip(more, x, y), after), chunk


def check_dtypes_equal_their_widened_forms(be):
    """case 3: a uint8 buffer against the float64 buffer holding k * (1./255), uint16 against k * (1./65535), float16 / float32 widened"""
    x, y, w, h = ROI
    for kind in ("u8", "u16", "f16", "f32"):
        v = clip(kind)[:10]
        wide = v * (1. / 255) if kind == "u8" else v.astype(np.float64) * (1. / 65535) if kind == "u16" else v.astype(np.float64)
        assert wide.dtype == np.float64
        for level in (0, 2):
            with Session(be, w, h, level) as a, Session(be, w, h, level) as b:
                assert np.array_equal(a.clip(v, x, y), b.clip(wide, x, y)), (kind, level)


MULTI_ROIS = [ROI, (50, 20, 37, 29), ROI]           # the second overlaps the first; the third repeats it, with its own state
MULTI_LEVELS = [1, 2, 1]


def check_multi_equals_singles(be):
    """case 3: K = 3 against three single calls -- outputs, rm_phase_motion_info and the states left behind --, then single and multi
    calls mixed on the states, a K = 1 multi call, and the multi call under the library's own chunking"""
    f = clip()
    rois, levels = MULTI_ROIS, MULTI_LEVELS
    A = [Session(be, r[2], r[3], l) for r, l in zip(rois, levels)]      # multi first
    B = [Session(be, r[2], r[3], l) for r, l in zip(rois, levels)]      # singles first
    try:
        ma = multi(be, A, f[:20], rois)
        sb = np.stack([s.clip(f[:20], r[0], r[1]) for s, r in zip(B, rois)], axis=1)
        assert ma.shape == (20, 3, 3) and np.array_equal(ma, sb)
        assert np.array_equal(ma[:, 0], ma[:, 2]) and (ma[1:, :, 0] > 0).all()
        assert [s.info() for s in A] == [s.info() for s in B] and A[1].info()[:3] == (20, 8, 10)
        # the states left behind: continue each side in the OTHER form
        sa = np.stack([s.clip(f[20:31], r[0], r[1]) for s, r in zip(A, rois)], axis=1)
        mb = multi(be, B, f[20:31], rois)
        assert np.array_equal(sa, mb)
        # ... and mixed further: one frame at a time, a multi call of one subject, chunked multi calls
        one_a = np.stack([multi(be, A[k:k + 1], f[31:33], rois[k:k + 1])[:, 0] for k in range(3)], axis=1)
        one_b = np.concatenate([multi(be, B, f[31:32], rois), multi(be, B, f[32:33], rois)])
        assert np.array_equal(one_a, one_b)
        be.debug_set("phase_motion_frames", 4)
        try:
            ca = multi(be, A, f[33:], rois)
        finally:
            be.debug_set("phase_motion_frames", 0)
        cb = multi(be, B, f[33:], rois)
        assert np.array_equal(ca, cb) and [s.info() for s in A] == [s.info() for s in B] and A[0].info()[0] == T
        # the whole sequence of subject 0 is the single-call sequence of check_cuts
        with Session(be, ROI[2], ROI[3], 1) as s:
            whole = s.clip(f, ROI[0], ROI[1])
        assert np.array_equal(np.concatenate([ma[:, 0], sa[:, 0], one_a[:, 0], ca[:, 0]]), whole)
        # another order of the subjects, other neighbours: the same numbers per subject
        for s in A:
            s.reset()
        perm = [2, 0, 1]
        mp = multi(be, [A[k] for k in perm], f[:20], [rois[k] for k in perm])
        assert np.array_equal(mp[:, [1, 2, 0]], ma)
    finally:
        for s in A + B:
            s.close()


def check_purpose(be):
    """case 4, on the library's own output: the running sum of v follows the true displacement"""
    x, y, w, h = ROI
    f = clip()
    with Session(be, w, h, 1) as s:
        sums = s.clip(f, x, y)
    return purpose_criteria(sums, "library")


def purpose_criteria(sums, who):
    x, y, w, h = ROI
    dx, dy = displacement()
    pos = np.cumsum(pmr.velocity(sums), axis=0)
    cx, cy = float(np.corrcoef(pos[:, 0], dx)[0, 1]), float(np.corrcoef(pos[:, 1], dy)[0, 1])
    kx, ky = float(np.polyfit(dx, pos[:, 0], 1)[0]), float(np.polyfit(dy, pos[:, 1], 1)[0])
    mean = clip()[:, y:y + h, x:x + w].reshape(T, -1).mean(axis=1)
    cm = max(abs(float(np.corrcoef(mean, dx)[0, 1])), abs(float(np.corrcoef(mean, dy)[0, 1])))
    print("%s: correlation of the summed phase velocity with dx %.6f, with dy %.6f; slopes %.3f, %.3f rad/px; |correlation| of the ROI mean %.3f"
          % (who, cx, cy, kx, ky, cm))
    assert cx >= 0.999 and cy >= 0.999, (who, cx, cy)
    assert kx > 0 and ky > 0, (who, kx, ky)
    return cx, cy, kx, ky


def check_refusals(be):
    """case 5: the documented code, sentinel-filled outputs untouched, frames_seen unchanged"""
    E, U, OK = _capi.RM_E_BADARG, _capi.RM_E_UNSUPPORTED, _capi.RM_OK
    lib = be.lib
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    assert lib.rm_phase_motion_create(None, 8, 8, 0, out) == E and lib.rm_phase_motion_create(be.ctx, 8, 8, 0, None) == E
    assert lib.rm_phase_motion_create(be.ctx, 0, 8, 0, out) == E and lib.rm_phase_motion_create(be.ctx, 8, 0, 0, out) == E
    assert lib.rm_phase_motion_create(be.ctx, 8, 8, -1, out) == E
    assert lib.rm_phase_motion_create(be.ctx, 8, 8, 9, out) == U and not h
    assert lib.rm_phase_motion_create(be.ctx, 8, 8, 8, out) == OK and h
    assert lib.rm_phase_motion_destroy(h) == OK and lib.rm_phase_motion_destroy(None) == OK
    assert lib.rm_phase_motion_info(None, None, None, None, None) == E and lib.rm_phase_motion_reset(be.ctx, None) == E

    x, y, w, hh = ROI
    f = clip()[:4]
    untouched = lambda o: np.array_equal(o, np.full(o.shape, SENTINEL))
    with Session(be, w, hh, 1) as s, Session(be, w, hh, 1) as s2, Session(be, 37, 29, 1) as s3:
        assert lib.rm_phase_motion_reset(None, s.handle) == E
        assert lib.rm_phase_motion_info(s.handle, None, None, None, None) == OK
        s.clip(f[:2], x, y)
        rcs = []

        def single(code, **kw):
            rc, o = s.clip_rc(f, kw.pop("x", x), kw.pop("y", y), **kw)
            rcs.append(rc)
            assert rc == code and untouched(o) and s.info()[0] == 2, (code, rc, kw, lib.rm_last_error_string())
        single(E, ctx=None)
        for name in ("state", "frames", "sums"):
            single(E, null=(name,))
        single(E, n=0); single(E, n=-1)
        single(E, dtype=5); single(E, dtype=99); single(E, dtype=-1)
        single(U, dtype=_capi.RM_BGR8)
        single(E, x=W - w + 1); single(E, y=H - hh + 1); single(E, x=-1); single(E, y=-1)

        hs, rois = [s.handle, s2.handle, s3.handle], [ROI, ROI, (50, 20, 37, 29)]

        def many(code, handles=hs, rois=rois, text=None, **kw):
            rc, o = multi_rc(be, handles, f, rois, **kw)
            msg = lib.rm_last_error_string()
            assert rc == code and untouched(o), (code, rc, kw, msg)
            assert (s.info()[0], s2.info()[0], s3.info()[0]) == (2, 0, 0)
            assert text is None or text in msg, msg
        many(E, k=0); many(E, k=-1)
        many(E, handles=hs + [h] * (_capi.RM_MAX_ROIS - 2), rois=rois + [ROI] * (_capi.RM_MAX_ROIS - 2), k=_capi.RM_MAX_ROIS + 1)
        many(E, n=0)
        for name in ("states", "frames", "rois", "sums"):
            many(E, null=(name,))
        many(E, handles=[s.handle, None, s3.handle], text=b"subject 1")
        many(E, dtype=5); many(U, dtype=_capi.RM_BGR8)
        many(E, rois=[ROI, (W - w + 1, y, w, hh), (50, 20, 37, 29)], text=b"rectangle 1")
        many(E, rois=[ROI, ROI, (92, 20, 37, 29)], text=b"rectangle 2")
        many(E, rois=[ROI, ROI, (50, 20, 36, 29)], text=b"subject 2")          # another size than its state
        many(E, rois=[ROI, ROI, (50, 20, 37, 0)])
        many(E, handles=[s.handle, s2.handle, s.handle], rois=[ROI, ROI, ROI], text=b"subject 2")   # the same state twice
        # ... and the states still work: the refusals left them alone
        got = multi(be, [s, s2, s3], f[2:], rois)
        with Session(be, w, hh, 1) as t:
            want = t.clip(f, x, y)
        assert np.array_equal(got[:, 0], want[2:]) and np.array_equal(got[0, 1], np.zeros(3))


def check_declared(lib):
    """case 6"""
    names = ["rm_phase_motion_create", "rm_phase_motion_destroy", "rm_phase_motion_reset", "rm_phase_motion_info", "rm_phase_motion_clip",
             "rm_phase_motion_multi_clip"]
    assert all(n in _capi.SIGNATURES for n in names) and all(hasattr(lib, n) for n in names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "respmon_hip.h")).read()
    assert all(("int %s(" % n) in header for n in names) and "typedef struct rm_phase_motion rm_phase_motion;" in header
    assert lib.rm_abi_version() == 1


# ---- case 7: the Python layer, on monitors and trackers the test files build on their backend -------------------------------------------
SIGNALS = ("data", "t", "freq", "filtered_data", "peak_indices", "peak_times")


def assert_same_signal(a, b, what):
    def arr(v):
        return np.array(v, dtype=np.float64)
    for name in SIGNALS:
        assert np.array_equal(arr(getattr(a, name)), arr(getattr(b, name)), equal_nan=True), (what, name)
    assert [v is np.nan for v in a.data] == [v is np.nan for v in b.data], what
    assert np.array_equal(np.array(a.motion_data, np.float32), np.array(b.motion_data, np.float32)), what
    assert len(a.all_data) == len(b.all_data) and np.array_equal(arr(a.all_data), arr(b.all_data), equal_nan=True), what


def check_monitor(make_monitor, wrap=lambda a: a, frame_wrap=None):
    """step_clip on the whole clip, and in pieces, gives the values of the per-frame step() loop bit for bit; the first value is 0.0;
    all-zero frames lead to the error state a flow monitor without points reaches.  make_monitor(frames, roi, **attrs) -> a 'phase'
    monitor past skip_calibration(*roi); wrap: what a clip is handed over as (numpy, or a device tensor); frame_wrap: the same for the
    frames of the per-frame loop where that differs (step() takes the frame as next_frame() delivers it: on the device)"""
    f = np.array(clip())
    one_by_one = frame_wrap or wrap
    loop = make_monitor(f, ROI, measure_buffer_length=16)
    loop._add_benchmark_tags()                                             # (what run() and step_clip() do before their first step)
    for i in range(T):
        loop._step_frame(one_by_one(f)[i])
    assert loop.state == 'measure' and len(loop.all_data) == T and len(loop.data) == 16 and len(loop.motion_data) == 16
    assert loop.all_data[0][1] == 0.0 and loop.all_data[1][1] == 0.0 and all(np.isfinite(v) for _, v in loop.all_data)
    assert len(set(v for _, v in loop.all_data[2:])) > 30
    one = make_monitor(f, ROI, measure_buffer_length=16)
    assert one.step_clip(wrap(f)) == T
    assert_same_signal(one, loop, "one clip")
    parts = make_monitor(f, ROI, measure_buffer_length=16)
    assert parts.step_clip(wrap(f[:1])) == 1 and parts.step_clip(wrap(f[1:14])) == 13 and parts.step_clip(wrap(f[14:])) == T - 14
    assert_same_signal(parts, loop, "pieces")
    mixed = make_monitor(f, ROI, measure_buffer_length=16)
    mixed.step_clip(wrap(f[:7]))
    for i in range(7, 12):
        mixed._step_frame(one_by_one(f)[i])
    mixed.step_clip(wrap(f[12:]))
    assert_same_signal(mixed, loop, "clips and frames mixed")
    # the level is the monitor's phase_params
    l0 = make_monitor(f, ROI, phase_params=dict(level=0))
    l0.step_clip(wrap(f[:12]))
    assert l0._phase_state.level == 0 and one._phase_state.level == 1 and len(l0.motion_data) == 11
    # all-zero frames: Sw == 0, the value is np.nan itself and the monitor leaves 'measure' where a flow monitor without points does
    z = np.zeros((20, H, W), np.uint8)
    for form in ("clip", "loop"):
        mon = make_monitor(z, ROI)
        if form == "clip":
            n = mon.step_clip(wrap(z))
        else:
            n = 0
            mon._add_benchmark_tags()
            while mon.state == 'measure':
                mon._step_frame(one_by_one(z)[n])
                n += 1
        assert n == mon.measure_initialization_length + 1 and mon.state == 'error' and mon.error_message == "error detection found poor signal"
        assert mon.data[0] == 0.0 and all(v is np.nan for v in list(mon.data)[1:]) and len(mon.motion_data) == 0
    mon.reset()
    assert mon._phase_state is None and len(mon.data) == 0
    # a relocation that changes the ROI discards the session and the rows, one that confirms it keeps them
    moved, other = make_monitor(f, ROI), (50, 20, 37, 29)
    moved.step_clip(wrap(f[:6]))
    kept = moved._phase_state
    moved._set_roi(ROI)
    assert moved._phase_state is kept and len(moved.motion_data) == 5
    moved._set_roi(other)
    assert moved._phase_state is None and len(moved.motion_data) == 0 and (moved.x, moved.y, moved.w, moved.h) == other
    moved.step_clip(wrap(f[6:12]))
    fresh = make_monitor(f, other)
    fresh.step_clip(wrap(f[6:12]))
    assert list(moved.data)[6:] == list(fresh.data) and moved.data[6] == 0.0 and moved._phase_state.w == 37
    assert np.array_equal(np.array(moved.motion_data, np.float32), np.array(fresh.motion_data, np.float32))


def check_tracker(make_tracker, make_monitor, wrap=lambda a: a):
    """SubjectTracker('phase') with three rectangles equals three monitors value for value; restart(k) begins subject k again"""
    f = np.array(clip())
    rois = [ROI, (50, 20, 37, 29), (3, 5, 5, 7)]
    mons = []
    for r in rois:
        m = make_monitor(f, r, measure_buffer_length=16)
        m.step_clip(wrap(f[:30]))
        mons.append(m)
    for sizes in ([30], [1, 7, 22]):
        tr = make_tracker(rois, measure_buffer_length=16)
        k = 0
        for n in sizes:
            assert tr.step_clip(wrap(f[k:k + n])) == n
            k += n
        assert tr.lost == [False] * 3
        for j in range(3):
            assert_same_signal(tr[j], mons[j], (sizes, j))
    # subject 1 begins again, at another rectangle size; the others go on without a gap
    kept = len(tr[1].all_data)
    tr.restart(1, roi=(40, 30, 33, 21))
    assert len(tr[1].data) == 0 and len(tr[1].motion_data) == 0 and tr.rois[1] == (40, 30, 33, 21)
    tr.step_clip(wrap(f[30:]))
    fresh = make_monitor(f, (40, 30, 33, 21), measure_buffer_length=16)
    fresh.step_clip(wrap(f[30:]))
    for name in SIGNALS:
        assert np.array_equal(np.array(getattr(tr[1], name), float), np.array(getattr(fresh, name), float), equal_nan=True), name
    assert np.array_equal(np.array(tr[1].all_data[kept:], float), np.array(fresh.all_data, float)) and tr[1].all_data[kept][1] == 0.0
    mons[0].step_clip(wrap(f[30:]))
    assert_same_signal(tr[0], mons[0], "through the restart")
    # a subject on all-zero frames is lost where its monitor leaves 'measure'
    z = np.zeros((20, H, W), np.uint8)
    tr = make_tracker(rois[:2])
    assert tr.step_clip(wrap(z)) == 20 and tr.lost == [True, True] and tr[0].error_message == "error detection found poor signal"
    assert len(tr[0].data) == tr[0].measure_initialization_length + 1
