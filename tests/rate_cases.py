"""Shared by tests/test_emu_rate_map.py and tests/test_gpu_rate_map.py (not a test module): the rate map (include/respmon_hip.h
rm_spectral_operator / rm_spectral_peak / rm_rate_map / rm_window_rate_map) against a reference written here, thin callers of the
C-ABI on raw pointers, and the checks both builds run.  The backend `be` is the one of tests/window_cases.py plus
    be.out_i32(shape) -> buffer      an int32 result area filled with -7
    be.cus                           compute units the library sees (the form switch is at NP = 64 * 4 * cus)

THE REFERENCE is the definition of include/respmon_hip.h evaluated in wider arithmetic on the same float64 y = x - x[0]: the operator
in mpmath at 40 digits (np.longdouble's 64-bit mantissa is too narrow for the operator's own tolerance), the contraction, the powers,
the logarithms and the refinement in np.longdouble.  It shares nothing with rm_rate.hip.

TOLERANCES, derived, never fitted.  u = 2^-53, K = T + 8 (T terms of one dot product, 8 for the rounded operator entries and the two
squares), e_j = K u max((|A| |y|)_(2j), (|A| |y|)_(2j+1)) bounds the error of both c_j and s_j, so
    |P_j - P_ref,j| <= eP_j := 2 (|c_ref| + |s_ref|) e_j + 2 e_j^2 + 3 u P_ref,j
    |total - sum P_ref| <= sum_j eP_j + F u sum P_ref
    index: a pixel is ambiguous when the reference's best and second-best P lie within 2 max_j eP_j; elsewhere index == reference's;
           at most 1 % of a case's pixels may be ambiguous.  On EVERY pixel the library's index must be a near-maximum of the reference
           (P_ref[index] >= max P_ref - 2 max eP) and power must be P_ref[index] within eP[index].
    frequency, on unambiguous interior pixels, with dL_k = eP_k / P_k + 4 u |log P_k|:
           |delta - delta_ref| <= 2 [(dL- + dL+) |den| + |num| (dL- + 2 dL0 + dL+)] / (2 den^2)     (first order, doubled)
           asserted where that is below 1e-6 (at most 1 % of a case's pixels may lie above).  The library returns freq, not delta:
           freq = fl(fl(fmin + index step) + fl(delta step)) adds three roundings of values below fmax, so the assertion is
           |freq - freq_ref| <= bound * step + 3 u fmax.
    operator: |A_lib - A_ref| <= 4 u w[t] per entry -- see check_operator for where a correctly rounded entry can meet that."""
import ctypes
import functools

import numpy as np

from respmon_amd import _capi
from tests import window_cases as wc

U = 2.0 ** -53
LD = np.longdouble
BAND = dict(fps=10.0, fmin=0.4, fmax=1.0)
TS = (2, 3, 7, 16, 33, 64, 128)
FS = (3, 16, 17, 64)
NPS = (1, 15, 16, 17, 257)
NPMAX = 257


# ---- the reference -------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def _to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


@functools.lru_cache(maxsize=None)
def ref_operator(T, fps, fmin, fmax, F):
    """-> (A [2F, T] longdouble, freqs [F] float64, w [T] float64 (the window, rounded), step)"""
    mp = _mp()
    step = (fmax - fmin) / (F - 1)
    freqs = np.array([fmin + j * step for j in range(F)])
    two_pi = 2 * mp.pi
    w = [mp.mpf("0.35875") - mp.mpf("0.48829") * mp.cos(two_pi * t / (T - 1)) + mp.mpf("0.14128") * mp.cos(2 * two_pi * t / (T - 1))
         - mp.mpf("0.01168") * mp.cos(3 * two_pi * t / (T - 1)) for t in range(T)]
    A = np.zeros((2 * F, T), dtype=LD)
    for j in range(F):
        f = mp.mpf(float(freqs[j]))
        ang = [two_pi * f * t / mp.mpf(fps) for t in range(T)]
        for part in range(2):
            e = [w[t] * mp.cos(ang[t]) if part == 0 else -(w[t] * mp.sin(ang[t])) for t in range(T)]
            mean = mp.fsum(e) / T
            A[2 * j + part] = [_to_ld(v - mean) for v in e]
    A.setflags(write=False)
    return A, freqs, np.array([float(v) for v in w]), step


class Ref:
    """the definition on x [T, n] float64 (n columns of interest)"""

    def __init__(self, x, fps, fmin, fmax, F):
        T = x.shape[0]
        A, self.freqs, _, self.step = ref_operator(T, float(fps), float(fmin), float(fmax), F)
        y = x - x[0]                                  # one rounded subtraction per element, as the kernel forms it
        yl = y.astype(LD)
        C = A @ yl
        c, s = C[0::2], C[1::2]
        self.P = c * c + s * s
        absAy = np.abs(A) @ np.abs(yl)
        e = (T + 8) * U * np.maximum(absAy[0::2], absAy[1::2])
        self.eP = 2 * (np.abs(c) + np.abs(s)) * e + 2 * e * e + 3 * U * self.P
        self.F, self.fmax = F, fmax
        self.total = self.P.sum(axis=0)
        self.still = ~y.any(axis=0)
        self.index = np.where(self.still, -1, np.argmax(self.P, axis=0))
        srt = np.sort(self.P, axis=0)
        self.tol_idx = 2 * self.eP.max(axis=0)
        self.ambiguous = ~self.still & (srt[-1] - srt[-2] <= self.tol_idx)
        n = x.shape[1]
        self.delta = np.zeros(n, dtype=LD)
        self.delta_bound = np.zeros(n, dtype=LD)
        self.den = np.full(n, np.nan)
        cols = np.arange(n)
        inner = ~self.still & (self.index > 0) & (self.index < F - 1)
        for p in cols[inner]:
            i = self.index[p]
            Pm, P0, Pp = self.P[i - 1, p], self.P[i, p], self.P[i + 1, p]
            if not (Pm > 0 and P0 > 0 and Pp > 0):
                continue
            a, b, c3 = np.log(Pm), np.log(P0), np.log(Pp)
            num, den = a - c3, (a - 2 * b) + c3
            self.den[p] = float(den)
            if den < 0:
                self.delta[p] = min(max(0.5 * num / den, LD(-0.5)), LD(0.5))
                dL = [self.eP[k, p] / self.P[k, p] + 4 * U * abs(np.log(self.P[k, p])) for k in (i - 1, i, i + 1)]
                self.delta_bound[p] = 2 * ((dL[0] + dL[2]) * abs(den) + abs(num) * (dL[0] + 2 * dL[1] + dL[2])) / (2 * den * den)
            else:
                self.delta_bound[p] = np.inf      # the branch itself hangs on the sign of a near-zero den
        self.inner = inner
        self.freq = np.where(self.still, np.nan, self.freqs[np.maximum(self.index, 0)].astype(LD) + self.delta * LD(self.step))


def check_against(ref, freq, power, total, index, tag):
    """the four outputs (ndarrays over the reference's columns) against the tolerances of the module docstring; -> figures"""
    n = len(index)
    st = ref.still
    assert np.array_equal(index[st], np.full(st.sum(), -1)), tag
    assert np.all(np.isnan(freq[st])) and not power[st].any() and not total[st].any(), tag
    mv = ~st
    cols = np.arange(n)[mv]
    assert np.all((index[mv] >= 0) & (index[mv] < ref.F)), tag
    # every pixel: a near-maximum of the reference, its power, the total
    Pi = ref.P[index[mv], cols]
    assert np.all(Pi >= ref.P.max(axis=0)[mv] - ref.tol_idx[mv]), (tag, "index is no maximum of the reference")
    dp = np.abs(power[mv].astype(LD) - Pi)
    assert np.all(dp <= ref.eP[index[mv], cols]), (tag, "power", float(np.max(dp / ref.eP[index[mv], cols])))
    tot_tol = ref.eP.sum(axis=0) + ref.F * U * ref.total
    dt = np.abs(total[mv].astype(LD) - ref.total[mv])
    assert np.all(dt <= tot_tol[mv]), (tag, "total", float(np.max(dt / tot_tol[mv])))
    # index
    clear = mv & ~ref.ambiguous
    assert np.array_equal(index[clear], ref.index[clear]), (tag, "index")
    n_amb = int(ref.ambiguous.sum())
    assert n_amb <= 0.01 * n, (tag, "ambiguous pixels", n_amb, n)
    # frequency
    edge = clear & ~ref.inner
    assert np.array_equal(freq[edge], ref.freqs[index[edge]]), (tag, "delta must be 0 on the grid's ends")
    fin = clear & ref.inner
    tight = fin & (ref.delta_bound < 1e-6)
    n_loose = int((fin & ~tight).sum())
    assert n_loose <= 0.01 * n, (tag, "pixels whose frequency bound exceeds 1e-6", n_loose, n)
    df = np.abs(freq[tight].astype(LD) - ref.freq[tight])
    lim = ref.delta_bound[tight] * ref.step + 3 * U * ref.fmax
    assert np.all(df <= lim), (tag, "freq", float(np.max(df / lim)))
    return dict(ambiguous=n_amb, loose=n_loose, max_bound=float(ref.delta_bound[tight].max()) if tight.any() else 0.0,
                min_abs_den=float(np.nanmin(np.abs(ref.den))) if np.isfinite(ref.den).any() else float("nan"))


# ---- callers -------------------------------------------------------------------------------------------------------------------
class Outs:
    def __init__(self, be, n, want=(1, 1, 1, 1)):
        self.be = be
        self.bufs = [be.out((n,)) if want[0] else None, be.out((n,)) if want[1] else None, be.out((n,)) if want[2] else None,
                     be.out_i32((n,)) if want[3] else None]

    def ptrs(self):
        return [self.be.p(b) if b is not None else None for b in self.bufs]

    def np(self):
        return [self.be.np(b) if b is not None else None for b in self.bufs]

    def untouched(self):
        f, p, t, i = self.np()
        return all(v is None or np.all(np.isnan(v)) for v in (f, p, t)) and (i is None or np.all(i == -7))


def peak_rc(be, xd, T, NP, fps, fmin, fmax, F, outs):
    return be.lib.rm_spectral_peak(be.ctx, be.p(xd) if xd is not None else None, T, NP, fps, fmin, fmax, F, *outs.ptrs(), be.stream())


def peak(be, x, fps, fmin, fmax, F, want=(1, 1, 1, 1)):
    x = np.ascontiguousarray(x, dtype=np.float64)
    T, NP = x.shape
    outs = Outs(be, NP, want)
    _capi.check(be.lib, peak_rc(be, be.dev(x), T, NP, fps, fmin, fmax, F, outs), "rm_spectral_peak")
    return outs.np()


def rate_map_rc(be, fd, code, T, H, W, level, fps, fmin, fmax, F, outs):
    return be.lib.rm_rate_map(be.ctx, be.p(fd) if fd is not None else None, code, T, H, W, level, fps, fmin, fmax, F, *outs.ptrs(), be.stream())


def level_shape(H, W, level):
    for _ in range(level):
        H, W = (H + 1) // 2, (W + 1) // 2
    return H, W


def rate_map(be, frames, level, fps, fmin, fmax, F):
    frames = np.ascontiguousarray(frames)
    T, H, W = frames.shape[:3]
    h, w = level_shape(H, W, level)
    outs = Outs(be, h * w)
    _capi.check(be.lib, rate_map_rc(be, be.dev(frames), wc.code_of(frames), T, H, W, level, fps, fmin, fmax, F, outs), "rm_rate_map")
    return outs.np()


def window_rate_map_rc(be, win, fps, fmin, fmax, F, outs):
    return be.lib.rm_window_rate_map(be.ctx, win.h, fps, fmin, fmax, F, *outs.ptrs(), be.stream())


def pyr_down_n(be, frames, level):
    """rm_pyr_down applied `level` times to [T,H,W] frames of any dtype (a BGR buffer through rm_bgr_to_gray first) -> [T, h*w] float64"""
    frames = np.ascontiguousarray(frames)
    T, H, W = frames.shape[:3]
    cur, code = be.dev(frames), wc.code_of(frames)
    if frames.ndim == 4:
        gray = be.dev(np.zeros((T, H, W), np.uint8))
        _capi.check(be.lib, be.lib.rm_bgr_to_gray(be.ctx, be.p(cur), T * H * W, be.p(gray), be.stream()), "rm_bgr_to_gray")
        cur, code = gray, _capi.RM_U8
    h, w = H, W
    for _ in range(level):
        dst = be.out((T, (h + 1) // 2, (w + 1) // 2))
        _capi.check(be.lib, be.lib.rm_pyr_down(be.ctx, be.p(cur), code, T, h, w, be.p(dst), be.stream()), "rm_pyr_down")
        cur, code, h, w = dst, _capi.RM_F64, (h + 1) // 2, (w + 1) // 2
    return be.np(cur).reshape(T, h * w)


class Form:
    """rate_wide forced to 0 / 1, or left alone (None)"""

    def __init__(self, be, wide):
        self.be, self.wide = be, wide

    def __enter__(self):
        if self.wide is not None:
            _capi.check(self.be.lib, self.be.lib.rm_debug_set(self.be.ctx, b"rate_wide", self.wide), "rm_debug_set")

    def __exit__(self, *exc):
        _capi.check(self.be.lib, self.be.lib.rm_debug_set(self.be.ctx, b"rate_wide", -1), "rm_debug_set")


def same_outputs(a, b, tag):
    for name, u, v in zip(("freq", "power", "total", "index"), a, b):
        assert np.array_equal(u, v, equal_nan=(name != "index")), (tag, name)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signals(T, n, fps, seed, f_lo=0.45, f_hi=0.9):
    """[T, n]: 0.5 + 0.05 sin(2 pi f0 t / fps + phi), f0 in [f_lo, f_hi] per column; odd columns carry 2 % noise (sigma 0.001)"""
    rng = np.random.default_rng(seed)
    f0 = f_lo + (f_hi - f_lo) * rng.random(n)
    phi = 2 * np.pi * rng.random(n)
    t = np.arange(T)[:, None]
    x = 0.5 + 0.05 * np.sin(2 * np.pi * f0[None, :] * t / fps + phi[None, :])
    x[:, 1::2] += 0.001 * rng.standard_normal((T, (n + 0) // 2))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref_case1(T, F):
    x = signals(128, NPMAX, BAND["fps"], 11)[:T]
    return x, Ref(x, BAND["fps"], BAND["fmin"], BAND["fmax"], F)


class RefCols:
    """a Ref restricted to its first n columns (columns are independent)"""

    def __init__(self, r, n):
        for k in ("P", "eP"):
            setattr(self, k, getattr(r, k)[:, :n])
        for k in ("total", "still", "index", "tol_idx", "ambiguous", "delta", "delta_bound", "den", "inner", "freq"):
            setattr(self, k, getattr(r, k)[:n])
        self.F, self.fmax, self.freqs, self.step = r.F, r.fmax, r.freqs, r.step


# ---- operator ------------------------------------------------------------------------------------------------------------------
OPERATOR_CASES = ((128, 10.0, 0.45, 0.9, 64), (64, 10.0, 0.45, 0.9, 16), (33, 10.0, 0.45, 0.9, 17), (256, 30.0, 0.45, 0.9, 64), (2, 10.0, 0.4, 1.0, 3),
                  (7, 10.0, 0.4, 1.0, 17))


def check_operator(lib, case):
    """|A_lib - A_ref| <= 4 u w[t] per entry wherever a correctly rounded entry can meet it, and "long double, rounded once" everywhere.
    A[r, t] = E[r, t] - mean_r carries the row's mean, which at a band inside the window's main lobe (short T) is of order 0.1 while
    w[t] falls to 6e-5 at the ends: half an ulp of such an entry alone exceeds 4 u w[t] there (the correctly rounded reference itself
    misses the bound at 22 of 2048 entries at T = 64 and 149 of 1122 at T = 33).  So the 4 u w[t] bound is asserted on the entries with
    |A_ref| <= 4 w[t], where one rounding (u |A_ref|) fits under it, and on ALL entries what the construction promises: one rounding
    to double plus the error of a long-double evaluation (v = 2^-64) whose angles are reduced to less than one turn before they are
    rounded: 2 pi v for the angle and some eight more roundings in the window, the cosine and the product, 16 v w[t] for E, and
    16 v mean(w) for the row's mean."""
    T, fps, fmin, fmax, F = case
    A_ref, freqs, w, _ = ref_operator(T, fps, fmin, fmax, F)
    A = np.full((2 * F, T), np.nan)
    fr = np.full(F, np.nan)
    _capi.check(lib, lib.rm_spectral_operator(T, fps, fmin, fmax, F, ctypes.c_void_p(A.ctypes.data), ctypes.c_void_p(fr.ctypes.data)), "rm_spectral_operator")
    assert np.array_equal(fr, freqs)
    d = np.abs(A.astype(LD) - A_ref)
    v = LD(2.0) ** -64
    built = U * np.abs(A_ref) + 16 * v * (w[None, :] + w.mean())
    assert np.all(d <= built), (case, float(np.max(d / built)))
    meetable = np.abs(A_ref) <= 4 * w[None, :]
    assert np.all(d[meetable] <= 4 * U * np.broadcast_to(w[None, :], d.shape)[meetable]), case
    # A 1 == 0 up to rounding: the mean removal is folded in
    assert np.all(np.abs(A.astype(LD).sum(axis=1)) <= T * U * np.abs(A_ref).sum(axis=1)), case
    # either output may be NULL
    assert lib.rm_spectral_operator(T, fps, fmin, fmax, F, None, ctypes.c_void_p(fr.ctypes.data)) == _capi.RM_OK
    assert lib.rm_spectral_operator(T, fps, fmin, fmax, F, ctypes.c_void_p(A.ctypes.data), None) == _capi.RM_OK
    return float(meetable.mean()), float(np.max(d[meetable] / (4 * U * np.broadcast_to(w[None, :], d.shape)[meetable])))


# ---- case 1 --------------------------------------------------------------------------------------------------------------------
def check_peak(be, T, F):
    """every NP of NPS in both forms against the reference (computed once at 257 columns: columns are independent)"""
    x, ref = _ref_case1(T, F)
    figs = None
    for n in NPS:
        for wide in (0, 1):
            with Form(be, wide):
                got = peak(be, x[:, :n], BAND["fps"], BAND["fmin"], BAND["fmax"], F)
            figs = check_against(RefCols(ref, n), *got, tag=(T, F, n, wide))
    return figs


# ---- case 1 at NH = 3 (33 <= nfreq <= 48), the instance FS never selected ------------------------------------------------------------
NH3_FS = (33, 48)                       # the two ends of NH = 3
NH3_TS = (3, 16, 33, 128)
NH3_NPS = (1, 15, 16, 17, 63, 65)
# frames whose level 1 has exactly NP pixels, for the ring arm (rm_window_rate_map reads the window's own level-S rows)
NH3_RING_GEOMS = {1: (2, 2), 15: (6, 10), 16: (8, 8), 17: (2, 34), 63: (14, 18), 65: (10, 26)}


def reference_caps(ref, n, tag):
    """what check_against demands of the REFERENCE on its first n columns (no library): at most 1 % ambiguous pixels, at most 1 % whose
    frequency bound exceeds 1e-6"""
    r = RefCols(ref, n)
    mv = ~r.still
    n_amb = int(r.ambiguous.sum())
    assert n_amb <= 0.01 * n, (tag, "ambiguous pixels", n_amb, n)
    fin = mv & ~r.ambiguous & r.inner
    n_loose = int((fin & ~(r.delta_bound < 1e-6)).sum())
    assert n_loose <= 0.01 * n, (tag, "pixels whose frequency bound exceeds 1e-6", n_loose, n)


@functools.lru_cache(maxsize=None)
def ring_frames(N, H, W):
    """uint8 [N, H, W]: every pixel swings by 60 levels at a rate of its own inside RM_KW's band, plus two levels of noise"""
    rng = np.random.default_rng(100 * H + W)
    f0 = RM_KW["fmin"] + (RM_KW["fmax"] - RM_KW["fmin"]) * rng.random((1, H, W))
    t = np.arange(N)[:, None, None]
    v = 128 + 60 * np.sin(2 * np.pi * f0 * t / RM_KW["fps"] + 2 * np.pi * rng.random((1, H, W))) + rng.integers(-2, 3, (N, H, W))
    v = np.rint(v).astype(np.uint8)
    v.setflags(write=False)
    return v


def check_peak_form(be, T, F, wide, nps=NH3_NPS):
    """every NP of nps in ONE form against the reference (check_peak's inputs and reference)"""
    x, ref = _ref_case1(T, F)
    for n in nps:
        with Form(be, wide):
            got = peak(be, x[:, :n], BAND["fps"], BAND["fmin"], BAND["fmax"], F)
        check_against(RefCols(ref, n), *got, tag=(T, F, n, wide))


def check_ring_form(be, T, F, wide, nps=NH3_NPS):
    """the ring arm in one form: a window of T frames whose head has wrapped, rm_window_rate_map against rm_spectral_peak on the unrolled
    window (rm_pyr_down of the frames it holds) bit for bit, as check_window does"""
    kw = RM_KW
    for n in nps:
        H, W = NH3_RING_GEOMS[n]
        assert int(np.prod(level_shape(H, W, 1))) == n
        v = ring_frames(T + 2, H, W)
        k = T + 2                                     # two frames past a full window: the head is inside the ring
        with wc.Window(be, T, H, W, 3, 1) as win:
            win.push_np(v[:T])
            win.push_np(v[T:k])
            outs = Outs(be, n)
            with Form(be, wide):
                _capi.check(be.lib, window_rate_map_rc(be, win, kw["fps"], kw["fmin"], kw["fmax"], F, outs), "rm_window_rate_map")
                want = peak(be, pyr_down_n(be, v[k - T:k], 1), kw["fps"], kw["fmin"], kw["fmax"], F)
        same_outputs(outs.np(), want, ("ring", T, F, n, wide))
        assert (want[3] >= 0).all(), ("ring", T, F, n, wide)          # every pixel moves: the comparison is not one of empty maps


def sample_columns(n, k=96):
    """columns of a wide case that meet the reference: both ends and a spread"""
    rng = np.random.default_rng(n)
    return np.unique(np.concatenate([np.arange(min(n, 40)), np.arange(max(n - 70, 0), n), rng.integers(0, n, k)]))


def check_form_switch(be, T=16, F=16):
    """one NP either side of the switch, the form left to the library; the two sides take different kernels, which shows in nothing
    but the rounding -- so each is also compared with the SAME columns under the form it is said to take"""
    edge = 64 * 4 * be.cus
    x = signals(T, edge, BAND["fps"], 13)
    for n, wide in ((edge - 1, 0), (edge, 1)):
        with Form(be, None):
            got = peak(be, x[:, :n], BAND["fps"], BAND["fmin"], BAND["fmax"], F)
        with Form(be, wide):
            forced = peak(be, x[:, :n], BAND["fps"], BAND["fmin"], BAND["fmax"], F)
        same_outputs(got, forced, (n, wide))
        cols = sample_columns(n)
        check_against(Ref(x[:, cols], BAND["fps"], BAND["fmin"], BAND["fmax"], F), *(v[cols] for v in got), tag=("switch", n))


def check_long_wide(be, T=512, F=64, fps=30.0):
    """GPU only: T = 512 with NP = 64 * 4 * CUs + 1 (the wide form with a last workgroup of one column), sampled columns"""
    n = 64 * 4 * be.cus + 1
    x = signals(T, n, fps, 17)
    with Form(be, None):
        got = peak(be, x, fps, BAND["fmin"], BAND["fmax"], F)
    assert np.all(got[3] >= 0) and np.all(np.isfinite(got[0]))
    cols = sample_columns(n, 64)
    return check_against(Ref(x[:, cols], fps, BAND["fmin"], BAND["fmax"], F), *(v[cols] for v in got), tag="T=512")


# ---- case 2 --------------------------------------------------------------------------------------------------------------------
def check_degenerate(be, T=128, F=64):
    fps, fmin, fmax = BAND["fps"], BAND["fmin"], BAND["fmax"]
    step = (fmax - fmin) / (F - 1)
    t = np.arange(T)
    x = np.empty((T, 8))
    x[:, 0] = 0.37                                   # constant
    x[:, 1] = 0.0                                    # zeros
    x[:, 2] = 0.5; x[T // 2, 2] = 0.75               # differs in one frame
    x[:, 3] = 0.5; x[0, 3] = 0.25                    # ... which is frame 0: y is a step
    x[:, 4] = 0.5 + 0.05 * np.sin(2 * np.pi * fmin * t / fps + 0.3)                       # peak on the grid's first point
    x[:, 5] = 0.5 + 0.05 * np.sin(2 * np.pi * (fmin + (F - 1) * step) * t / fps + 1.1)    # ... and on its last
    x[:, 6] = 200.0                                  # a large constant
    x[:, 7] = 0.5 + 0.05 * np.sin(2 * np.pi * 0.7 * t / fps)
    ref = Ref(x, fps, fmin, fmax, F)
    assert ref.index[4] == 0 and ref.index[5] == F - 1 and not ref.ambiguous[4] and not ref.ambiguous[5]
    for wide in (0, 1):
        with Form(be, wide):
            full = peak(be, x, fps, fmin, fmax, F)
            freq, power, total, index = full
            for c in (0, 1, 6):
                assert index[c] == -1 and np.isnan(freq[c]) and power[c] == 0.0 and total[c] == 0.0 and not np.signbit(power[c]), (wide, c)
            assert index[4] == 0 and freq[4] == fmin, (wide, freq[4])
            assert index[5] == F - 1 and freq[5] == fmin + (F - 1) * step, (wide, freq[5])
            # every moving column, the nearly flat spectra of the single-frame ones included: the index is a near-maximum of the
            # reference, power and total lie within their bounds; where the reference is unambiguous the index is its own, and the
            # frequency lies within its bound where that is tight
            for c in (2, 3, 4, 5, 7):
                i = index[c]
                assert 0 <= i < F and ref.P[i, c] >= ref.P[:, c].max() - ref.tol_idx[c], (wide, c)
                assert abs(LD(power[c]) - ref.P[i, c]) <= ref.eP[i, c], (wide, c)
                assert abs(LD(total[c]) - ref.total[c]) <= ref.eP[:, c].sum() + F * U * ref.total[c], (wide, c)
                if not ref.ambiguous[c]:
                    assert i == ref.index[c], (wide, c)
                    if ref.inner[c] and ref.delta_bound[c] < 1e-6:
                        assert abs(LD(freq[c]) - ref.freq[c]) <= ref.delta_bound[c] * step + 3 * U * fmax, (wide, c)
            assert not ref.ambiguous[7] and ref.inner[7] and ref.delta_bound[7] < 1e-6
            # NULL outputs in every combination: what is asked for is what the full call gave
            for m in range(1, 15):
                want = tuple((m >> k) & 1 for k in range(4))
                part = peak(be, x, fps, fmin, fmax, F, want)
                for k in range(4):
                    assert (part[k] is None) == (not want[k])
                    if want[k]:
                        assert np.array_equal(part[k], full[k], equal_nan=(k < 3)), (wide, want, k)


# ---- case 3 --------------------------------------------------------------------------------------------------------------------
RM_KW = dict(fps=wc.KW["fps"], fmin=wc.KW["fmin"], fmax=wc.KW["fmax"], F=17)
RATE_GEOMS = ((70, 90, 1), (70, 90, 2), (33, 47, 1))


def dtype_variants(v):
    yield "u8", v
    for dt in (np.float16, np.float32, np.float64):
        yield np.dtype(dt).name, (v * (1. / 255)).astype(dt)
    rng = np.random.default_rng(5)
    yield "bgr8", np.ascontiguousarray(np.clip(v[..., None].astype(np.int16) + rng.integers(-20, 21, v.shape + (3,)), 0, 255).astype(np.uint8))


def check_rate_map_equals_peak(be, geom, T):
    H, W, level = geom
    v = wc.stream(16, H, W)[5:5 + T]
    kw = RM_KW
    for name, frames in dtype_variants(v):
        got = rate_map(be, frames, level, kw["fps"], kw["fmin"], kw["fmax"], kw["F"])
        g = pyr_down_n(be, frames, level)
        want = peak(be, g, kw["fps"], kw["fmin"], kw["fmax"], kw["F"])
        same_outputs(got, want, (geom, T, name))
        assert (got[3] >= 0).any(), (geom, T, name)          # the blob breathes: the comparison is not one of empty maps


# ---- case 4 --------------------------------------------------------------------------------------------------------------------
def check_window(be, T):
    H, W, L, S = wc.SMALL
    v = wc.stream(T, H, W)
    kw = RM_KW
    n_px = int(np.prod(level_shape(H, W, S)))
    with wc.Window(be, T, H, W, L, S) as win:
        outs = Outs(be, n_px)
        assert window_rate_map_rc(be, win, kw["fps"], kw["fmin"], kw["fmax"], kw["F"], outs) == _capi.RM_E_BADARG and outs.untouched()
        for k in range(1, 2 * T + 2):
            win.push_np(v[k - 1:k])
            m = min(k, T)
            outs = Outs(be, n_px)
            rc = window_rate_map_rc(be, win, kw["fps"], kw["fmin"], kw["fmax"], kw["F"], outs)
            if m < 2:
                assert rc == _capi.RM_E_BADARG and outs.untouched()
                continue
            _capi.check(be.lib, rc, "rm_window_rate_map")
            want = rate_map(be, v[k - m:k], S, kw["fps"], kw["fmin"], kw["fmax"], kw["F"])
            same_outputs(outs.np(), want, (T, k))
        # the ROI stage is left alone: the same ROI before the call, after it, and on the contiguous frames
        k = 2 * T + 1
        _, _, roi = wc.contiguous(be, v[k - T:k], L, S)
        before = win.locate()
        outs = Outs(be, n_px)
        _capi.check(be.lib, window_rate_map_rc(be, win, kw["fps"], kw["fmin"], kw["fmax"], kw["F"], outs), "rm_window_rate_map")
        assert win.locate() == before == (_capi.RM_OK, roi)
    with wc.Window(be, T, H, W, L, S, flags=_capi.RM_FLAG_FILTER_LAPLACIANS) as win:
        win.push_np(v[:T])
        outs = Outs(be, n_px)
        assert window_rate_map_rc(be, win, kw["fps"], kw["fmin"], kw["fmax"], kw["F"], outs) == _capi.RM_E_UNSUPPORTED and outs.untouched()


# ---- case 5 --------------------------------------------------------------------------------------------------------------------
PURPOSE = dict(H=70, W=90, T=128, fps=10.0, fmin=0.1, fmax=1.0, F=64, level=1, sigma=5.0, swing=40.0,
               blobs=(((20, 22), 0.5), ((48, 45), 0.65), ((22, 68), 0.8)))      # ((row, column), Hz)


@functools.lru_cache(maxsize=None)
def purpose_clip():
    """uint8 [128, 70, 90]: three soft blobs (Gaussian, cut off at 3 sigma) whose brightness swings at 0.5, 0.65 and 0.8 Hz over a static
    textured background"""
    P = PURPOSE
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:P["H"], 0:P["W"]]
    bg = 110 + 25 * np.sin(yy / 3.1) * np.cos(xx / 4.3) + rng.integers(-12, 13, (P["H"], P["W"]))
    t = np.arange(P["T"])[:, None, None]
    clip = np.broadcast_to(bg[None], (P["T"], P["H"], P["W"])).astype(np.float64).copy()
    for k, ((cy, cx), f) in enumerate(P["blobs"]):
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        g = np.where(d2 <= (3 * P["sigma"]) ** 2, np.exp(-d2 / (2 * P["sigma"] ** 2)), 0.0)
        clip += P["swing"] * g[None] * np.sin(2 * np.pi * f * t / P["fps"] + 0.7 * k)
    clip = np.clip(np.rint(clip), 0, 255).astype(np.uint8)
    clip.setflags(write=False)
    return clip


def purpose_masks():
    """level-1 pixel sets: the interior of each blob (within sigma of its centre), and the background (no pixel of its 5 x 5 pyrDown
    footprint ever changes)"""
    P = PURPOSE
    clip = purpose_clip()
    h, w = level_shape(P["H"], P["W"], 1)
    moving = (clip != clip[0]).any(axis=0)
    bgm = np.zeros((h, w), bool)
    for i in range(h):
        for j in range(w):
            bgm[i, j] = not moving[max(2 * i - 2, 0):2 * i + 3, max(2 * j - 2, 0):2 * j + 3].any()
    yy, xx = np.mgrid[0:h, 0:w]
    inner = [((2 * yy - cy) ** 2 + (2 * xx - cx) ** 2) <= P["sigma"] ** 2 for (cy, cx), _ in P["blobs"]]
    rects = [(cx - 10, cy - 10, 21, 21) for (cy, cx), _ in P["blobs"]]      # full-resolution (x, y, w, h): centre +- 2 sigma
    return inner, bgm, rects


def roi_bpm_host(freq, power, index, shape, level, roi):
    """RateMap.roi_bpm's definition on host arrays"""
    x, y, w, h = roi
    f, p, i = (a.reshape(shape)[y >> level:((y + h - 1) >> level) + 1, x >> level:((x + w - 1) >> level) + 1] for a in (freq, power, index))
    keep = i >= 0
    return None if not keep.any() else float(np.sum(p[keep] * 60 * f[keep]) / np.sum(p[keep]))


def purpose_criteria(freq, power, index, tag):
    """the criteria of the purpose case on [h*w] outputs (the library's, or the reference's own)"""
    P = PURPOSE
    shape = level_shape(P["H"], P["W"], 1)
    inner, bgm, rects = purpose_masks()
    step_bpm = 60 * (P["fmax"] - P["fmin"]) / (P["F"] - 1)
    assert abs(step_bpm - 0.857) < 1e-3
    bpm = 60 * freq.reshape(shape)
    worst = 0.0
    for m, rect, (_, f) in zip(inner, rects, P["blobs"]):
        assert m.sum() >= 9
        err = np.abs(bpm[m] - 60 * f)
        assert np.all(err <= step_bpm), (tag, f, float(err.max()))
        r = roi_bpm_host(freq, power, index, shape, 1, rect)
        assert r is not None and abs(r - 60 * f) <= step_bpm, (tag, f, r)
        worst = max(worst, float(err.max()), abs(r - 60 * f))
    assert bgm.sum() > 200 and np.all(index.reshape(shape)[bgm] == -1), tag
    return worst / step_bpm


def purpose_reference():
    """the reference alone on the clip's level 1 (pyrDown in float64 numpy: cv2's 1-4-6-4-1 / 256 with BORDER_REFLECT_101), so that the
    criteria are known to be the estimator's to meet before the library is asked"""
    P = PURPOSE
    clip = purpose_clip().astype(np.float64)
    k = np.array([1., 4., 6., 4., 1.])

    def down(a):
        pad = np.pad(a, ((0, 0), (2, 2), (2, 2)), mode="reflect")
        hh, ww = a.shape[1], a.shape[2]
        rows = sum(k[i] * pad[:, i:i + hh] for i in range(5))[:, ::2]
        return (sum(k[i] * rows[:, :, i:i + ww] for i in range(5))[:, :, ::2]) / 256.0
    g = down(clip)
    r = Ref(g.reshape(P["T"], -1), P["fps"], P["fmin"], P["fmax"], P["F"])
    return r.freq.astype(np.float64), r.P.max(axis=0).astype(np.float64) * ~r.still, r.index


def check_purpose(be):
    P = PURPOSE
    freq, power, total, index = rate_map(be, purpose_clip(), 1, P["fps"], P["fmin"], P["fmax"], P["F"])
    return purpose_criteria(freq, power, index, "library")


# ---- case 6 --------------------------------------------------------------------------------------------------------------------
def check_argument_errors(be):
    lib = be.lib
    fps, fmin, fmax, F = BAND["fps"], BAND["fmin"], BAND["fmax"], 16
    T, NP = 16, 40
    x = be.dev(np.ascontiguousarray(signals(T, NP, fps, 3)))
    nan = float("nan")
    bad_bands = ((fps, 0.0, fmax), (fps, -0.1, fmax), (fps, fmax, fmax), (fps, fmax, fmin), (fps, fmin, fps / 2 + 1e-9), (0.0, fmin, fmax),
                 (-fps, fmin, fmax), (nan, fmin, fmax), (fps, nan, fmax), (fps, fmin, nan))
    B, U_ = _capi.RM_E_BADARG, _capi.RM_E_UNSUPPORTED

    def refused(rc_fn, code, what):
        outs = Outs(be, 4096)
        assert rc_fn(outs) == code, what
        assert outs.untouched(), what

    # rm_spectral_peak
    for t in (1, 0, -3):
        refused(lambda o: peak_rc(be, x, t, NP, fps, fmin, fmax, F, o), B, ("T", t))
    refused(lambda o: peak_rc(be, x, 4097, NP, fps, fmin, fmax, F, o), U_, "T > 4096")
    for f in (2, 65, 0, -1):
        refused(lambda o: peak_rc(be, x, T, NP, fps, fmin, fmax, f, o), B, ("nfreq", f))
    for b in bad_bands:
        refused(lambda o: peak_rc(be, x, T, NP, b[0], b[1], b[2], F, o), B, b)
    refused(lambda o: peak_rc(be, None, T, NP, fps, fmin, fmax, F, o), B, "NULL input")
    assert lib.rm_spectral_peak(be.ctx, be.p(x), T, NP, fps, fmin, fmax, F, None, None, None, None, be.stream()) == B
    assert lib.rm_spectral_peak(None, be.p(x), T, NP, fps, fmin, fmax, F, None, None, None, None, be.stream()) == B
    refused(lambda o: 0 if peak_rc(be, x, T, 0, fps, fmin, fmax, F, o) == _capi.RM_OK else -99, 0, "NP == 0 is an empty call")
    # rm_spectral_operator
    A = np.full((2 * F, T), np.nan)
    ap = ctypes.c_void_p(A.ctypes.data)
    assert lib.rm_spectral_operator(1, fps, fmin, fmax, F, ap, None) == B
    assert lib.rm_spectral_operator(4097, fps, fmin, fmax, F, None, None) == U_
    for f in (2, 65):
        assert lib.rm_spectral_operator(T, fps, fmin, fmax, f, ap, None) == B
    for b in bad_bands:
        assert lib.rm_spectral_operator(T, b[0], b[1], b[2], F, ap, None) == B, b
    assert np.all(np.isnan(A))
    # rm_rate_map
    H, W = 33, 47
    frames = be.dev(np.ascontiguousarray(wc.stream(16, H, W)[:T]))
    U8 = _capi.RM_U8
    refused(lambda o: rate_map_rc(be, frames, U8, 1, H, W, 1, fps, fmin, fmax, F, o), B, "T < 2")
    refused(lambda o: rate_map_rc(be, frames, U8, 4097, H, W, 1, fps, fmin, fmax, F, o), U_, "T > 4096")
    for lv in (0, -1):
        refused(lambda o: rate_map_rc(be, frames, U8, T, H, W, lv, fps, fmin, fmax, F, o), B, ("level", lv))
    for lv in (8, 9, 30):
        refused(lambda o: rate_map_rc(be, frames, U8, T, H, W, lv, fps, fmin, fmax, F, o), U_, ("level", lv))
    for f in (2, 65):
        refused(lambda o: rate_map_rc(be, frames, U8, T, H, W, 1, fps, fmin, fmax, f, o), B, ("nfreq", f))
    for b in bad_bands:
        refused(lambda o: rate_map_rc(be, frames, U8, T, H, W, 1, b[0], b[1], b[2], F, o), B, b)
    refused(lambda o: rate_map_rc(be, None, U8, T, H, W, 1, fps, fmin, fmax, F, o), B, "NULL input")
    refused(lambda o: rate_map_rc(be, frames, 99, T, H, W, 1, fps, fmin, fmax, F, o), B, "dtype")
    assert lib.rm_rate_map(be.ctx, be.p(frames), U8, T, H, W, 1, fps, fmin, fmax, F, None, None, None, None, be.stream()) == B
    # rm_window_rate_map
    Hs, Ws, L, S = wc.SMALL
    with wc.Window(be, 10, Hs, Ws, L, S) as win:
        win.push_np(wc.stream(10, Hs, Ws)[:1])
        refused(lambda o: window_rate_map_rc(be, win, fps, fmin, fmax, F, o), B, "count < 2")
        win.push_np(wc.stream(10, Hs, Ws)[1:4])
        for f in (2, 65):
            refused(lambda o: window_rate_map_rc(be, win, fps, fmin, fmax, f, o), B, ("nfreq", f))
        for b in bad_bands:
            refused(lambda o: window_rate_map_rc(be, win, b[0], b[1], b[2], F, o), B, b)
        assert lib.rm_window_rate_map(be.ctx, win.h, fps, fmin, fmax, F, None, None, None, None, be.stream()) == B
        assert lib.rm_window_rate_map(be.ctx, None, fps, fmin, fmax, F, None, None, None, None, be.stream()) == B
        outs = Outs(be, int(np.prod(level_shape(Hs, Ws, S))))
        assert window_rate_map_rc(be, win, fps, fmin, fmax, F, outs) == _capi.RM_OK and not outs.untouched()
    for flag in (_capi.RM_FLAG_FILTER_LAPLACIANS, _capi.RM_FLAG_UNFUSED_SMALL):
        with wc.Window(be, 10, Hs, Ws, L, S, flags=flag) as win:
            win.push_np(wc.stream(10, Hs, Ws)[:4])
            refused(lambda o: window_rate_map_rc(be, win, fps, fmin, fmax, F, o), U_, ("window flag", flag))
