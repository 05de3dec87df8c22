"""TEST INFRASTRUCTURE: high-precision references for the motion-extraction path (reference base.py:354-407) and the edge-case
inputs the motion tests sweep (tests/test_emu_motion_edges.py, tests/test_gpu_motion_edges.py).

- roi_mean_exact / roi_mean_bound: np.average(crop) (base.py:357) summed exactly, and a rigorous bound on the rounding error of
  k_roi_mean's summation order.
- pca_exact: base.py:396-405 in exact arithmetic (Fraction covariance, 50-digit eigenpairs).
- the sweep drivers: corners and Lucas-Kanade on every small crop against the oracle, through any backend that offers the
  adapter methods named in `sweep_corners` / `sweep_lk` (the host emulation or the GPU)."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                                         # unit roundoff of float64


# ------------------------------------------------------------------------------------------------------------------------------
# ROI mean (base.py:357, k_roi_mean)
# ------------------------------------------------------------------------------------------------------------------------------
def roi_values(frame, x, y, w, h):
    """The crop's pixels as float64, converted the way the product converts them: k * (1/255) for uint8 (load_px), float16 and
    float32 widened exactly."""
    c = np.asarray(frame)[y:y + h, x:x + w]
    if c.dtype == np.uint8:
        return c.astype(np.float64) * (1. / 255)
    return c.astype(np.float64)


def roi_mean_exact(frame, x, y, w, h):
    """The exact mean of the converted crop as a Fraction.  math.fsum is correctly rounded; the residual sum it leaves is added
    back (a second fsum), so the result is exact to within u^2 of the sum -- far below any tolerance used with it."""
    v = roi_values(frame, x, y, w, h).ravel().tolist()
    s = math.fsum(v)
    v.append(-s)
    r = math.fsum(v)
    return (Fraction(s) + Fraction(r)) / len(v[:-1])


def roi_mean_bound(n, sum_abs):
    """Rigorous bound on |k_roi_mean - exact mean| for n pixels whose converted magnitudes sum to sum_abs: every lane adds
    ceil(n/256) terms in sequence, then a 6-level xor tree, 3 adds of the four wave partials and the division, so every term
    passes through at most ceil(n/256) + 8 roundings: gamma_k * sum|v| / n, gamma_k = k u / (1 - k u)."""
    k = -(-n // 256) + 8
    gamma = Fraction(k) * Fraction(U) / (1 - Fraction(k) * Fraction(U))
    return gamma * Fraction(sum_abs) / n


# ------------------------------------------------------------------------------------------------------------------------------
# PCA (base.py:396-405, k_pca_reduce)
# ------------------------------------------------------------------------------------------------------------------------------
def exact_cov(motion_f32):
    """np.cov(ddof=1) of the float32 rows, exactly: (cxx, cxy, cyy) as Fractions."""
    m = np.asarray(motion_f32, dtype=np.float32).reshape(-1, 2)
    n = len(m)
    xs = [Fraction(float(v)) for v in m[:, 0]]
    ys = [Fraction(float(v)) for v in m[:, 1]]
    mx, my = sum(xs) / n, sum(ys) / n
    cxx = sum((a - mx) ** 2 for a in xs) / (n - 1)
    cxy = sum((a - mx) * (b - my) for a, b in zip(xs, ys)) / (n - 1)
    cyy = sum((b - my) ** 2 for b in ys) / (n - 1)
    return cxx, cxy, cyy


def pca_exact(motion_f32, oracle=None):
    """base.py:396-405 in exact arithmetic -> (value, g, (cxx, cxy, cyy)).

    The eigenpairs of the exact covariance are taken at 50 digits and ordered by the reference's rule: argsort(vals)[::-1], then
    the FIRST ROW of eig_vecs[:, idx] -- the x-components of the major and the minor unit eigenvectors -- is dotted with the last
    row.  g = (l1 - l2) / l1 is the relative eigen-gap (0 for a zero covariance).  Eigenvectors are defined up to sign, and the
    reference's value depends on both signs: with `oracle` given and g not tiny, the signs are those of the candidate nearest
    oracle.pca_first_component (numpy's dgeev); otherwise both components are taken non-negative.
    Equal eigenvalues (g == 0, covariance c*I) have no eigenvector basis to speak of: there the value is the one dgeev's rule gives
    on c*I (the identity; the reversed stable argsort picks column 1, so evec1 = (0, 1)): exactly y_last."""
    import mpmath
    m = np.asarray(motion_f32, dtype=np.float32).reshape(-1, 2)
    cxx, cxy, cyy = cov = exact_cov(m)
    xl, yl = float(m[-1, 0]), float(m[-1, 1])
    with mpmath.workdps(50):
        a, b, c = (mpmath.mpf(t.numerator) / t.denominator for t in cov)
        half, mid = (a - c) / 2, (a + c) / 2
        rad = mpmath.sqrt(half * half + b * b)
        l1, l2 = mid + rad, mid - rad
        if rad == 0:
            return yl, 0.0, cov
        g = float((l1 - l2) / l1)
        # major unit eigenvector: the better conditioned of (l1 - c, b) and (b, l1 - a)
        p, q = (l1 - c, b) if abs(l1 - c) >= abs(l1 - a) else (b, l1 - a)
        nrm = mpmath.sqrt(p * p + q * q)
        v1 = (p / nrm, q / nrm)
        v2 = (-v1[1], v1[0])                                   # minor eigenvector (orthogonal)
        e0, e1 = abs(v1[0]), abs(v2[0])                         # first row: x-components of major, minor
        cands = [xl * s0 * e0 + yl * s1 * e1 for s0 in (1, -1) for s1 in (1, -1)]
        val = cands[0]
        if oracle is not None and g > 1e-6:
            ref = oracle.pca_first_component([list(r) for r in m])
            val = min(cands, key=lambda z: abs(z - ref))
        return val, g, cov


def pca_bound(motion_f32, g):
    """Tolerance for a well-conditioned case (g >= 1e-6): 64 u (|x_last| + |y_last|) (1 + 1/g)."""
    m = np.asarray(motion_f32, dtype=np.float32).reshape(-1, 2)
    return 64 * U * (abs(float(m[-1, 0])) + abs(float(m[-1, 1]))) * (1 + 1 / g)


def pca_families(rng):
    """(name, float32 [n,2]) cases: generic rows, collinear rows, identical rows, isotropic dyadic sets, magnitudes 1e-20 ... 1e20,
    n = 2 and n = 128 (the motion_data deque's cap, base.py:136)."""
    out = []
    for n in (2, 3, 17, 128):
        for k in range(6):
            ang = rng.uniform(0, np.pi)
            rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
            base = rng.standard_normal((n, 2)) * [rng.uniform(0.3, 3.0), rng.uniform(0.01, 1.0)]
            out.append(("generic n=%d #%d" % (n, k), (base @ rot.T + rng.uniform(-1, 1, 2)).astype(np.float32)))
    for n in (2, 128):
        for a in (1.0, -1.0, 2.0, 1e-3):
            x = (rng.standard_normal(n) + rng.uniform(-0.5, 0.5)).astype(np.float32)
            out.append(("collinear a=%g n=%d" % (a, n), np.stack([x, (np.float32(a) * x).astype(np.float32)], 1)))
    for n in (2, 128):
        out.append(("identical n=%d" % n, np.tile(np.array([[0.3, -1.7]], np.float32), (n, 1))))
    for n, d, o in ((4, 0.25, 0.0), (128, 2.0 ** -10, 0.5), (8, 3.0, -1.25)):
        pat = np.array([[o + d, o], [o - d, o], [o, o + d], [o, o - d]], np.float64)
        out.append(("isotropic n=%d d=%g" % (n, d), np.tile(pat, (n // 4, 1)).astype(np.float32)))
    for e in (-20, -10, -3, 3, 10, 20):
        for n in (2, 128):
            base = rng.standard_normal((n, 2)) * [1.0, 0.3] + rng.uniform(-0.5, 0.5, 2)
            out.append(("scale 1e%d n=%d" % (e, n), (base * 10.0 ** e).astype(np.float32)))
    return out


def check_pca(got, m, oracle):
    """Assert the product's value against pca_exact; returns |got - exact| / bound (0 for the equal-eigenvalue rule)."""
    val, g, cov = pca_exact(m, oracle)
    if g == 0.0:
        assert got == float(m[-1, 1]), (got, float(m[-1, 1]))
        return 0.0
    assert g >= 1e-6, g                                        # (the families hold no nearly-degenerate, non-degenerate case)
    err = abs(got - float(val))
    bound = pca_bound(m, g)
    assert err <= bound, (got, float(val), g, bound)
    return err / bound


# ------------------------------------------------------------------------------------------------------------------------------
# corner and LK sweeps on small crops
# ------------------------------------------------------------------------------------------------------------------------------
SMALL = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 23)
WINS = ((3, 3), (9, 9), (15, 15), (7, 21), (31, 31), (32, 32))
LEVELS = (0, 1, 2, 3, 4, 9)                                   # 9: clamped by lk_max_level on every crop here
FEATURE = dict(maxCorners=100, qualityLevel=0.3, minDistance=7)


def crop_pair(texture, h, w, shift=(0.6, -0.4)):
    """Textured (prev, next) crops of h x w from the top-left of a 64 x 64 synthetic texture, and a flat crop."""
    a, b = texture(0.0, 0.0)[:h, :w].copy(), texture(*shift)[:h, :w].copy()
    return a, b, np.full((h, w), 117, np.uint8)


def probe_points(h, w):
    """Points inside the crop, on its border, and 0.5 px and 5 px outside it."""
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    p = [(cx, cy), (0.0, 0.0), (w - 1.0, h - 1.0), (0.0, cy), (cx, h - 1.0), (-0.5, cy), (cx, h - 0.5), (w + 4.0, cy),
         (cx, -5.0), (w - 1.25, 0.75)]
    return np.array(p, np.float32).reshape(-1, 1, 2)


def reference_crop(oracle, frame_u8):
    """What extract_motion tracks for a uint8 frame (base.py:364): float_to_uint8(uint8_to_float(frame)) -- not the identity on
    every uint8 value."""
    return oracle.float_to_uint8(oracle.uint8_to_float(frame_u8))


def sweep_corners(be, oracle, texture):
    """Every small crop, textured and flat, blockSize 3, 5 and 7 (7 is the reference's; on crops 3 to 6 pixels wide its reflect-101
    border wraps more than once): be.gftt(img, blockSize) and be.begin(img, blockSize) (the resident
    path, whole frame = the crop, so its image is reference_crop(img)) must return None exactly when the oracle does, and the same
    corners otherwise."""
    ncases = 0
    for h in SMALL:
        for w in SMALL:
            a, _, flat = crop_pair(texture, h, w)
            for img in (a, flat):
                for bs in (3, 5, 7):
                    for got, src in ((be.gftt(img, bs), img), (be.begin(img, bs), reference_crop(oracle, img))):
                        ref = oracle.goodFeaturesToTrack(src, FEATURE["maxCorners"], FEATURE["qualityLevel"], FEATURE["minDistance"],
                                                         blockSize=bs)
                        assert (got is None) == (ref is None), (h, w, bs)
                        assert ref is None or np.array_equal(got, ref), (h, w, bs)
                        ncases += 1
    return ncases


def lk_expect_unsupported(h, w, win, level):
    """What the product must refuse with RM_E_UNSUPPORTED (rm_flow.h LK_MAX_WIN / LK_MAX_LEVELS)."""
    if win[0] * win[1] > 1024:
        return True
    sh, sw, lv = h, w, level
    for l in range(level + 1):
        sw, sh = (sw + 1) // 2, (sh + 1) // 2
        if sw <= win[0] or sh <= win[1]:
            lv = l
            break
    return lv + 1 > 8


def sweep_lk(be, oracle, texture, crops=SMALL, wins=WINS, levels=LEVELS):
    """Pyramidal LK on every small crop: the four-call path on probe points (status bit-exact, p1[st == 1] bit-exact), and
    the resident path (begin on the crop's own corners -- qualityLevel 0.01, minDistance 1 so that small crops have some --
    then one step) against the oracle's LK of those corners: n_good, mean flow and surviving points bit-exact."""
    import pytest
    from respmon_amd import _capi
    ncases = 0
    for h in crops:
        for w in crops:
            a, b, _ = crop_pair(texture, h, w)
            pts = probe_points(h, w)
            ra, rb = reference_crop(oracle, a), reference_crop(oracle, b)
            corners = oracle.goodFeaturesToTrack(ra, 50, 0.01, 1, blockSize=3)
            for win in wins:
                for lvl in levels:
                    crit = (3, 10, 0.03)
                    if lk_expect_unsupported(h, w, win, lvl):
                        with pytest.raises(_capi.RespmonError, match=r"\(%d\)" % _capi.RM_E_UNSUPPORTED):
                            be.lk(a, b, pts, win, lvl, crit)
                        if corners is not None:                 # (a step without points tracks nothing and refuses nothing)
                            be.begin_pts(a, 50, 0.01, 1, 3)
                            with pytest.raises(_capi.RespmonError, match=r"\(%d\)" % _capi.RM_E_UNSUPPORTED):
                                be.step(b, win, lvl, crit)
                        ncases += 1
                        continue
                    p1, st = be.lk(a, b, pts, win, lvl, crit)
                    r1, rs, _ = oracle.calcOpticalFlowPyrLK(a, b, pts, None, winSize=win, maxLevel=lvl, criteria=crit)
                    assert np.array_equal(st, rs), (h, w, win, lvl)
                    ok = rs.ravel() == 1
                    assert np.array_equal(p1.reshape(-1, 2)[ok], r1.reshape(-1, 2)[ok]), (h, w, win, lvl)
                    ncases += 1
                    if corners is None:
                        continue
                    got0 = be.begin_pts(a, 50, 0.01, 1, 3)
                    assert np.array_equal(got0, corners), (h, w)
                    mean, ng, left = be.step(b, win, lvl, crit)
                    r1, rs, _ = oracle.calcOpticalFlowPyrLK(ra, rb, corners, None, winSize=win, maxLevel=lvl, criteria=crit)
                    good = rs.ravel() == 1
                    assert ng == int(good.sum()), (h, w, win, lvl)
                    if ng:
                        want = np.mean(corners.reshape(-1, 2)[good] - r1.reshape(-1, 2)[good], axis=0)
                        assert np.array_equal(mean, want), (h, w, win, lvl)
                    assert np.array_equal(left.reshape(-1, 2), r1.reshape(-1, 2)[good]), (h, w, win, lvl)
                    ncases += 1
    return ncases
