"""TEST INFRASTRUCTURE (not a test module): what a Lucas-Kanade tracker converges to, in real arithmetic, and how far a correct
fixed-point tracker may stay from it.  Shares nothing with oracle/cvref_flow.c or respmon_amd/csrc/rm_flow.h beyond the definition of
the problem: no weight bits, no descale, no float32 sums, no iteration rules.  Integers are numpy int64, reals numpy longdouble.

Images (exact integers)
    pyr_down(u8)   [1 4 6 4 1] x [1 4 6 4 1] sum, BORDER_REFLECT_101, (s + 128) >> 8, output size (n + 1) // 2
    scharr(u8)     gx = [-1 0 1] along x (x) [3 10 3] along y, gy the transpose, the image reflected (101) for the taps
both through scipy.ndimage.correlate1d(mode="mirror") on int64; lengths below 3 are extended by hand (index reflection).

The level-0 functional (class Functional)
    For a point p and a candidate q the window is win_w x win_h taps at p - ((win_w - 1) / 2, (win_h - 1) / 2) + (i, j).
    Samples are exactly bilinear; outside the image the IMAGE is reflected (101), the DERIVATIVE is zero.
        I~_k = I(p + tap_k)   g~_k = (gx, gy)(p + tap_k) in raw Scharr units   J~_k(q) = J(q + tap_k)   d_k(q) = J~_k(q) - I~_k
        G = sum g~ g~^T       b(q) = sum d_k(q) g~_k
    A raw Scharr unit is 1/32 grey level per pixel ([3 10 3] sums to 16, [-1 0 1] spans two pixels), so the Gauss-Newton step in
    pixels is
        delta(q) = -32 G^-1 b(q)
    fixed_point(p, q0) iterates q <- q + delta(q) in longdouble until |delta| < 1e-9 px and says where that failed.
    min_eig(p) = lambda_min(G) * 2^-20 / (win_w * win_h): the documented status quantity "minimum eigenvalue of the 2 x 2 normal matrix
    of the optical flow equations, divided by the number of pixels in the window".  The scaling, from the definition: the tracker forms
    its normal equations from samples kept as 32 x grey level and derivatives kept as 32 x gradient, and brings both sides back by one
    common factor 2^-20 = 32^-4 (the right-hand side carries 32 * 32 from its two factors and the step is a ratio, so any common factor
    would do for the step; for the eigenvalue it is this one).  G in raw units is 32^2 sum grad grad^T, so G * 2^-20 = sum grad grad^T / 32^2:
    min_eig is the smaller eigenvalue of the window mean of the gradient tensor of the image I / 32.  The status rule compares it with 1e-4.

The tolerance tol(p, q*, criteria)  --  derived, not observed
    A fixed-point tracker evaluates F~(q) = delta(q) + e(q).  Near q*, delta(q) = (M - I)(q - q*) with M = I + d delta / dq, which
    the reference measures by central differences of delta at q* +- 2^-10 px; rho = ||M||_2 is the local contraction factor.
    With E >= |e|, iterates obey err_{j+1} = M err_j + e, so
      (1) resting error                       <= E / (1 - rho)
      (2) stop by |step| <= eps:  step_j = (M - I) err_j + e, err_{j+1} = err_j + step_j     =>  extra rho * eps / (1 - rho)
      (3) stop by OpenCV's oscillation rule (two successive steps sum to < 0.01 on each axis, the midpoint is returned):
          s + t = err_{j+1} - err_{j-1} = (M^2 - I) err_{j-1} + ..., |s + t| <= c = 0.01 sqrt 2         =>  extra rho * c / (1 - rho^2)
      (4) stop by count: rho^count * R, R = 2 px being the distance at which a pyramid tracker enters level 0 at the latest if level 1
          was resolved to one of its own pixels (an assumption, stated; with count >= 10 it matters only where rho > 0.5).
    One of (2) - (4) ends the iteration, so the slack is their maximum.
    E = 32 ||G^-1||_2 * (sum_k (eps_d,k |g~_k| + |d_k| eta_k + eps_d,k eta_k)  +  gamma_{n+1} sum_k |d_k| |g~_k|), term by term:
      - image samples are kept to 1/32 grey level, rounded: 1/64 each for I~ and J~ (I~ exact when p - half is a whole pixel);
      - bilinear weights are kept to 2^-14: each of three is off by at most e_w = (1/2 + 3 * 2^-10) * 2^-14 (rounding, and three float32
        roundings of a product below 2^14), the fourth takes the remainder, so sum |dw| <= 6 e_w while sum dw = 0: a sample moves by at
        most 3 e_w * (max - min of its four neighbours).  eps_d,k = 1/64 + 1/64 + 3 e_w (spread_I,k + spread_J,k);
      - derivative samples are kept to one raw unit, rounded: 1/2 + 3 e_w * spread per component (0 on whole pixels), eta_k the norm
        of the two components;
      - the two sums of b run in float32 over n = win_w * win_h integer products that may exceed 2^24: gamma_{n+1} = (n+1)u / (1 - (n+1)u),
        u = 2^-24, in any order of summation.
      The quantised G changes M, not the place where b vanishes; the float32 evaluation of the 2 x 2 solve is relative to the step and
      vanishes with it.
    Coordinates are float32: p - half is rounded once (moves the template, hence q*, by as much), and the last iterate is rounded
    three times on the way out (+= step, + half, - step / 2): 2 ulp per axis at the largest coordinate involved.
    Second order (M is not constant over the neighbourhood: J~ is piecewise bilinear; spreads taken at q*, not at the iterate):
    the safety factor 2 on (1) - (4), no more.

    tol = 2 * (E / (1 - rho) + slack) + 2 sqrt 2 ulp32

The status band  min_eig_band(p)
    lambda_min moves by at most ||dG||_2 (Weyl) <= sum_k (2 |g~_k| eta_k + eta_k^2) + (2 gamma_{n+1} + 8u) trace G  (three float32 sums,
    Frobenius <= 2 max entry; the eigenvalue formula is eight float32 operations on values <= trace), times 2^-20 / n.
    det >= FLT_EPSILON is implied by min_eig >= 1e-4 for every window of 4 taps or more ((n * 1e-4)^2 > 2^-23), so it needs no band."""
import numpy as np
import scipy.ndimage as ndi

LD = np.longdouble
U32 = LD(2) ** -24
E_W = (LD(0.5) + 3 * LD(2) ** -10) * LD(2) ** -14
C_OSC = LD(0.01) * np.sqrt(LD(2))
R_ENTRY = LD(2)
STEP_DONE = LD(1e-9)
MIN_EIG_THRESHOLD = LD(1e-4)
COND_MAX = 1e3            # (a) leaves out points whose G has a larger condition number: the linearisation the bound rests on needs both directions pinned
FD_H = LD(2) ** -10


def reflect101(i, n):
    """index reflection gfedcb|abcdefgh|gfedcba for any distance"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    m = np.mod(i, 2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def _corr(a, k, axis):
    """correlate1d with the mirror border; axes shorter than the kernel's reach are extended by index reflection first"""
    r = len(k) // 2
    n = a.shape[axis]
    if n > r:
        return ndi.correlate1d(a, k, axis=axis, mode="mirror", output=np.int64)
    ext = np.take(a, reflect101(np.arange(-r, n + r), n), axis=axis)
    out = ndi.correlate1d(ext, k, axis=axis, mode="constant", output=np.int64)
    return np.take(out, np.arange(r, r + n), axis=axis)


def pyr_down(img):
    a = np.asarray(img).astype(np.int64)
    k = [1, 4, 6, 4, 1]
    s = _corr(_corr(a, k, 0), k, 1)[::2, ::2]
    return ((s + 128) >> 8).astype(np.uint8)


def scharr(img):
    """-> (gx, gy) int64"""
    a = np.asarray(img).astype(np.int64)
    return _corr(_corr(a, [3, 10, 3], 0), [-1, 0, 1], 1), _corr(_corr(a, [3, 10, 3], 1), [-1, 0, 1], 0)


def pyramid(img, levels):
    out = [np.asarray(img, dtype=np.uint8)]
    for _ in range(levels):
        out.append(pyr_down(out[-1]))
    return out


def ulp32(v):
    v = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 1.0).astype(np.float32)
    return LD(1) * (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


class Template:
    pass


class Functional:
    def __init__(self, prev, nxt, win):
        self.I = np.asarray(prev).astype(np.int64)
        self.J = np.asarray(nxt).astype(np.int64)
        assert self.I.shape == self.J.shape and self.I.ndim == 2
        self.H, self.W = self.I.shape
        self.gx, self.gy = scharr(prev)
        self.ww, self.wh = int(win[0]), int(win[1])
        self.n = self.ww * self.wh
        j, i = np.divmod(np.arange(self.n), self.ww)
        self.ti, self.tj = i.astype(np.int64)[None, :], j.astype(np.int64)[None, :]
        self.half = np.array([LD(self.ww - 1) / 2, LD(self.wh - 1) / 2], dtype=LD)

    # -- sampling ---------------------------------------------------------------------------------------------------------------
    def origin(self, P):
        """whole-pixel window origin [N,2] int64 and the fractions [N,2]"""
        X = np.asarray(P, dtype=LD).reshape(-1, 2) - self.half
        o = np.floor(X)
        return o.astype(np.int64), X - o

    def in_range(self, P):
        """the window origin lies in [-win, size) on both axes"""
        o, _ = self.origin(P)
        return (o[:, 0] >= -self.ww) & (o[:, 0] < self.W) & (o[:, 1] >= -self.wh) & (o[:, 1] < self.H)

    def _gather(self, arr, iy, ix, zero_pad):
        if zero_pad:
            ok = (iy >= 0) & (iy < self.H) & (ix >= 0) & (ix < self.W)
            return np.where(ok, arr[np.clip(iy, 0, self.H - 1), np.clip(ix, 0, self.W - 1)], 0)
        return arr[reflect101(iy, self.H), reflect101(ix, self.W)]

    def _bilinear(self, arr, P, zero_pad):
        """-> (samples [N,n] longdouble, max - min of each sample's four neighbours [N,n])"""
        o, f = self.origin(P)
        ix, iy = o[:, 0:1] + self.ti, o[:, 1:2] + self.tj
        a, b = f[:, 0:1], f[:, 1:2]
        v = [self._gather(arr, iy + dy, ix + dx, zero_pad) for dy in (0, 1) for dx in (0, 1)]
        val = (1 - a) * (1 - b) * v[0] + a * (1 - b) * v[1] + (1 - a) * b * v[2] + a * b * v[3]
        st = np.stack(v)
        return val, (st.max(axis=0) - st.min(axis=0)).astype(LD)

    # -- the functional ---------------------------------------------------------------------------------------------------------
    def template(self, P):
        """what depends on p alone; every method below takes either the points p [N,2] or their template"""
        if isinstance(P, Template):
            return P
        T = Template()
        T.P = np.asarray(P, dtype=LD).reshape(-1, 2)
        T.I, T.spread_I = self._bilinear(self.I, T.P, False)
        T.gx, T.spread_gx = self._bilinear(self.gx, T.P, True)
        T.gy, T.spread_gy = self._bilinear(self.gy, T.P, True)
        _, f = self.origin(T.P)
        T.whole = (f[:, 0] == 0) & (f[:, 1] == 0)
        T.g11, T.g12, T.g22 = (T.gx * T.gx).sum(1), (T.gx * T.gy).sum(1), (T.gy * T.gy).sum(1)
        T.det = T.g11 * T.g22 - T.g12 * T.g12
        root = np.sqrt((T.g11 - T.g22) ** 2 + 4 * T.g12 * T.g12)
        T.lmin, T.lmax = (T.g11 + T.g22 - root) / 2, (T.g11 + T.g22 + root) / 2
        T.in_range = self.in_range(T.P)
        return T

    def residual(self, T, Q, rows=None):
        rows = slice(None) if rows is None else rows
        Jq, spread_J = self._bilinear(self.J, Q, False)
        return Jq - T.I[rows], spread_J

    def delta(self, T, Q, rows=None):
        """the Gauss-Newton step at Q [N,2] (NaN where G is singular)"""
        rows = slice(None) if rows is None else rows
        d, _ = self.residual(T, Q, rows)
        b1, b2 = (d * T.gx[rows]).sum(1), (d * T.gy[rows]).sum(1)
        det = T.det[rows]
        with np.errstate(divide="ignore", invalid="ignore"):
            dx = -32 * (T.g22[rows] * b1 - T.g12[rows] * b2) / det
            dy = -32 * (T.g11[rows] * b2 - T.g12[rows] * b1) / det
        out = np.stack([dx, dy], axis=1)
        out[det <= 0] = np.nan
        return out

    def fixed_point(self, T, Q0, max_iter=300):
        """-> (q* [N,2], converged [N] bool).  Not converged: G singular, the iterate left the range, or max_iter steps did not do."""
        T = self.template(T)
        Q = np.array(Q0, dtype=LD).reshape(-1, 2)
        done = np.zeros(len(Q), bool)
        alive = (T.det > 0) & T.in_range
        for _ in range(max_iter):
            rows = np.flatnonzero(alive & ~done)
            if len(rows) == 0:
                break
            ok = self.in_range(Q[rows])
            alive[rows[~ok]] = False
            rows = rows[ok]
            if len(rows) == 0:
                break
            step = self.delta(T, Q[rows], rows)
            Q[rows] += step
            done[rows] = np.hypot(step[:, 0], step[:, 1]) < STEP_DONE
        return Q, done & alive

    def min_eig(self, T):
        T = self.template(T)
        return T.lmin * LD(2) ** -20 / self.n

    def min_eig_band(self, T):
        T = self.template(T)
        eta = self._eta(T)
        gnorm = np.hypot(T.gx, T.gy)
        gam = (self.n + 1) * U32 / (1 - (self.n + 1) * U32)
        dG = (2 * gnorm * eta + eta * eta).sum(1) + (2 * gam + 8 * U32) * (T.g11 + T.g22)
        return dG * LD(2) ** -20 / self.n

    def cond(self, T):
        T = self.template(T)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(T.lmin > 0, T.lmax / T.lmin, np.inf).astype(np.float64)

    def pre_status(self, T):
        """what the status rule says before the first iteration: 1, 0, or -1 inside the band of the eigenvalue test"""
        T = self.template(T)
        me, band = self.min_eig(T), self.min_eig_band(T)
        st = np.where(me >= MIN_EIG_THRESHOLD, 1, 0)
        st[np.abs(me - MIN_EIG_THRESHOLD) <= band] = -1
        st[~T.in_range] = 0
        return st

    def _eta(self, T):
        ex = np.where(T.whole[:, None], 0, LD(0.5) + 3 * E_W * T.spread_gx)
        ey = np.where(T.whole[:, None], 0, LD(0.5) + 3 * E_W * T.spread_gy)
        return np.hypot(ex, ey)

    def contraction(self, T, Q):
        """rho = ||I + d delta / dq||_2 at Q, by central differences"""
        cols = []
        for e in (np.array([FD_H, 0], dtype=LD), np.array([0, FD_H], dtype=LD)):
            cols.append((self.delta(T, Q + e) - self.delta(T, Q - e)) / (2 * FD_H))
        M = np.stack(cols, axis=2).astype(np.float64) + np.eye(2)      # M[:, :, c] = column c
        rho = np.full(len(Q), np.inf)
        ok = np.isfinite(M).all(axis=(1, 2))
        rho[ok] = np.linalg.norm(M[ok], ord=2, axis=(1, 2))
        return rho.astype(LD)

    def tol(self, T, Qs, criteria):
        """-> (tol [N], parts dict).  criteria = (type, count, eps) as given to the tracker (count is clamped to [0, 100], eps to [0, 10])."""
        T = self.template(T)
        _, count, eps = criteria
        count, eps = min(max(int(count), 0), 100), min(max(LD(eps), LD(0)), LD(10))
        d, spread_J = self.residual(T, Qs)
        eps_I = np.where(T.whole[:, None], 0, LD(1) / 64 + 3 * E_W * T.spread_I)
        eps_d = eps_I + LD(1) / 64 + 3 * E_W * spread_J
        eta = self._eta(T)
        gnorm = np.hypot(T.gx, T.gy)
        gam = (self.n + 1) * U32 / (1 - (self.n + 1) * U32)
        db = (eps_d * gnorm + np.abs(d) * eta + eps_d * eta).sum(1) + gam * (np.abs(d) * gnorm).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            E = np.where(T.lmin > 0, 32 * db / T.lmin, np.inf)
            rho = self.contraction(T, Qs)
            rest = np.where(rho < 1, E / (1 - rho), np.inf)
            slack = np.where(rho < 1, np.maximum(np.maximum(rho * eps / (1 - rho), rho * C_OSC / (1 - rho * rho)), rho ** count * R_ENTRY), np.inf)
        coord = 2 * np.sqrt(LD(2)) * ulp32(np.maximum(np.abs(T.P).max(1), np.abs(Qs).max(1)) + max(self.ww, self.wh))
        return 2 * (rest + slack) + coord, dict(E=E, rho=rho, rest=rest, slack=slack, coord=coord)
