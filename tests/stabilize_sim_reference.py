"""TEST INFRASTRUCTURE: a numpy restatement of the rule of rm_stab_sim_* and rm_warp_similarity (include/respmon_hip.h), operation by
operation, in float64.  The gray value, the pyramid, the conversions, the sums' orders and the level step of the shift model are those
of tests/stabilize_reference.py; the similarity levels, the L D L^T factorisation, the substitutions and the warp are written out here.

`order` selects the order of the sums as there: 'fsum', 'seq', 'rev', 'pairwise'.  The spread of the four frame corners' positions under
the reported parameters across the four is what the tolerance of the tests is made of (tests/stabilize_sim_cases.py)."""
import math

import numpy as np

from tests import stabilize_reference as sr

FLAG_LEVEL_SKIPPED, FLAG_CLAMPED, FLAG_LINEAR_CLAMPED = 1, 2, 4
ORDERS = sr.ORDERS
PAIRS = [(i, j) for i in range(4) for j in range(i + 1)]


def bilinear_at(F, fx, fy):
    """bilinear(F, fx, fy) of the rule at gathered positions (arrays of one shape)"""
    h, w = F.shape
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = fx - x0, fy - y0
    i0, i1 = np.clip(x0, 0, w - 1).astype(np.int64), np.clip(x0 + 1, 0, w - 1).astype(np.int64)
    j0, j1 = np.clip(y0, 0, h - 1).astype(np.int64), np.clip(y0 + 1, 0, h - 1).astype(np.int64)
    return ((1 - ax) * F[j0, i0] + ax * F[j0, i1]) * (1 - ay) + ((1 - ax) * F[j1, i0] + ax * F[j1, i1]) * ay


def positions(p, cx, cy, xs, ys, sx, sy):
    """(fx, fy) [len(ys), len(xs)]: fx = (cx + (m u - p1 v)) + sx, fy = (cy + (p1 u + m v)) + sy"""
    u, v = (np.asarray(xs, dtype=np.float64) - cx)[None, :], (np.asarray(ys, dtype=np.float64) - cy)[:, None]
    m, p1 = np.float64(1.0) + np.float64(p[0]), np.float64(p[1])
    return (cx + (m * u - p1 * v)) + sx, (cy + (p1 * u + m * v)) + sy


def ldlt(Hm):
    """(L, D, valid) of the rule: row by row, no square root, every inner sum left to right"""
    L, D = np.zeros((4, 4)), np.zeros(4)
    with np.errstate(all="ignore"):
        for j in range(4):
            acc = None
            for k in range(j):
                t = (L[j, k] * L[j, k]) * D[k]
                acc = t if acc is None else acc + t
            D[j] = Hm[j, j] if acc is None else Hm[j, j] - acc
            for i in range(j + 1, 4):
                acc = None
                for k in range(j):
                    t = (L[i, k] * L[j, k]) * D[k]
                    acc = t if acc is None else acc + t
                L[i, j] = (Hm[i, j] if acc is None else Hm[i, j] - acc) / D[j]
    return L, D, bool(np.all(np.isfinite(D)) and np.all(D > 0))


def solve(L, D, g):
    z0 = g[0]
    z1 = g[1] - L[1, 0] * z0
    z2 = g[2] - (L[2, 0] * z0 + L[2, 1] * z1)
    z3 = g[3] - ((L[3, 0] * z0 + L[3, 1] * z1) + L[3, 2] * z2)
    y0, y1, y2, y3 = z0 / D[0], z1 / D[1], z2 / D[2], z3 / D[3]
    x3 = y3
    x2 = y2 - L[3, 2] * x3
    x1 = y1 - (L[2, 1] * x2 + L[3, 1] * x3)
    x0 = y0 - ((L[1, 0] * x1 + L[2, 0] * x2) + L[3, 0] * x3)
    return x0, x1, x2, x3


class Reference:
    """The session's state for one reference frame, and the estimate of any frame against it."""

    def __init__(self, frame, level_coarse=3, level_fine=0, level_linear=1, iterations=2, max_shift=8.0, max_linear=0.03, order="fsum"):
        self.lc, self.lf, self.ll, self.iterations, self.order = level_coarse, level_fine, level_linear, iterations, order
        self.max_shift, self.max_linear = float(max_shift), float(max_linear)
        f = sr.gray(frame)
        H, W = f.shape
        self.cx, self.cy = (W - 1) * 0.5, (H - 1) * 0.5
        self.R = sr.pyramid(f, level_coarse)
        # the levels above level_linear: the shift model itself, with level_fine there
        top = max(level_fine, level_linear + 1)
        self.shift = sr.Reference(frame, level_coarse, top, iterations, max_shift, order) if top <= level_coarse else None
        self.lv = {}
        for l in range(min(level_linear, level_coarse), level_fine - 1, -1):
            R = self.R[l]
            h, w = R.shape
            inv = 1.0 / 2 ** l
            b = int(math.ceil((self.max_shift + self.max_linear * (self.cx + self.cy)) * inv)) + 2
            if w - 2 * b < 1 or h - 2 * b < 1:
                self.lv[l] = None
                continue
            Rx = (0.5 * (R[:, 2:] - R[:, :-2]))[b:h - b, b - 1:w - b - 1]
            Ry = (0.5 * (R[2:, :] - R[:-2, :]))[b - 1:h - b - 1, b:w - b]
            xs, ys = np.arange(b, w - b, dtype=np.float64), np.arange(b, h - b, dtype=np.float64)
            u, v = (xs - self.cx * inv)[None, :], (ys - self.cy * inv)[:, None]
            J = [Rx * u + Ry * v, Ry * u - Rx * v, Rx, Ry]
            Hm = np.zeros((4, 4))
            for i, j in PAIRS:
                Hm[i, j] = sr._sum(J[i] * J[j], order)
            self.lv[l] = (b, J, xs, ys) + ldlt(Hm)

    def estimate(self, frame):
        """(p [4], flags) of one frame"""
        flags = 0
        d = np.zeros(2)
        if self.shift is not None:
            d, flags = self.shift.estimate(frame)
            if self.shift.lf != self.lf:
                flags &= ~FLAG_CLAMPED                                                     # (its last level is not level_fine)
        F = sr.pyramid(sr.gray(frame), self.lc)
        q = np.zeros(2)
        for l in sorted(self.lv, reverse=True):
            lv = self.lv[l]
            if lv is None or not lv[6]:
                flags |= FLAG_LEVEL_SKIPPED
                continue
            b, J, xs, ys, L, D, valid = lv
            R = self.R[l]
            h, w = R.shape
            inv = 1.0 / 2 ** l
            lim, lin = self.max_shift / 2 ** l, self.max_linear
            s = d * inv
            clamped = lin_clamped = False
            for _ in range(self.iterations):
                fx, fy = positions(q, self.cx * inv, self.cy * inv, xs, ys, s[0], s[1])
                e = bilinear_at(F[l], fx, fy) - R[b:h - b, b:w - b]
                g = [sr._sum(Ji * e, self.order) for Ji in J]
                x = solve(L, D, g)
                t = np.array([q[0] - x[0], q[1] - x[1], s[0] - x[2], s[1] - x[3]])
                lin_clamped = bool(np.any(t[:2] < -lin) or np.any(t[:2] > lin))
                clamped = bool(np.any(t[2:] < -lim) or np.any(t[2:] > lim))
                q = np.minimum(np.maximum(t[:2], -lin), lin)
                s = np.minimum(np.maximum(t[2:], -lim), lim)
            d = s * 2 ** l
            if l == self.lf and clamped:
                flags |= FLAG_CLAMPED
            if l == self.lf and lin_clamped:
                flags |= FLAG_LINEAR_CLAMPED
        return np.array([q[0], q[1], d[0], d[1]]), flags

    def estimate_clip(self, frames):
        out = [self.estimate(f) for f in frames]
        return np.array([o[0] for o in out]).reshape(-1, 4), np.array([o[1] for o in out], np.int32)


def estimate_clip(frames, **kw):
    """params [N,4], flags [N] of a sequence since create / reset: the first frame is the reference"""
    return Reference(frames[0], **kw).estimate_clip(frames)


def warp(frames, params, out_dtype):
    """out[n][y][x] = bilinear(f_n, fx, fy) with the level-0 formula, converted; [N,H,W,3] uint8 channel by channel (out_dtype uint8)"""
    frames = np.asarray(frames)
    params = np.asarray(params, dtype=np.float64).reshape(-1, 4)
    N, H, W = frames.shape[:3]
    cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
    out = np.empty(frames.shape, dtype=out_dtype)
    for n in range(N):
        f = sr.channel_to_float(frames[n])
        fx, fy = positions(params[n], cx, cy, np.arange(W), np.arange(H), params[n, 2], params[n, 3])
        if f.ndim == 3:
            for ch in range(3):
                out[n, :, :, ch] = sr.convert(bilinear_at(f[:, :, ch], fx, fy), out_dtype)
        else:
            out[n] = sr.convert(bilinear_at(f, fx, fy), out_dtype)
    return out


def stabilize(frames, out_dtype, **kw):
    """(frames, params, flags) of rm_stab_sim_push on a fresh session"""
    params, flags = estimate_clip(frames, **kw)
    return warp(frames, params, out_dtype), params, flags


def corners(params, H, W):
    """[N,4,2]: the positions of the four frame corners under the parameters"""
    p = np.asarray(params, dtype=np.float64).reshape(-1, 4)
    cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
    out = np.empty((len(p), 4, 2))
    for k, (x, y) in enumerate(((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1))):
        u, v = x - cx, y - cy
        out[:, k, 0] = cx + ((1 + p[:, 0]) * u - p[:, 1] * v) + p[:, 2]
        out[:, k, 1] = cy + (p[:, 1] * u + (1 + p[:, 0]) * v) + p[:, 3]
    return out


def rotation_deg(params):
    p = np.asarray(params, dtype=np.float64).reshape(-1, 4)
    return np.degrees(np.arctan2(p[:, 1], 1 + p[:, 0]))


def zoom(params):
    p = np.asarray(params, dtype=np.float64).reshape(-1, 4)
    return np.hypot(1 + p[:, 0], p[:, 1])
