"""TEST INFRASTRUCTURE: a numpy restatement of the rule of rm_stab_* and rm_warp_shift (include/respmon_hip.h), operation by operation,
in float64.  pyrDown and the integer cvtColor are the oracle's; everything else is written out here.

The only freedom the rule leaves is the order of its five sums.  `order` selects it: 'fsum' (math.fsum: exactly rounded, no order),
'seq' (left to right over the region, row-major), 'rev' (right to left) and 'pairwise' (numpy's).  The spread of the reported shift
across the four is what the tolerance of the tests is made of (tests/stabilize_cases.py)."""
import math

import numpy as np

from oracle import respmon_oracle as oracle

FLAG_LEVEL_SKIPPED, FLAG_CLAMPED = 1, 2
ORDERS = ("fsum", "seq", "rev", "pairwise")


def _sum(a, order):
    v = np.ascontiguousarray(a, dtype=np.float64).ravel()
    if order == "fsum":
        return math.fsum(v.tolist())
    if order == "seq":
        return float(np.cumsum(v)[-1])
    if order == "rev":
        return float(np.cumsum(v[::-1])[-1])
    return float(np.sum(v))


def channel_to_float(a):
    """a gray buffer (or the channels of a BGR one) as the library reads it"""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a * (1. / 255)
    if a.dtype == np.uint16:
        return a.astype(np.float64) * (1. / 65535)
    return a.astype(np.float64)


def gray(frame):
    """f: the gray value of one frame, [H,W] of a gray dtype or [H,W,3] uint8 BGR"""
    frame = np.asarray(frame)
    if frame.ndim == 3:
        return oracle.cvtColor_bgr2gray(frame) * (1. / 255)
    return channel_to_float(frame)


def pyramid(f, level_coarse):
    g = [np.ascontiguousarray(f, dtype=np.float64)]
    for _ in range(level_coarse):
        g.append(oracle.pyrDown(g[-1]))
    return g


def bilinear_grid(F, fx, fy):
    """bilinear(F, fx[i], fy[j]) for every (j, i): the sample positions of the rule form a grid (one shift per frame)"""
    h, w = F.shape
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[None, :], (fy - y0)[:, None]
    i0, i1 = np.clip(x0, 0, w - 1).astype(np.int64), np.clip(x0 + 1, 0, w - 1).astype(np.int64)
    j0, j1 = np.clip(y0, 0, h - 1).astype(np.int64), np.clip(y0 + 1, 0, h - 1).astype(np.int64)
    top, bot = F[j0], F[j1]
    return ((1 - ax) * top[:, i0] + ax * top[:, i1]) * (1 - ay) + ((1 - ax) * bot[:, i0] + ax * bot[:, i1]) * ay


class Reference:
    """The session's state for one reference frame: R_l and (a, bb, c, det) per level, and the estimate of any frame against it."""

    def __init__(self, frame, level_coarse=3, level_fine=0, iterations=2, max_shift=8.0, order="fsum"):
        self.lc, self.lf, self.iterations, self.max_shift, self.order = level_coarse, level_fine, iterations, float(max_shift), order
        self.R = pyramid(gray(frame), level_coarse)
        self.lv = {}
        for l in range(level_coarse, level_fine - 1, -1):
            R = self.R[l]
            h, w = R.shape
            b = int(math.ceil(self.max_shift / 2 ** l)) + 2
            if w - 2 * b < 1 or h - 2 * b < 1:
                self.lv[l] = None
                continue
            Rx = (0.5 * (R[:, 2:] - R[:, :-2]))[b:h - b, b - 1:w - b - 1]
            Ry = (0.5 * (R[2:, :] - R[:-2, :]))[b - 1:h - b - 1, b:w - b]
            a, bb, c = _sum(Rx * Rx, order), _sum(Rx * Ry, order), _sum(Ry * Ry, order)
            det = a * c - bb * bb
            self.lv[l] = (b, Rx, Ry, a, bb, c, det)

    def estimate(self, frame):
        """(d [2], flags) of one frame"""
        F = pyramid(gray(frame), self.lc)
        d = np.zeros(2)
        flags = 0
        for l in range(self.lc, self.lf - 1, -1):
            lv = self.lv[l]
            if lv is None or not (np.isfinite(lv[6]) and lv[6] > 0):
                flags |= FLAG_LEVEL_SKIPPED
                continue
            b, Rx, Ry, a, bb, c, det = lv
            R = self.R[l]
            h, w = R.shape
            lim = self.max_shift / 2 ** l
            s = d / 2 ** l
            xs, ys = np.arange(b, w - b, dtype=np.float64), np.arange(b, h - b, dtype=np.float64)
            clamped = False
            for _ in range(self.iterations):
                e = bilinear_grid(F[l], xs + s[0], ys + s[1]) - R[b:h - b, b:w - b]
                gx, gy = _sum(Rx * e, self.order), _sum(Ry * e, self.order)
                sx = s[0] - (c * gx - bb * gy) / det
                sy = s[1] - (a * gy - bb * gx) / det
                clamped = bool(sx < -lim or sx > lim or sy < -lim or sy > lim)
                s = np.array([min(max(sx, -lim), lim), min(max(sy, -lim), lim)])
            d = s * 2 ** l
            if l == self.lf and clamped:
                flags |= FLAG_CLAMPED
        return d, flags

    def estimate_clip(self, frames):
        out = [self.estimate(f) for f in frames]
        return np.array([o[0] for o in out]).reshape(-1, 2), np.array([o[1] for o in out], np.int32)


def estimate_clip(frames, **kw):
    """shifts [N,2], flags [N] of a sequence since create / reset: the first frame is the reference"""
    return Reference(frames[0], **kw).estimate_clip(frames)


def convert(m, out_dtype):
    """rm_magnify's output rules"""
    out_dtype = np.dtype(out_dtype)
    if out_dtype == np.float64:
        return m
    if out_dtype == np.float32:
        return m.astype(np.float32)
    scale = 255 if out_dtype == np.uint8 else 65535
    c = np.where(m < 0.0, 0.0, np.where(m > 1.0, 1.0, m))
    return (c * scale).astype(np.int64).astype(out_dtype)


def warp(frames, shifts, out_dtype):
    """out[n][y][x] = bilinear(f_n, x + d.x, y + d.y), converted; [N,H,W,3] uint8 channel by channel (out_dtype uint8)"""
    frames = np.asarray(frames)
    shifts = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    N, H, W = frames.shape[:3]
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    out = np.empty(frames.shape, dtype=out_dtype)
    for n in range(N):
        f = channel_to_float(frames[n])
        if f.ndim == 3:
            for ch in range(3):
                out[n, :, :, ch] = convert(bilinear_grid(f[:, :, ch], xs + shifts[n, 0], ys + shifts[n, 1]), out_dtype)
        else:
            out[n] = convert(bilinear_grid(f, xs + shifts[n, 0], ys + shifts[n, 1]), out_dtype)
    return out


def stabilize(frames, out_dtype, **kw):
    """(frames, shifts, flags) of rm_stab_push on a fresh session"""
    shifts, flags = estimate_clip(frames, **kw)
    return warp(frames, shifts, out_dtype), shifts, flags
