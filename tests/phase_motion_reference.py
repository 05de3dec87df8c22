"""TEST INFRASTRUCTURE: a numpy restatement of the rule of rm_phase_motion_* (include/respmon_hip.h), operation by operation, in
float64, down to the per-pixel terms wgt, wgt * dc, wgt * ds of every frame.

The level is the oracle's create_laplacian_video_pyramid on the crop with l + 2 levels (the device pyramid is bit-exact against it);
riesz, the perturbation of atan2 and the dtype conversion are those of tests/phase_reference.py, unchanged.  Everything but atan2 is
reproducible bit for bit, so the tolerance of the tests comes from this file alone: the sum of a frame's terms is taken with
math.fsum (exactly rounded, no order), any order of n terms stays within (n - 1) 2^-53 sum |term| of it, and with `perturb_seed`
every inexact atan2 is multiplied by 1 + k 2^-52, k uniform in -4 .. 4: the largest deviation D of such runs measures how far a
libm a few ulp away from numpy's may land."""
import math

import numpy as np

from oracle import respmon_oracle as oracle
from tests.phase_reference import _Perturb, riesz, to_float


def _div_where(pos, num, den):
    out = np.zeros_like(num)
    np.divide(num, den, out=out, where=pos)
    return out


def level_of(frames, roi, level):
    """I[T, lh, lw]: level `level` of the Laplacian pyramid of the crop, an image of its own"""
    x, y, w, h = roi
    crop = np.ascontiguousarray(to_float(np.asarray(frames)[:, y:y + h, x:x + w]))
    return np.array(oracle.create_laplacian_video_pyramid(crop, level + 2)[level])


def terms(frames, roi, level, perturb_seed=None):
    """(wgt, wgt * dc, wgt * ds), each [T, lh, lw], for the frames of one sequence since create / reset (frame 0: zeros)"""
    lvl = level_of(frames, roi, level)
    pert = _Perturb(perturb_seed)
    T = lvl.shape[0]
    tw, tc, ts = np.zeros_like(lvl), np.zeros_like(lvl), np.zeros_like(lvl)
    Ip = R1p = R2p = Ap = None
    for t in range(T):
        I = lvl[t]
        R1, R2 = riesz(I)
        A = np.sqrt((I * I + R1 * R1) + R2 * R2)
        if t > 0:
            re = (I * Ip + R1 * R1p) + R2 * R2p
            qx = Ip * R1 - I * R1p
            qy = Ip * R2 - I * R2p
            hyp = np.sqrt(qx * qx + qy * qy)
            d = pert(np.arctan2(hyp, re), hyp == 0)
            dc = np.where(hyp > 0, d * _div_where(hyp > 0, qx, hyp), 0.0)
            ds = np.where(hyp > 0, d * _div_where(hyp > 0, qy, hyp), 0.0)
            wgt = A * Ap
            tw[t], tc[t], ts[t] = wgt, wgt * dc, wgt * ds
        Ip, R1p, R2p, Ap = I, R1, R2, A
    return tw, tc, ts


def fsums(tr):
    """[T, 3]: the exactly rounded sums Sw, Sc, Ss of every frame"""
    T = tr[0].shape[0]
    return np.array([[math.fsum(a[t].ravel().tolist()) for a in tr] for t in range(T)])


def abs_sums(tr):
    """[T, 3]: sum |term| of every frame"""
    T = tr[0].shape[0]
    return np.array([[math.fsum(np.abs(a[t]).ravel().tolist()) for a in tr] for t in range(T)])


def velocity(sums):
    """v[T, 2] = (Sc / Sw, Ss / Sw), 0 where Sw == 0 (the first frame)"""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 3)
    v = np.zeros((len(s), 2))
    ok = s[:, 0] > 0
    v[ok, 0] = s[ok, 1] / s[ok, 0]
    v[ok, 1] = s[ok, 2] / s[ok, 0]
    return v
