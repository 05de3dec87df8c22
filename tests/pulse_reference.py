"""The pulse path (include/respmon_hip.h rm_bgr_block_sums / rm_bgr_roi_sums / rm_pulse_pos) restated without the library (not a test
module): integer sums in numpy, POS in plain Python floats following the header's rule literally, and the textbook POS of the paper
(means subtracted, ratio of standard deviations) that the rule simplifies."""
import numpy as np


def block_sums(frames, block):
    """uint8 [N,H,W,3] -> uint64 [N, ceil(H/block), ceil(W/block), 3]"""
    f = np.asarray(frames).astype(np.uint64)
    rows = np.add.reduceat(f, np.arange(0, f.shape[1], block), axis=1)
    return np.add.reduceat(rows, np.arange(0, f.shape[2], block), axis=2)


def roi_sums(frames, rois):
    """uint8 [N,H,W,3], K rectangles (x, y, w, h) -> uint64 [N, K, 3]"""
    f = np.asarray(frames)
    return np.stack([f[:, y:y + h, x:x + w].astype(np.uint64).sum(axis=(1, 2)) for x, y, w, h in rois], axis=1)


def pos_scalar(s, l, alphas=None):
    """s: integer [N, NP, 3] (B, G, R) -> H [N, NP] float64, the rule of rm_pulse_pos operation by operation in Python floats (IEEE
    binary64, one rounding each; math.sqrt is correctly rounded).  `alphas`: a list that receives the a of every window that is not skipped."""
    import math
    s = np.asarray(s)
    N, NP = s.shape[:2]
    H = np.zeros((N, NP))
    fl = float(l)
    for p in range(NP):
        col = [[int(v) for v in s[t, p]] for t in range(N)]
        h_acc = [0.0] * N
        for n in range(N - l + 1):
            S = [sum(col[n + k][c] for k in range(l)) for c in range(3)]
            if S[0] == 0 or S[1] == 0 or S[2] == 0:
                continue
            Sf = [float(v) for v in S]
            S1, S2 = [], []
            for k in range(l):
                xb, xg, xr = ((float(col[n + k][c]) * fl) / Sf[c] for c in range(3))
                S1.append(xg - xb)
                S2.append((xg + xb) - 2.0 * xr)
            v1 = v2 = 0.0
            for k in range(l):
                v1 = v1 + S1[k] * S1[k]
                v2 = v2 + S2[k] * S2[k]
            a = math.sqrt(v1 / v2) if v2 > 0 else 0.0
            if alphas is not None:
                alphas.append(a)
            for k in range(l):          # ascending n for every t = n + k: the outer loop is ascending n
                h_acc[n + k] = h_acc[n + k] + (S1[k] + a * S2[k])
        H[:, p] = h_acc
    return H


def pos_textbook(s, l):
    """Algorithm 1 of Wang et al. 2017: C_n = C / mean_t(C), S = P C_n with P = [[0, 1, -1], [-2, 1, 1]] (R, G, B), h = S1 +
    std(S1) / std(S2) S2, H[n : n + l] += h - mean(h); a window with an all-zero channel is skipped, a zero std(S2) gives a = 0"""
    s = np.asarray(s).astype(np.float64)
    N, NP = s.shape[:2]
    H = np.zeros((N, NP))
    for p in range(NP):
        for n in range(N - l + 1):
            C = s[n:n + l, p, :]
            m = C.mean(axis=0)
            if (m == 0).any():
                continue
            Cn = C / m
            S1 = Cn[:, 1] - Cn[:, 0]
            S2 = Cn[:, 1] + Cn[:, 0] - 2.0 * Cn[:, 2]
            sd2 = S2.std()
            h = S1 + ((S1.std() / sd2) if sd2 > 0 else 0.0) * S2
            H[n:n + l, p] += h - h.mean()
    return H
