"""TEST INFRASTRUCTURE: a numpy restatement of the rule of rm_phase_* (include/respmon_hip.h), operation by operation, in float64.

Pyramid and collapse are the oracle's create_laplacian_video_pyramid / collapse_laplacian_video_pyramid (the device pyramid is bit-exact
against these); the filter is an explicit loop in rm_sosfilt's operation order; the blur is the separable 9-tap binomial, along x and
then along y, each pass the left-to-right sum of k[i] * v[i] with indices reflected 101 repeatedly.

Everything but atan2, cos and sin is reproducible bit for bit, so the tolerance of the tests comes from this file alone: with
`perturb_seed` every result of those three functions is multiplied by 1 + k * 2**-52, k uniform in -4 .. 4 (a libm a few ulp away from
numpy's; a value that is exact in every libm -- cos 0, sin 0, atan2(0, re) -- stays as it is, so a first frame has D == 0), and the largest
deviation D of such runs from the unperturbed one measures how far a correct implementation may land."""
import numpy as np

from oracle import respmon_oracle as oracle

KERNEL = np.array([1, 8, 28, 56, 70, 56, 28, 8, 1], dtype=np.float64) / 256


def reflect101(idx, n):
    """BORDER_REFLECT_101 applied until the index is inside (period 2 (n - 1)); an axis of length 1 reads index 0"""
    idx = np.asarray(idx)
    if n == 1:
        return np.zeros_like(idx)
    p = 2 * (n - 1)
    idx = np.mod(idx, p)
    return np.where(idx >= n, p - idx, idx)


def riesz(I):
    h, w = I.shape
    x, y = np.arange(w), np.arange(h)
    R1 = 0.5 * (I[:, reflect101(x + 1, w)] - I[:, reflect101(x - 1, w)])
    R2 = 0.5 * (I[reflect101(y + 1, h), :] - I[reflect101(y - 1, h), :])
    return R1, R2


def blur(v):
    h, w = v.shape
    xi = reflect101(np.arange(w)[:, None] + np.arange(-4, 5)[None, :], w)
    acc = KERNEL[0] * v[:, xi[:, 0]]
    for i in range(1, 9):
        acc = acc + KERNEL[i] * v[:, xi[:, i]]
    yi = reflect101(np.arange(h)[:, None] + np.arange(-4, 5)[None, :], h)
    out = KERNEL[0] * acc[yi[:, 0], :]
    for i in range(1, 9):
        out = out + KERNEL[i] * acc[yi[:, i], :]
    return out


class _Perturb:
    def __init__(self, seed):
        self.rng = None if seed is None else np.random.default_rng(seed)

    def __call__(self, v, exact):
        """`exact`: where the function's value is exact in every libm (cos 0 == 1, sin 0 == 0, atan2(0, re)): left alone"""
        if self.rng is None:
            return v
        return np.where(exact, v, v * (1.0 + self.rng.integers(-4, 5, size=v.shape).astype(np.float64) * 2.0 ** -52))


def _div_where(pos, num, den):
    out = np.zeros_like(num)
    np.divide(num, den, out=out, where=pos)
    return out


def to_float(frames):
    """a frame buffer as the library reads it"""
    frames = np.asarray(frames)
    if frames.dtype == np.uint8:
        return oracle.uint8_to_float(frames)
    if frames.dtype == np.uint16:
        return frames.astype(np.float64) * (1. / 65535)
    return frames.astype(np.float64)


def to_uint(m, scale):
    """rm_magnify's integer outputs: the clamp to [0, 1], then the C truncation of m * scale"""
    c = np.where(m < 0.0, 0.0, np.where(m > 1.0, 1.0, m))
    return (c * scale).astype(np.int64).astype(np.uint8 if scale == 255 else np.uint16)


def phase_magnify(frames, levels, skip, sos, amplification, blur_on=True, perturb_seed=None):
    """out[T,H,W] float64 (before the conversion) for the frames of one sequence since create / reset."""
    f = to_float(frames)
    T = f.shape[0]
    sos = np.asarray(sos, dtype=np.float64).reshape(-1, 6)
    assert np.all(sos[:, 3] == 1.0)
    pert = _Perturb(perturb_seed)
    pyr = oracle.create_laplacian_video_pyramid(f, levels)
    for l in range(skip, levels - 1):
        lvl = pyr[l]
        shape = lvl.shape[1:]
        Pc, Ps = np.zeros(shape), np.zeros(shape)
        zc, zs = np.zeros((len(sos), 2) + shape), np.zeros((len(sos), 2) + shape)
        Ip = R1p = R2p = None
        new = np.empty_like(lvl)
        for t in range(T):
            I = lvl[t]
            R1, R2 = riesz(I)
            if t == 0:
                dc, ds = np.zeros(shape), np.zeros(shape)
            else:
                re = (I * Ip + R1 * R1p) + R2 * R2p
                qx = Ip * R1 - I * R1p
                qy = Ip * R2 - I * R2p
                hyp = np.sqrt(qx * qx + qy * qy)
                d = pert(np.arctan2(hyp, re), hyp == 0)
                dc = np.where(hyp > 0, d * _div_where(hyp > 0, qx, hyp), 0.0)
                ds = np.where(hyp > 0, d * _div_where(hyp > 0, qy, hyp), 0.0)
            Pc = Pc + dc
            Ps = Ps + ds
            A = np.sqrt((I * I + R1 * R1) + R2 * R2)
            F = []
            for P, z in ((Pc, zc), (Ps, zs)):
                cur = P
                for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
                    nw = b0 * cur + z[s, 0]
                    z[s, 0] = (b1 * cur - a1 * nw) + z[s, 1]
                    z[s, 1] = b2 * cur - a2 * nw
                    cur = nw
                F.append(cur)
            Fc, Fs = F
            if blur_on:
                den, nc, ns = blur(A), blur(A * Fc), blur(A * Fs)
                bc = _div_where(den > 0, nc, den)
                bs = _div_where(den > 0, ns, den)
            else:
                bc, bs = Fc, Fs
            m = np.sqrt(bc * bc + bs * bs)
            am = amplification * m
            c, s = pert(np.cos(am), am == 0), pert(np.sin(am), am == 0)
            ux = _div_where(m > 0, bc, m)
            uy = _div_where(m > 0, bs, m)
            new[t] = I * c - (R1 * ux + R2 * uy) * s
            Ip, R1p, R2p = I, R1, R2
        pyr[l] = new
    return np.array(oracle.collapse_laplacian_video_pyramid(pyr))
