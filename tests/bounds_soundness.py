"""Shared body of tests/test_emu_bounds_soundness.py and tests/test_gpu_bounds_soundness.py (test infrastructure only).

A tile bound is SOUND when tile_lo[u, tile] <= every full-resolution raw value of its (unique frame, 16 x 64 tile) pair and
tile_hi[u, tile] >= every one.  The selection (k_select_pairs), the store-less sums and the level-1 stops prune on that promise, so an
unsound bound silently changes the heatmap.  Here every bound producer is driven through its switch, its bounds are checked against
the full-resolution values the oracle's pyrUp forms from the device's own collapsed level, and the heatmap / extrema against the
exhaustive evaluation -- at magnitudes from 1e-300 to 1e300, where float32 intermediates overflow or underflow.

A `runner` hides the two libraries: calibrate(v, amp, L, S, flags) -> (heat ndarray, (min, max)), set(key, value),
workspace(name, shape), kept(), locate(v, amp, L, S)."""
import numpy as np

FLAG_NO_PRUNE, FLAG_TINY_STORE, FLAG_DENSE_SUM, FLAG_SPARSE_SUM, FLAG_FF_PER_LEVEL = 1, 4, 128, 256, 512
PRUNE_REL_MARGIN = 1e-12          # rm_kernels.h: the selection's margin, relative to the largest |bound|
DEFAULTS = dict(bounds_l1=2, bounds_scalar=0, bounds_l1_rows=0, bounds_up1=-1, dense_t_low=-1)

# amplifications of the ladder (negative ones too): float32 overflows from ~3e37 (intermediates of 64 |C_2|), float64 never here;
# at 1e-40 / 1e-44 float(C_2) is a float32 subnormal (the additive 2^-140 of the float32 margin), at 1e-300 it is zero
LADDER = [1e-300, 1e-44, 1e-40, 1e-30, 1.0, 500.0, 1e30, 3e37, 1e38, 1e39, 1e40, 1e100, 1e300]


def sizes(H, W, S):
    h, w = [H], [W]
    for _ in range(S):
        h.append((h[-1] + 1) // 2); w.append((w[-1] + 1) // 2)
    return h, w


def full_res(oracle, cS, H, W, S):
    """raw of every unique frame: S pyrUp steps of the device's collapsed level along the pyramid's sizes (transforms.py)."""
    h, w = sizes(H, W, S)
    out = np.empty((cS.shape[0], H, W))
    for u in range(cS.shape[0]):
        x = cS[u]
        for k in range(S - 1, -1, -1):
            x = oracle.pyrUp(x, (w[k], h[k]))
        out[u] = x
    return out


def tile_extrema(raw):
    """[unique frame][tile] min / max of 16 x 64 tiles (ragged edges clipped), vectorised."""
    Th, H, W = raw.shape
    nty, ntx = (H + 15) // 16, (W + 63) // 64
    p = np.full((Th, nty * 16, ntx * 64), np.inf); p[:, :H, :W] = raw
    mn = p.reshape(Th, nty, 16, ntx, 64).min(axis=(2, 4))
    p[:, :H, :W] = raw; p[:, H:, :] = -np.inf; p[:, :, W:] = -np.inf
    mx = p.reshape(Th, nty, 16, ntx, 64).max(axis=(2, 4))
    return mn.reshape(Th, -1), mx.reshape(Th, -1)


def check_sound(r, oracle, T, H, W, S, what):
    """the bounds the last call left against the full-resolution values of the device's own C_S"""
    Th = T // 2 + 1
    h, w = sizes(H, W, S)
    ntiles = ((H + 15) // 16) * ((W + 63) // 64)
    cS = r.workspace("cS", (Th, h[S], w[S]))
    lo = r.workspace("tile_lo", (Th, ntiles)); hi = r.workspace("tile_hi", (Th, ntiles))
    assert np.isfinite(cS).all(), what
    raw = full_res(oracle, cS, H, W, S)
    if not np.isfinite(raw).all():
        return                       # (the oracle itself overflows: nothing finite to bound)
    mn, mx = tile_extrema(raw)
    assert not np.isnan(lo).any() and not np.isnan(hi).any(), (what, "NaN bound")
    assert np.isfinite(lo).all() and np.isfinite(hi).all(), (what, "infinite bound while every value is finite")
    # the pairs are pruned on lo - m / hi + m (k_select_pairs), m = PRUNE_REL_MARGIN * the largest |bound|: the rounding of the
    # pyrUp chain between the bound's level and level 0 is what that margin is for
    m = PRUNE_REL_MARGIN * max(abs(hi.max()), abs(lo.min()))
    bad_lo = ~(lo - m <= mn); bad_hi = ~(hi + m >= mx)
    assert not bad_lo.any(), (what, "tile_lo above a value of its pair", int(bad_lo.sum()), lo[bad_lo][:3], mn[bad_lo][:3])
    assert not bad_hi.any(), (what, "tile_hi below a value of its pair", int(bad_hi.sum()), hi[bad_hi][:3], mx[bad_hi][:3])


def producers(S):
    """(switches, extra flags, name) of every bound producer reachable at skip S"""
    out = [({}, 0, "default (fused small pyramid where it fits)")]
    if S == 2:
        out += [({}, FLAG_FF_PER_LEVEL, "k_frame_bounds_l1f"),
                (dict(bounds_l1_rows=1), FLAG_FF_PER_LEVEL, "k_frame_bounds_l1f, one tile row per band"),
                (dict(bounds_l1=1), FLAG_FF_PER_LEVEL, "k_frame_bounds_l1"),
                (dict(bounds_l1=1, bounds_l1_rows=2), FLAG_FF_PER_LEVEL, "k_frame_bounds_l1, two tile rows per band")]
    out += [(dict(bounds_l1=0, bounds_scalar=1), FLAG_FF_PER_LEVEL, "level-S bounds, table form"),
            (dict(bounds_l1=0, bounds_scalar=2), FLAG_FF_PER_LEVEL, "level-S bounds, streaming rows")]
    if S in (3, 4):
        out += [(dict(bounds_up1=1), 0, "k_bounds_up1")]
    return out


def with_switches(r, sw, fn):
    try:
        for k, v in sw.items():
            r.set(k, v)
        return fn()
    finally:
        for k in sw:
            r.set(k, DEFAULTS[k])


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def same_mm(a, b):
    return all(x == y or (np.isnan(x) and np.isnan(y)) for x, y in zip(a, b))


def run_case(r, oracle, v, amp, L, S, what, prods=None, sums=True, sound=True):
    """every producer (or `prods`), every sum path: the exhaustive evaluation's heatmap and extrema bit for bit; bounds sound.
    Returns the exhaustive heatmap."""
    T, H, W = v.shape[:3]
    # (the exhaustive evaluation of the same front half: the per-level pyramid (FLAG_FF_PER_LEVEL) and the fused one may differ in
    #  the last bit of C_S, so each is compared with its own)
    exh = {b: r.calibrate(v, amp, L, S, b | FLAG_NO_PRUNE) for b in (0, FLAG_FF_PER_LEVEL)}
    ref, mm = exh[0]
    finite = np.isfinite(mm).all()
    for sw, fl, name in (producers(S) if prods is None else prods):
        tag = (what, amp, (T, H, W, L, S), name)
        ref_f, mm_f = exh[fl & FLAG_FF_PER_LEVEL]
        got, mm2 = with_switches(r, sw, lambda: r.calibrate(v, amp, L, S, fl))
        if sound and finite:
            check_sound(r, oracle, T, H, W, S, tag)
        assert same(got, ref_f) and same_mm(mm_f, mm2), (tag, "heatmap / extrema differ from the exhaustive evaluation")
    if S == 2 and prods is None:     # the float64 level-1 bounds: the same heatmap
        got, mm2 = with_switches(r, dict(bounds_l1=1), lambda: r.calibrate(v, amp, L, S, 0))
        assert same(got, ref) and same_mm(mm, mm2), (what, amp, "bounds_l1=1")
    if sums:
        for sw, fl, name in [({}, FLAG_DENSE_SUM, "dense sum"), ({}, FLAG_SPARSE_SUM, "sparse sum"), ({}, FLAG_TINY_STORE, "tiny store"),
                             (dict(dense_t_low=1), FLAG_DENSE_SUM, "k_dense_sum_t")]:
            got, mm2 = with_switches(r, sw, lambda: r.calibrate(v, amp, L, S, fl))
            assert same(got, ref) and same_mm(mm, mm2), (what, amp, (T, H, W, L, S), name)
    return ref


def mixed_scale(rng, T, H, W):
    """neighbouring tiles at 1e30 and 1e-30 (checkerboard of 16 x 64 tiles)"""
    v = rng.random((T, H, W))
    ty = (np.arange(H) // 16)[:, None]; tx = (np.arange(W) // 64)[None, :]
    return v * np.where((ty + tx) % 2 == 0, 1e30, 1e-30)


def hot_pixel(rng, T, H, W):
    """one pixel of 1e35 in one frame of a quiet stream"""
    v = rng.random((T, H, W)) * 1e-3
    v[T // 2, H // 3, W // 2] = 1e35
    return v


def to_dtype(v, kind):
    """a [0, 1) float64 video as a frame buffer of `kind` (f64 / f32 / f16 / u8 / bgr8)"""
    if kind == "f64":
        return v
    if kind == "f32":
        return v.astype(np.float32)
    if kind == "f16":
        return v.astype(np.float16)
    u8 = (v * 255).astype(np.uint8)
    if kind == "u8":
        return u8
    b = np.stack([u8, np.roll(u8, 1, axis=2), np.roll(u8, 2, axis=1)], axis=-1)
    return np.ascontiguousarray(b)


def with_non_finite(v, kind):
    """one NaN and one +inf pixel in different frames and tiles"""
    v = to_dtype(v, kind).copy()
    T, H, W = v.shape
    v[T // 3, H // 2, W // 3] = np.nan
    v[T - 1, H // 4, (3 * W) // 4] = np.inf
    return v
