"""Shared by tests/test_emu_geometry.py and tests/test_gpu_geometry.py (not a test module): the newer entry points at the sizes where
their launch geometry turns -- partial folds over more than 64 tiles, grids capped in y or in blocks, frame buffers that start off a
16-byte boundary, the smallest and the thinnest frames.  The case tables of the other modules each stay inside one regime; this one holds
the others.  Every comparison is against a reference that exists already (tests/stabilize_reference.py, tests/stabilize_sim_reference.py,
tests/pulse_reference.py, tests/rate_cases.py, tests/stream_cases.py, the oracle); nothing here restates a kernel.  A backend `be` hides
where the memory lives, the union of what the case modules used here ask for:
    be.lib, be.ctx, be.stream()                 the bound library, a context, the stream argument
    be.dev(ndarray, offset=0) -> buffer         the array's bytes `offset` bytes past a 64-byte boundary, where the library reads them
    be.full(shape, dtype, value) -> buffer      a result area filled with a sentinel;  be.out(shape): float64 NaNs;  be.out_i32(shape): -7
    be.empty(shape, dtype) -> buffer            a result area;  be.np(buffer) -> its host copy
    be.get(buffer, dtype, shape) -> ndarray     the bytes of a be.dev / be.fill buffer read as `dtype`;  be.fill(nbytes): pulse_cases.SENTINEL
    be.p(buffer) -> c_void_p                    its address
    be.debug_set(key, value)                    rm_debug_set on the context

Tolerance of the fold cases (derived as in tests/stabilize_cases.py and tests/stabilize_sim_cases.py, recomputed on the cases here): D is
the largest spread of the restatement's own answer across the summation orders 'fsum', 'seq', 'rev' and 'pairwise' over all frames of all
FOLD_CASES; a build must stay within max(64 D, 2^-40) px of the 'fsum' form and report equal flags.  D as measured on the CPU (numpy 2),
for the record -- the tests compute it afresh:"""
import functools

import numpy as np

from respmon_amd import _capi, synth
from tests import pulse_cases as pc
from tests import pulse_reference as pr
from tests import rate_cases as rc
from tests import stabilize_cases as sc
from tests import stabilize_reference as sr
from tests import stabilize_sim_cases as ssc
from tests import stabilize_sim_reference as ssr
from tests import stream_cases as stc
from tests import window_cases as wc

RECORDED_D = {"shift": 2.2e-14, "sim": 2.3e-13}       # px; 64 D = 1.4e-12 and 1.5e-11 px, both above the floor of 2^-40 = 9.1e-13 px (the emulated build
                                                      # and the MI355X land at 8.9e-16 and 1.1e-13 px): more terms per sum than the 96 x 128 of the older tables
FACTOR, FLOOR = sc.FACTOR, sc.FLOOR
SENTINEL = sc.SENTINEL
same = sc.same
ESZ = {"u8": 1, "u16": 2, "f16": 2, "f32": 4, "f64": 8, "bgr": 1}


def code_of(frames):
    return sc.code_of(frames)


def oracle():
    from oracle import respmon_oracle
    respmon_oracle.build()
    return respmon_oracle


def as_read(frames):
    """the frames as every entry point reads them, float64 [T,H,W] (BGR: the oracle's cvtColor first)"""
    frames = np.asarray(frames)
    if frames.ndim == 4:
        frames = np.stack([oracle().cvtColor_bgr2gray(np.ascontiguousarray(f)) for f in frames])
    return sr.channel_to_float(frames)


# ---- 1. folds over more than 64 tiles ---------------------------------------------------------------------------------------------
# name -> (H, W, kind, level_linear of the similarity model).  The reduction tile is 64 wide and 16 high; stab_wave_fold
# (rm_stabilize_kernels.h) gives lane k the tiles k, k + 64, ...  The border of a linear level grows with the frame's half-diagonal
# (max_linear * (cx + cy) = 62 px at 16 x 4160, of 16 rows), so that shape has no linear level: there the similarity session runs its
# shift levels alone (level_linear -1), the two-sum fold over 65 tiles behind rm_stab_sim_push; the ten-sum fold has the other shapes.
FOLD_CASES = {
    "520x65": (520, 65, "u8", 1),           # 33 x 2 = 66 tiles: the second trip, two lanes
    "16x4160": (16, 4160, "u8", -1),        # 1 x 65 = 65 tiles: the second trip, one lane; levels 1 and 2 have no region (flag bit 0)
    "1040x129": (1040, 129, "u8", 1),       # 65 x 3 = 195 tiles: three trips, the last partial
    "520x65_bgr": (520, 65, "bgr", 1),
}
FOLD = dict(level_coarse=2, level_fine=0, iterations=2, max_shift=4.0)
NF = 5


def fold_tiles(name):
    H, W, kind, ll = FOLD_CASES[name]
    return ((W + 63) // 64) * ((H + 15) // 16)


@functools.lru_cache(maxsize=None)
def fold_frames(name, model):
    """the first NF frames of the clip tests/stabilize_cases.py (shifts) or tests/stabilize_sim_cases.py (rotation, zoom and shifts, where
    the similarity session has a linear level) draws for the shape"""
    H, W, kind, ll = FOLD_CASES[name]
    k = (sc._clip_u8(H, W, FOLD["max_shift"])[0] if model == "shift" or ll < 0 else ssc._clip_u8(H, W, FOLD["max_shift"])[0])[:NF]
    v = np.array(ssc.as_kind(k, kind))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def fold_reference(name, model):
    """{order: (shifts [NF,2] or params [NF,4], flags [NF])} of the restatement, every summation order"""
    f = fold_frames(name, model)
    if model == "shift":
        return {order: sr.estimate_clip(f, order=order, **FOLD) for order in sr.ORDERS}
    return {order: ssr.estimate_clip(f, order=order, level_linear=FOLD_CASES[name][3], max_linear=ssc.MAX_LINEAR, **FOLD) for order in ssr.ORDERS}


def _answer(name, model, v):
    """what the tolerance is about: the shift itself, or the positions of the four frame corners"""
    return v if model == "shift" else ssr.corners(v, *FOLD_CASES[name][:2])


@functools.lru_cache(maxsize=None)
def fold_spread(model):
    D = 0.0
    for name in FOLD_CASES:
        ref = fold_reference(name, model)
        s = np.stack([_answer(name, model, ref[order][0]) for order in sr.ORDERS])
        D = max(D, float((s.max(axis=0) - s.min(axis=0)).max()))
        assert all(np.array_equal(ref[order][1], ref["fsum"][1]) for order in sr.ORDERS), name
    return D


def fold_tolerance(model):
    return max(FACTOR * fold_spread(model), FLOOR)


def check_fold_case(be, name, model):
    H, W, kind, ll = FOLD_CASES[name]
    assert fold_tiles(name) > 64
    ref, ref_flags = fold_reference(name, model)["fsum"]
    tol, D = fold_tolerance(model), fold_spread(model)
    f = fold_frames(name, model)
    if model == "shift":
        ses, warp = sc.Session(be, H, W, FOLD["level_coarse"], FOLD["level_fine"], FOLD["iterations"], FOLD["max_shift"]), sc.warp
    else:
        ses = ssc.Session(be, H, W, FOLD["level_coarse"], FOLD["level_fine"], ll, FOLD["iterations"], FOLD["max_shift"], ssc.MAX_LINEAR)
        warp = ssc.warp
    out_dtype = np.uint8 if kind == "bgr" else np.float64
    with ses as s:
        out, got, flags = s.push(f, out_dtype)
        assert s.info()[:2] == (NF, 1)
    err = float(np.abs(_answer(name, model, got) - _answer(name, model, ref)).max())
    print("%s (%s, %d tiles): max |device - restatement| %.3g px (bound %.3g, D %.3g, recorded D %.3g); flags %s"
          % (name, model, fold_tiles(name), err, tol, D, RECORDED_D[model], sorted(set(flags.tolist()))))
    assert np.array_equal(got[0], np.zeros(got.shape[1])) and not np.signbit(got[0]).any()     # the reference itself
    assert np.array_equal(flags, ref_flags), (name, flags, ref_flags)
    assert err <= tol, (name, err, tol)
    assert np.abs(ref[1:, -2:]).max() > 0.25 * FOLD["max_shift"]                             # the case is not vacuous
    assert same(out, warp(be, f, got, out_dtype)), name


# ---- 2. the row cap and long-thin frames in the four warps -------------------------------------------------------------------------
# The warps launch min(H, 65535) rows and take the others in further passes (rm_stabilize.hip stab_warp, stab_warp_sim).
THIN_SHAPES = ((65537, 1), (65536, 2), (131075, 2), (1, 70000), (3, 66000))       # two passes (one row in the second), ..., three passes; 274 and 258 workgroups in x
THIN_BGR_SHAPES = ((65537, 1), (1, 70000))
THIN_N = 4


@functools.lru_cache(maxsize=None)
def thin_frames(H, W, kind, n=THIN_N):
    """n frames of noise whose every value is at least 16 gray levels, so that no warped uint8 value is the sentinel"""
    rng = np.random.Generator(np.random.PCG64([H, W, n]))
    k = rng.integers(16, 256, size=(n, H, W, 3) if kind == "bgr" else (n, H, W), dtype=np.uint8)
    v = k if kind in ("u8", "bgr") else np.array(ssc.as_kind(k, kind))
    v.setflags(write=False)
    return v


def check_thin_warp(be, model, H, W, kind):
    f = thin_frames(H, W, kind)
    out_dtype = np.float64 if kind == "f64" else np.uint8
    if model == "shift":
        got, want = sc.warp(be, f, sc.WARP_SHIFTS[:THIN_N], out_dtype), sr.warp(f, sc.WARP_SHIFTS[:THIN_N], out_dtype)
    else:
        got, want = ssc.warp(be, f, ssc.WARP_PARAMS[:THIN_N], out_dtype), ssr.warp(f, ssc.WARP_PARAMS[:THIN_N], out_dtype)
    assert (got[:, -1] != SENTINEL).all() and (got[:, :, -1] != SENTINEL).all(), (model, H, W, kind)   # the last row and column were written
    assert same(got, want), (model, H, W, kind, int((got != want).sum()))
    assert same(got[0], sr.convert(sr.channel_to_float(f[0]), got.dtype))                  # a zero transform: the conversion rule
    assert not same(got[1], got[0]) and len(np.unique(got[1])) > 16                        # the case is not vacuous


# ---- 3a. rm_bgr_to_gray: block cap, grid stride, scalar tail and misaligned bases together ---------------------------------------------
# The launch takes aligned quads with at most 1 << 16 blocks of 256 lanes and strides beyond; 1- to 3-byte misaligned bases take the
# scalar kernel for everything (rm_ctx.hip launch_bgr_to_gray).  NPIX_CAP on aligned bases: 256 * 65536 + 1 quads, one block more than the
# cap, so the quad kernel makes a second trip of a single quad, and a scalar tail of npix % 4 = 1 pixel; on misaligned bases the scalar
# kernel alone, four full trips of the capped grid and five pixels of a fifth.
NPIX_CAP = 4 * 256 * 65536 + 5
NPIX_SMALL = 4 * 256 * 3 + 5
GRAY_OFFSETS = tuple((i, o) for i in range(4) for o in range(4))
GUARD = 8


@functools.lru_cache(maxsize=2)
def gray_case(npix):
    """(bgr bytes [npix, 3], the oracle's gray [npix]): noise of a period that no grid size divides"""
    block = np.random.Generator(np.random.PCG64(npix)).integers(0, 256, size=1000003, dtype=np.uint8)
    bgr = np.resize(block, 3 * npix).reshape(npix, 3)
    rows = 1 << 16
    want = np.concatenate([oracle().cvtColor_bgr2gray(np.ascontiguousarray(bgr[a:a + rows][None]))[0] for a in range(0, npix, rows)])
    bgr.setflags(write=False)
    want.setflags(write=False)
    return bgr, want


def check_bgr_to_gray(be, npix, in_off, out_off):
    bgr, want = gray_case(npix)
    src = be.dev(bgr, offset=in_off)
    dst = be.dev(np.full(npix + GUARD, SENTINEL, np.uint8), offset=out_off)
    _capi.check(be.lib, be.lib.rm_bgr_to_gray(be.ctx, be.p(src), npix, be.p(dst), be.stream()), "rm_bgr_to_gray")
    got = be.get(dst, np.uint8, (npix + GUARD,))
    assert (got[npix:] == SENTINEL).all(), (in_off, out_off)
    bad = np.flatnonzero(got[:npix] != want)
    assert bad.size == 0, (in_off, out_off, bad.size, int(bad[0]), int(bad[-1]))
    assert len(np.unique(want[-5:])) > 1


# ---- 3b. misaligned and odd-sized frame buffers through the frame-buffer chain -------------------------------------------------------
# launch_down_chain (rm_down.hip) takes the vector arms when w % V == 0, h * w * esz % 16 == 0 and the base is 16-byte aligned; a view
# `off` bytes into an allocation, or an odd width, takes the element-wise arm.  off >= esz: the header promises element alignment only.
CHAIN_KINDS = ("u8", "u16", "f16", "f32", "f64", "bgr")
CHAIN_T = 16
CHAIN_KW = dict(fps=10.0, fmin=0.1, fmax=1.0, amp=500.0, thr=0.7)
CHAIN_LEVELS = 6


def chain_offsets(kind):
    return (1, 2, 8) if ESZ[kind] == 1 else tuple(sorted({ESZ[kind], 16 - ESZ[kind]}))


CHAIN_CASES = [(kind, 48, 64, off) for kind in CHAIN_KINDS for off in chain_offsets(kind)] + [(kind, 47, 65, 0) for kind in CHAIN_KINDS]


def chain_id(c):
    return "%s_%dx%d_off%d" % c


@functools.lru_cache(maxsize=None)
def chain_frames(kind, H, W, T=CHAIN_T):
    u8 = synth.synth_breathing(T, H, W, seed=H + W)
    if kind == "u16":
        rng = np.random.default_rng(W)
        v = (u8.astype(np.uint16) * 256 + rng.integers(0, 256, u8.shape).astype(np.uint16)).astype(np.uint16)     # the low byte matters
    elif kind == "bgr":
        rng = np.random.default_rng(H)
        v = np.ascontiguousarray(np.clip(u8[..., None].astype(np.int32) + rng.integers(-20, 21, u8.shape + (3,)), 0, 255).astype(np.uint8))
    elif kind == "u8":
        v = u8
    else:
        v = (u8 * (1.0 / 255)).astype({"f16": np.float16, "f32": np.float32, "f64": np.float64}[kind])
    v.setflags(write=False)
    return v


def both(be, frames, off, call):
    """call(buffer) on the aligned buffer and on the same bytes `off` bytes into a larger allocation: identical bit for bit; -> the first"""
    a = call(be.dev(frames, offset=0))
    if off:
        b = call(be.dev(frames, offset=off))
        for u, v in zip(a if isinstance(a, (list, tuple)) else [a], b if isinstance(b, (list, tuple)) else [b]):
            assert same(u, v), off
    return a


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def check_chain_calibrate(be, case):
    kind, H, W, off = case
    f = chain_frames(kind, H, W)
    kw = CHAIN_KW
    for skip in (1, 2, 4):
        def call(buf):
            heat = be.out((H, W))
            _capi.check(be.lib, be.lib.rm_calibrate(be.ctx, be.p(buf), code_of(f), CHAIN_T, H, W, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"],
                                                    CHAIN_LEVELS, skip, kw["thr"], 0, be.p(heat), None, be.stream()), "rm_calibrate")
            return be.np(heat)
        heat = both(be, f, off, call)
        ref, mid = oracle().locate(as_read(f), kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], pyramid_levels=CHAIN_LEVELS, skip_levels_at_top=skip,
                                   return_intermediates=True)
        assert np.abs(mid["avg_frame"]).max() > 0 and _rel(heat, mid["avg_frame"]) <= 1e-12, (case, skip, _rel(heat, mid["avg_frame"]))


def check_chain_rate_map(be, case):
    kind, H, W, off = case
    f = chain_frames(kind, H, W)
    kw = rc.RM_KW
    x = as_read(f)
    for level in (1, 3):
        h, w = rc.level_shape(H, W, level)

        def call(buf):
            outs = rc.Outs(be, h * w)
            _capi.check(be.lib, rc.rate_map_rc(be, buf, code_of(f), CHAIN_T, H, W, level, kw["fps"], kw["fmin"], kw["fmax"], kw["F"], outs), "rm_rate_map")
            return outs.np()
        got = both(be, f, off, call)
        g = np.ascontiguousarray(x)
        for _ in range(level):
            g = np.stack([oracle().pyrDown(t) for t in g])
        want = rc.peak(be, g.reshape(CHAIN_T, h * w), kw["fps"], kw["fmin"], kw["fmax"], kw["F"])
        rc.same_outputs(got, want, (case, level))
        assert (got[3] >= 0).any(), (case, level)


def check_chain_window(be, case, levels=3, skip=1):
    kind, H, W, off = case
    f = chain_frames(kind, H, W)
    kw = wc.KW
    want = both(be, f, 0, lambda buf: _calibrate(be, buf, f, levels, skip, kw))

    def call(buf):
        with wc.Window(be, CHAIN_T, H, W, levels, skip) as win:
            win.push(buf, code_of(f), CHAIN_T)
            return win.calibrate(kw)
    got = both(be, f, off, call)
    assert np.array_equal(got, want, equal_nan=True) and np.abs(want).max() > 0, case


def _calibrate(be, buf, f, levels, skip, kw):
    T, H, W = f.shape[:3]
    heat = be.out((H, W))
    _capi.check(be.lib, be.lib.rm_calibrate(be.ctx, be.p(buf), code_of(f), T, H, W, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], levels, skip, kw["thr"],
                                            0, be.p(heat), None, be.stream()), "rm_calibrate")
    return be.np(heat)


def check_chain_stream(be, case, L=4, S=2):
    kind, H, W, off = case
    f = chain_frames(kind, H, W)
    sos, zi = stc.design(True)
    x = as_read(f)
    want = x + stc.composition(be, x, L, S, sos, zi, stc.AMP)

    def call(buf):
        with stc.Stream(be, H, W, L, S, sos, zi) as st:
            out = be.empty((CHAIN_T, H, W), np.float64)
            _capi.check(be.lib, st.push_rc(buf, code_of(f), CHAIN_T, out, _capi.RM_F64), "rm_stream_push")
            return be.np(out)
    got = both(be, f, off, call)
    assert np.array_equal(got, want) and np.abs(want - x).max() > 1e-3, (case, float(np.abs(got - want).max()))


def check_chain_time_average(be, case):
    kind, H, W, off = case
    f = chain_frames(kind, H, W)

    def call(buf):
        out = be.out((H, W))
        rc_ = be.lib.rm_time_average(be.ctx, be.p(buf), code_of(f), CHAIN_T, H * W, be.p(out), be.stream())
        return rc_, be.np(out)
    if kind == "bgr":                                                                      # gray dtypes only (include/respmon_hip.h RM_BGR8)
        rc_, out = call(be.dev(f, offset=off))
        assert rc_ == _capi.RM_E_BADARG and np.isnan(out).all()
        return
    rc_, got = both(be, f, off, call)
    _capi.check(be.lib, rc_, "rm_time_average")
    acc = np.zeros((H, W))
    for t in as_read(f):
        acc = acc + t
    assert same(got, acc / CHAIN_T), case


# ---- 4. degenerate and extreme-aspect frames through the stateful entry points ---------------------------------------------------------
# (H, W): frames smaller than any tile, one row, one column, and rows / columns longer than a grid dimension.  T frames of noise: every
# pixel moves, nothing is smooth.
TINY_SHAPES = ((1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 3), (5, 4), (1, 65), (65, 1))
LONG_SHAPES = ((1, 70000), (70000, 1), (3, 66000))
EDGE_SHAPES = TINY_SHAPES + LONG_SHAPES
TINY_T, LONG_T = 6, 4
MAG_PAIRS = ((2, 0), (3, 1), (5, 3), (6, 4))              # (levels, skip): the plain path, the fused path at three depths
MAG_KW = dict(fps=10.0, fmin=0.1, fmax=1.0, amp=500.0)
EDGE_CHUNKS = (1, 2, 3)


def edge_T(H, W):
    return TINY_T if H * W < 1000 else LONG_T


@functools.lru_cache(maxsize=None)
def edge_frames(H, W, kind="u8"):
    T = edge_T(H, W)
    rng = np.random.Generator(np.random.PCG64([H, W, T]))
    v = rng.integers(0, 256, size=(T, H, W, 3) if kind == "bgr" else (T, H, W), dtype=np.uint8)
    v.setflags(write=False)
    return v


def eulerian_raw(be, frames, L, S, kw=MAG_KW):
    """raw_dev of rm_eulerian_magnification_bandpass"""
    T, H, W = frames.shape[:3]
    d, raw = be.dev(frames), be.out((T, H, W))
    _capi.check(be.lib, be.lib.rm_eulerian_magnification_bandpass(be.ctx, be.p(d), code_of(frames), T, H, W, kw["fps"], kw["fmin"], kw["fmax"],
                                                                   kw["amp"], L, S, 0.7, None, be.p(raw), None, be.stream()), "rm_eulerian_magnification_bandpass")
    return be.np(raw)


def magnify_f64(be, v, L, S, kw=MAG_KW):
    T, H, W = v.shape
    d, out = be.dev(v), be.full((T, H, W), np.float64, SENTINEL)
    _capi.check(be.lib, be.lib.rm_magnify(be.ctx, be.p(d), _capi.RM_U8, T, H, W, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], L, S, be.p(out),
                                          _capi.RM_F64, be.stream()), "rm_magnify")
    return be.np(out)


def check_edge_magnify(be, H, W):
    """rm_magnify: f + raw of the library bit for bit; rm_magnify_bgr: u8(clamp01(k * (1./255) + raw)) per channel"""
    kw = MAG_KW
    v, b = edge_frames(H, W), edge_frames(H, W, "bgr")
    T = len(v)
    f = as_read(v)
    for L, S in MAG_PAIRS:
        raw = eulerian_raw(be, v, L, S)
        m = magnify_f64(be, v, L, S)
        assert same(m, f + raw), (H, W, L, S, float(np.abs(m - (f + raw)).max()))
        raw_b = eulerian_raw(be, b, L, S)
        d, out = be.dev(b), be.full((T, H, W, 3), np.uint8, SENTINEL)
        _capi.check(be.lib, be.lib.rm_magnify_bgr(be.ctx, be.p(d), T, H, W, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], L, S, be.p(out), be.stream()),
                    "rm_magnify_bgr")
        assert same(be.np(out), stc.to_u8(b * (1.0 / 255) + raw_b[..., None])), (H, W, L, S)


def check_edge_magnify_reference(be, H, W, L, S):
    """rm_magnify within 4 d0 + e_raw of the oracle's collapse of the magnified pyramid, the bound of
    test_emu_magnify_means_what_the_reference_means (tests/test_emu_magnify.py): d0 the cost of the reordering measured with the oracle
    alone, e_raw the 1e-12 * max|raw| the suite allows between the library's raw and the oracle's, both over max|ref|"""
    from tests.test_emu_magnify import reference_magnified
    o, kw = oracle(), MAG_KW
    v = edge_frames(H, W)
    f = as_read(v)
    m = magnify_f64(be, v, L, S)
    ref = reference_magnified(o, f, kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], L, S)
    raw_o = o.eulerian_magnification_bandpass(f.copy(), kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], pyramid_levels=L, skip_levels_at_top=S)[1]
    scale = np.abs(ref).max()
    d0, e_raw, err = np.abs(ref - (f + raw_o)).max() / scale, 1e-12 * np.abs(raw_o).max() / scale, np.abs(m - ref).max() / scale
    print("magnify vs reference: T%d %dx%d L%d S%d d0=%.3g e_raw=%.3g err=%.3g max|raw of the oracle|=%.3g" % (len(v), H, W, L, S, d0, e_raw, err, np.abs(raw_o).max()))
    assert d0 < 1e-14 and err <= 4 * d0 + e_raw, (H, W, L, S, err, d0, e_raw)


def check_edge_stream(be, H, W, L=3, S=1):
    v = edge_frames(H, W)
    sos, zi = stc.design(True)
    x = as_read(v)
    want = x + stc.composition(be, x, L, S, sos, zi, stc.AMP)
    with stc.Stream(be, H, W, L, S, sos, zi) as st:
        assert same(st.run(v, _capi.RM_F64, EDGE_CHUNKS), want), (H, W)
        st.reset()
        assert same(st.run(v, _capi.RM_U8), stc.to_u8(want)), (H, W)
        assert st.info()[0] == len(v)


def check_edge_window(be, H, W, L=3, S=1):
    v = edge_frames(H, W)
    T = len(v)
    with wc.Window(be, T, H, W, L, S) as win:
        k = 0
        for n in (1, 2, T - 3, 2):                                                          # T + 2 frames: the ring wraps
            win.push_np(np.concatenate([v, v])[k:k + n])
            k += n
        assert win.info()[:2] == (T, 2)
        held = np.concatenate([v, v])[k - T:k]
        wc.same(win, held, L, S, tag=(H, W))
        # the rows are G_S whatever the size of level S (one pixel included): the window's rate map is rm_rate_map of the frames held
        kw = rc.RM_KW
        outs = rc.Outs(be, int(np.prod(rc.level_shape(H, W, S))))
        _capi.check(be.lib, rc.window_rate_map_rc(be, win, kw["fps"], kw["fmin"], kw["fmax"], kw["F"], outs), "rm_window_rate_map")
        rc.same_outputs(outs.np(), rc.rate_map(be, held, S, kw["fps"], kw["fmin"], kw["fmax"], kw["F"]), (H, W, L, S))


def check_edge_rate_map(be, H, W, level=1):
    v = edge_frames(H, W)
    kw = rc.RM_KW
    got = rc.rate_map(be, v, level, kw["fps"], kw["fmin"], kw["fmax"], kw["F"])
    ref = rc.Ref(rc.pyr_down_n(be, v, level), kw["fps"], kw["fmin"], kw["fmax"], kw["F"])
    print("rate map %dx%d: %s" % (H, W, rc.check_against(ref, *got, (H, W))))
    assert not ref.still.all()


def check_edge_stab(be, H, W):
    """no level of these frames has a region: both sessions skip every level as their restatements do, report exact zeros and hand the
    frames back converted"""
    v = edge_frames(H, W)
    T = len(v)
    rs, rf = sr.estimate_clip(v, **FOLD)
    rp, rpf = ssr.estimate_clip(v, level_linear=1, max_linear=ssc.MAX_LINEAR, **FOLD)
    assert (rf == sr.FLAG_LEVEL_SKIPPED).all() and (rpf == sr.FLAG_LEVEL_SKIPPED).all() and not rs.any() and not rp.any()
    want = sr.convert(sr.channel_to_float(v), np.uint8)
    with sc.Session(be, H, W, FOLD["level_coarse"], FOLD["level_fine"], FOLD["iterations"], FOLD["max_shift"]) as s:
        out, shifts, flags = s.push(v, np.uint8)
        assert np.array_equal(flags, rf) and same(shifts, rs) and same(out, want), (H, W)
        assert s.info()[:2] == (T, 1)
    with ssc.Session(be, H, W, FOLD["level_coarse"], FOLD["level_fine"], 1, FOLD["iterations"], FOLD["max_shift"], ssc.MAX_LINEAR) as s:
        out, par, flags = s.push(v, np.uint8)
        assert np.array_equal(flags, rpf) and same(par, rp) and same(out, want), (H, W)


def check_edge_phase(be, H, W):
    from tests import phase_cases as phc
    from tests import phase_reference as phr
    T = edge_T(H, W)
    v = phc.moving(T, H, W, "f64")
    sos, amp = phc.butter_sos(1), 20.0
    for levels in (2, 3):
        ref = phr.phase_magnify(v, levels, 0, sos, amp, True)
        D = max(float(np.abs(phr.phase_magnify(v, levels, 0, sos, amp, True, perturb_seed=seed) - ref).max()) for seed in (11, 12, 13))
        with phc.Phase(be, H, W, levels, 0, sos, amp) as ph:
            got = ph.push(v)
            assert ph.info()[0] == T
        phc.check_float(got, ref, D, "edge_%dx%d_levels%d float64" % (H, W, levels))


def check_edge_pulse(be, H, W):
    b = edge_frames(H, W, "bgr")
    for block in pc.BLOCKS:
        got = pc.block_sums(be, b, block)
        want = pr.block_sums(b, block)
        assert got.shape == want.shape and np.array_equal(got.astype(np.uint64), want), (H, W, block)
    rois = [(0, 0, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, H), (W // 2, H // 2, W - W // 2, H - H // 2)]
    assert np.array_equal(pc.roi_sums(be, b, rois).astype(np.uint64), pr.roi_sums(b, rois)), (H, W)
