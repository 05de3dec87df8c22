"""Shared by tests/test_emu_instantiations.py and tests/test_gpu_instantiations.py (not a test module): one case per kernel instantiation
that a run-time argument (or a debug knob) can select and that the feature suites did not launch -- the work list is the "never launched"
section of profiles/kernel_census.txt as tools/kernel_census.py found it before these cases existed (DESIGN.md "Launch census").

A case names its entry point, the arguments that select the instance, the instantiation(s) it claims in the census's spelling, and
runs the check function of the module that already judges that entry point: no case brings a tolerance or a reference of its own.
    rate     tests/rate_cases.py    check_against: the long-double reference; the ring arm bit for bit against rm_spectral_peak
    pulse    tests/pulse_cases.py   check_block_sums: numpy sums, exact
    filter   tests/stream_cases.py  sos_restated, bit for bit
    phase    tests/phase_cases.py   the numpy restatement within 64 D; every cut bit for bit with one push
    magnify  tests/test_emu_magnify.py's definition: f + raw of the library's own band-pass, bit for bit (stream: the sos_restated composition)
    chain    tests/geometry_cases.py  rm_rate_map against rm_spectral_peak of the oracle's pyrDown, bit for bit; rm_calibrate within 1e-12 of the oracle
    window   tests/window_cases.py  rm_calibrate on the contiguous frames, bit for bit
    flow     tests/flow_multi_cases.py  the rm_flow_step loop bit for bit, and that loop against the oracle's LK bit for bit
    roi      tests/roi_reference.py check_product

The emulated runner asserts the result AND that the claimed name is in the launched set; the GPU runner asserts the result only (there
is nothing to observe there).  The claims transfer because dispatch depends on the arguments, on alignment (the backends hand out
buffers aligned to 16 bytes or better; a case that claims an unaligned arm says so) and on the CU count, which the emulation answers as
256, the MI355X's own: the GPU runner refuses any other.

The feature modules grew up with a backend each (where the memory lives, how a buffer is typed); `Backends` carries one per module."""
import collections
import ctypes

import numpy as np

from respmon_amd import _capi
from tests import flow_multi_cases as fm
from tests import geometry_cases as gc
from tests import phase_cases as phc
from tests import pulse_cases as puc
from tests import rate_cases as rc
from tests import roi_reference as rr
from tests import stream_cases as sc
from tests import u16_cases as u16c
from tests import window_cases as wc

CUS = 256
Case = collections.namedtuple("Case", "id entry claims run")
Backends = collections.namedtuple("Backends", "lib ctx cus rate pulse stream phase roi flow")


# ---- backends ------------------------------------------------------------------------------------------------------------------
def _aligned(a, offset=0):
    """a copy of the bytes of `a`, `offset` bytes past a 64-byte boundary"""
    a = np.ascontiguousarray(a)
    raw = np.empty(a.nbytes + offset + 64, np.uint8)
    start = (-raw.ctypes.data) % 64 + offset
    view = raw[start:start + a.nbytes]
    view[:] = a.reshape(-1).view(np.uint8)
    return view


def emu_backends(emu):
    """the backends of tests/test_emu_{rate_map,pulse,stream,phase}.py on one emulated library and context"""
    def typed(a):
        a = np.ascontiguousarray(a)
        return _aligned(a).view(a.dtype).reshape(a.shape)

    class Common:
        lib, ctx, cus = emu.lib, emu.ctx, CUS
        stream = staticmethod(lambda: None)
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        np = staticmethod(lambda a: a)
        out = staticmethod(lambda shape: typed(np.full(shape, np.nan)))
        out_i32 = staticmethod(lambda shape: typed(np.full(shape, -7, np.int32)))

    class Rate(Common):
        dev = staticmethod(typed)

    class Pulse(Common):
        dev = staticmethod(_aligned)
        fill = staticmethod(lambda nbytes: _aligned(np.full(nbytes, puc.SENTINEL, np.uint8)))
        get = staticmethod(lambda buf, dtype, shape: buf.view(np.uint8).reshape(-1).view(dtype).reshape(shape).copy())

    class Stream(Common):
        dev = staticmethod(typed)
        empty = staticmethod(lambda shape, dtype: typed(np.zeros(shape, dtype)))

    class Phase(Common):
        dev = staticmethod(typed)
        full = staticmethod(lambda shape, dtype, value: typed(np.full(shape, value, dtype=dtype)))

    return Backends(emu.lib, emu.ctx, CUS, Rate, Pulse, Stream, Phase, rr.EmuRoi(emu), fm.EmuApi(emu))


def gpu_backends():
    """the backends of tests/test_gpu_{rate_map,pulse,stream,phase}.py (torch allocations are aligned to 256 bytes)"""
    import torch
    from respmon_amd import device
    TD = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32,
          np.dtype(np.float64): torch.float64}

    def typed(a):
        t = torch.from_numpy(np.array(a, order="C")).cuda()
        assert t.data_ptr() % 16 == 0
        return t

    def raw(a, offset=0):
        a = np.ascontiguousarray(a)
        buf = torch.empty(a.nbytes + offset, dtype=torch.uint8, device="cuda")
        view = buf[offset:]
        view.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
        assert view.data_ptr() % 16 == offset % 16
        return view

    class Common:
        lib = _capi.load()
        ctx = device.ctx()
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        stream = staticmethod(device.stream_ptr)
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        np = staticmethod(lambda t: t.cpu().numpy())
        out = staticmethod(lambda shape: torch.full(tuple(shape), float("nan"), dtype=torch.float64, device="cuda"))
        out_i32 = staticmethod(lambda shape: torch.full(tuple(shape), -7, dtype=torch.int32, device="cuda"))

    class Rate(Common):
        dev = staticmethod(typed)

    class Pulse(Common):
        dev = staticmethod(raw)
        fill = staticmethod(lambda nbytes: torch.full((nbytes,), puc.SENTINEL, dtype=torch.uint8, device="cuda"))
        get = staticmethod(lambda buf, dtype, shape: buf.cpu().numpy().view(dtype).reshape(shape))

    class Stream(Common):
        dev = staticmethod(typed)
        empty = staticmethod(lambda shape, dtype: torch.zeros(tuple(shape), dtype=TD[np.dtype(dtype)], device="cuda"))

    class Phase(Common):
        dev = staticmethod(typed)
        full = staticmethod(lambda shape, dtype, value: torch.full(tuple(shape), value, dtype=TD[np.dtype(dtype)], device="cuda"))

    from respmon_amd.base import _Backend
    return Backends(Common.lib, Common.ctx, Common.cus, Rate, Pulse, Stream, Phase, rr.GpuRoi(), fm.GpuApi(_Backend()))


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _b(v):
    return "true" if v else "false"


def _rate_cases():
    """rm_spectral_peak / rm_window_rate_map at NH = 3: nfreq 33 and 48, both forms (debug knob rate_wide), plain and ring"""
    out = []
    for F in rc.NH3_FS:
        for T in rc.NH3_TS:
            for wide in (0, 1):
                k = "rm::k_rate_peak_px" if wide else "rm::k_rate_peak"
                out.append(Case("rate_F%d_T%d_wide%d" % (F, T, wide), "rm_spectral_peak", ("%s<3, 0>" % k,),
                                lambda bk, T=T, F=F, wide=wide: rc.check_peak_form(bk.rate, T, F, wide)))
                out.append(Case("rate_F%d_T%d_wide%d_ring" % (F, T, wide), "rm_window_rate_map", ("%s<3, 1>" % k, "%s<3, 0>" % k),
                                lambda bk, T=T, F=F, wide=wide: rc.check_ring_form(bk.rate, T, F, wide)))
    for F, NH in ((16, 1), (64, 4)):           # the ring arm of the other instances no window test reached (RM_KW's nfreq 17 is NH = 2)
        for wide in (0, 1):
            k = "rm::k_rate_peak_px" if wide else "rm::k_rate_peak"
            out.append(Case("rate_F%d_T33_wide%d_ring" % (F, wide), "rm_window_rate_map", ("%s<%d, 1>" % (k, NH),),
                            lambda bk, F=F, wide=wide: rc.check_ring_form(bk.rate, 33, F, wide)))
    return out


PULSE_FAST_SHAPES, PULSE_BYTE_SHAPES = ((33, 64), (5, 1040)), ((17, 37), (3, 1030))      # W % 16 == 0: the 16-byte loads; else bytes


def _pulse_misaligned(be, block):
    """a frame tensor one byte into its allocation: the shape alone would take the 16-byte loads (check_block_sums_misaligned's case)"""
    frames = puc.block_inputs(3, 33, 64)[0][1]
    assert np.array_equal(puc.block_sums(be, frames, block, offset=1).astype(np.uint64), puc.pr.block_sums(frames, block)), block


def _pulse_cases():
    """rm_bgr_block_sums at blocks 8 (NB = 2) and 32 (L = 2), on the 16-byte path and on the byte path"""
    out = []
    for block in (8, 32):
        for fast, shapes in ((True, PULSE_FAST_SHAPES), (False, PULSE_BYTE_SHAPES)):
            out.append(Case("pulse_block%d_%s" % (block, "fast" if fast else "bytes"), "rm_bgr_block_sums", ("rm::k_bgr_block_sums<%d, %s>" % (block, _b(fast)),),
                            lambda bk, block=block, shapes=shapes: [puc.check_block_sums(bk.pulse, H, W, block, 3) for H, W in shapes]))
        out.append(Case("pulse_block%d_misaligned" % block, "rm_bgr_block_sums", ("rm::k_bgr_block_sums<%d, false>" % block,),
                        lambda bk, block=block: _pulse_misaligned(bk.pulse, block)))
    return out


FILTER_SECTIONS = (3, 4, 5, 7)


def _filter_cases():
    """rm_sosfilt (from rest and from zi) and rm_stream_push (cut three ways) with 3, 4, 5 and 7 sections: the section count is a switch
    inside k_sosfilt, so the census sees the four (STATE, INIT) kernels only; the count is in the arguments"""
    out = []
    for n in FILTER_SECTIONS:
        out.append(Case("sosfilt_sections%d" % n, "rm_sosfilt", ("rm::k_sosfilt<0, 0>", "rm::k_sosfilt<0, 1>"),
                        lambda bk, n=n: sc.check_sosfilt_sections(bk.stream, n, sc.SOS_RATES[1], Ts=(1, 2, 13), NPs=(1, 64, 65))))
        out.append(Case("stream_sections%d_rest" % n, "rm_stream_push", ("rm::k_sosfilt<1, 0>",), lambda bk, n=n: sc.check_stream_sections(bk.stream, n, False)))
        out.append(Case("stream_sections%d_zi" % n, "rm_stream_push", ("rm::k_sosfilt<1, 1>", "rm::k_sosfilt<1, 0>"),
                        lambda bk, n=n: sc.check_stream_sections(bk.stream, n, True)))
    return out


def _phase_cases():
    """rm_phase_push with the section counts the first table left out, whole (against the reference) and cut (bit for bit with the whole)"""
    out = []
    for n, blur in [(n, True) for n in phc.SECTIONS_BLUR] + [(n, False) for n in phc.SECTIONS_NO_BLUR]:
        name = ("moving_37x45_skip0_nsec%d_f64" if blur else "no_blur_nsec%d") % n
        claim = "rm::k_phase_time<%d, %s>" % (n if n <= 4 else 8, _b(blur))
        out.append(Case("phase_%s_whole" % name, "rm_phase_push", (claim,), lambda bk, name=name: phc.check_reference_case(bk.phase, name)))
        out.append(Case("phase_%s_cut" % name, "rm_phase_push", (claim,),
                        lambda bk, name=name: phc.check_chunk_invariance(bk.phase, internal=True, cases=((name, _capi.RM_F64),))))
    return out


# ---- rm_magnify / rm_magnify_bgr / rm_stream_push: k_magnify<S, Tin, Tout, SYM> and k_magnify_plain<Tin, Tout, SYM> ----------------------
# skip -> (H, W, levels): the smallest shapes of tests/test_emu_magnify.py that take the fused kernel at that S; 0: the plain sum
MAG_GEOMS = {1: (40, 70, 3), 2: (33, 64, 4), 3: (40, 72, 5), 4: (70, 152, 6), 0: (20, 30, 3)}
MAG_TIN = (("u8", "unsigned char"), ("u16", "short unsigned int"), ("f16", "__half"), ("f32", "float"), ("f64", "double"), ("bgr", "rm::bgr8_t"))
MAG_TOUT = ((_capi.RM_U8, "unsigned char"), (_capi.RM_U16, "short unsigned int"), (_capi.RM_F32, "float"), (_capi.RM_F64, "double"))
MAG_KW = (10.0, 0.1, 1.0, 500.0)          # fps, band, amplification


def mag_video(kind, N, H, W):
    if kind == "u16":
        v = sc.video(H, W, np.uint8)[:N].astype(np.uint16) * 257
        v.setflags(write=False)
        return v
    return sc.video(H, W, {"u8": np.uint8, "f16": np.float16, "f32": np.float32, "f64": np.float64, "bgr": "bgr"}[kind])[:N]


def mag_as_read(be, v):
    """f: the frames as the calibration reads them, float64"""
    return v.astype(np.float64) * u16c.SCALE if v.dtype == np.uint16 else sc.as_read(be, v)


def mag_convert(m, code):
    """the output conversions of the float64 sum m (tests/test_emu_magnify.py, tests/u16_cases.py)"""
    return {_capi.RM_F64: lambda: m, _capi.RM_F32: lambda: m.astype(np.float32), _capi.RM_U8: lambda: sc.to_u8(m), _capi.RM_U16: lambda: u16c.u16_of(m)}[code]()


def check_magnify(be, skip, kind):
    """rm_magnify's definition, bit for bit: m[t] = f[t] + raw[t], raw the raw_bandpassed_data of rm_eulerian_magnification_bandpass on the same
    buffer; every output dtype is the conversion of that sum; BGR frames also through rm_magnify_bgr (the same raw onto the three channels)"""
    H, W, L = MAG_GEOMS[skip]
    v = mag_video(kind, 6, H, W)
    T = len(v)
    d = be.dev(v)
    code = sc.code_of(v)
    raw = be.empty((T, H, W), np.float64)
    _capi.check(be.lib, be.lib.rm_eulerian_magnification_bandpass(be.ctx, be.p(d), code, T, H, W, *MAG_KW, L, skip, 0.7, None, be.p(raw), None, be.stream()),
                "rm_eulerian_magnification_bandpass")
    raw = be.np(raw)
    assert np.abs(raw).max() > 1e-3
    want = mag_as_read(be, v) + raw
    for oc, _ in MAG_TOUT:
        out = be.empty((T, H, W), sc.OUT_NP[oc])
        _capi.check(be.lib, be.lib.rm_magnify(be.ctx, be.p(d), code, T, H, W, *MAG_KW, L, skip, be.p(out), oc, be.stream()), "rm_magnify")
        assert np.array_equal(be.np(out), mag_convert(want, oc)), (skip, kind, oc)
    if kind == "bgr":
        out = be.empty(v.shape, np.uint8)
        _capi.check(be.lib, be.lib.rm_magnify_bgr(be.ctx, be.p(d), T, H, W, *MAG_KW, L, skip, be.p(out), be.stream()), "rm_magnify_bgr")
        assert np.array_equal(be.np(out), sc.to_u8(v * (1.0 / 255) + raw[..., None])), (skip, kind, "bgr out")


def check_stream_magnify(be, skip, kind):
    """rm_stream_push's definition (tests/stream_cases.py: the composition with sos_restated as the filter), one push of nine frames
    (two frame groups of the sum kernel), in every output dtype"""
    H, W, L = MAG_GEOMS[skip]
    v = mag_video(kind, 9, H, W)
    sos, zi = sc.design(True)
    raw = sc.composition(be, mag_as_read(be, v), L, skip, sos, zi, sc.AMP)
    assert np.abs(raw).max() > 1e-3
    want = mag_as_read(be, v) + raw
    with sc.Stream(be, H, W, L, skip, sos, zi) as st:
        for oc, _ in MAG_TOUT:
            assert np.array_equal(st.run(v, oc), mag_convert(want, oc)), (skip, kind, oc)
            st.reset()
        if kind == "bgr":
            assert np.array_equal(st.run(v, _capi.RM_BGR8), sc.to_u8(v * (1.0 / 255) + raw[..., None])), (skip, kind, "bgr out")


def _magnify_cases():
    out = []
    for sym, entry, check in ((1, "rm_magnify", check_magnify), (0, "rm_stream_push", check_stream_magnify)):
        for skip in (1, 2, 3, 4, 0):
            for kind, tin in MAG_TIN:
                fmt = ("rm::k_magnify<%d, " % skip if skip else "rm::k_magnify_plain<") + tin + ", %s, " + "%d>" % sym
                claims = tuple(fmt % tout for _, tout in MAG_TOUT) + ((fmt % "rm::bgr8_t",) if kind == "bgr" else ())
                out.append(Case("%s_%s_%s" % (entry[3:], "S%d" % skip if skip else "plain", kind), entry, claims,
                                lambda bk, check=check, skip=skip, kind=kind: check(bk.stream, skip, kind)))
    return out


# ---- the frame-buffer chain k_down_chain<Tin, S, VB> through rm_rate_map ---------------------------------------------------------------
DC_TIN = (("u8", "unsigned char"), ("u16", "short unsigned int"), ("f16", "__half"), ("f32", "float"), ("f64", "double"))
DC_THIN, DC_DEEP = (2, 70), (33, 47)       # two rows: a filtered level of fewer than three rows takes VB = true at every depth; 33 rows keep three at level 4


def check_down_chain(be, H, W, level, kind):
    """check_rate_map_equals_peak for one dtype: rm_rate_map (the fused chain to level `level`, then the contraction) equals rm_spectral_peak
    of the ORACLE's pyrDown applied `level` times to the frames as the calibration reads them, bit for bit (geometry_cases.check_chain_rate_map's
    comparison)"""
    kw = rc.RM_KW
    v = rc.ring_frames(9, H, W)
    frames = {"u8": lambda: v, "u16": lambda: v.astype(np.uint16) * 257, "f16": lambda: (v * (1. / 255)).astype(np.float16),
              "f32": lambda: (v * (1. / 255)).astype(np.float32), "f64": lambda: v * (1. / 255)}[kind]()
    T = len(frames)
    h, w = rc.level_shape(H, W, level)
    outs = rc.Outs(be, h * w)
    _capi.check(be.lib, rc.rate_map_rc(be, be.dev(frames), sc.code_of(frames), T, H, W, level, kw["fps"], kw["fmin"], kw["fmax"], kw["F"], outs), "rm_rate_map")
    g = np.ascontiguousarray(gc.as_read(frames))
    for _ in range(level):
        g = np.stack([gc.oracle().pyrDown(t) for t in g])
    want = rc.peak(be, g.reshape(T, h * w), kw["fps"], kw["fmin"], kw["fmax"], kw["F"])
    rc.same_outputs(outs.np(), want, (H, W, level, kind))
    assert (want[3] >= 0).all(), (H, W, level, kind)


def _down_chain_cases():
    out = []
    for kind, tin in DC_TIN:
        for S in (1, 2, 3, 4, 5):
            out.append(Case("down_chain_%s_S%d_thin" % (kind, S), "rm_rate_map", ("rm::k_down_chain<%s, %d, true>" % (tin, S),),
                            lambda bk, S=S, kind=kind: check_down_chain(bk.rate, *DC_THIN, S, kind)))
    for kind, tin in (("f16", "__half"), ("f32", "float")):
        out.append(Case("down_chain_%s_S5" % kind, "rm_rate_map", ("rm::k_down_chain<%s, 5, false>" % tin,),
                        lambda bk, kind=kind: check_down_chain(bk.rate, *DC_DEEP, 5, kind)))
    return out


# ---- the ring arm of the matrix-core temporal filter at two and three tiles of merged rows -------------------------------------------
# (T, band): the number of kept frequency bins decides the tiles; tests/window_cases.py's band (0.25 - 0.9 Hz at 2.5 fps, T <= 16) keeps one
WINDOW_TILES = {2: (128, dict(wc.KW, fps=10.0, fmin=0.1, fmax=4.9)), 3: (128, dict(wc.KW, fps=10.0, fmin=0.0, fmax=5.0))}


def check_window_tiles(be, tiles, wide):
    """window_cases.same with a band of its own: a window whose head has wrapped gives the heatmap of rm_calibrate on the contiguous
    frames it holds, bit for bit"""
    T, kw = WINDOW_TILES[tiles]
    H, W, L, S = wc.SMALL
    v = wc.stream(T, H, W)
    k = T + 2
    with wc.Knobs(be, {"temporal_wide": wide}), wc.Window(be, T, H, W, L, S) as win:
        win.push_np(v[:T])
        win.push_np(v[T:k])
        assert win.info()[:2] == (T, 2)
        want = wc.contiguous(be, v[k - T:k], L, S, kw=kw)[0]
        got = win.calibrate(kw)
    assert np.array_equal(got, want, equal_nan=True), (tiles, wide, float(np.abs(got - want).max()))
    assert np.abs(want).max() > 0


def _window_cases():
    return [Case("window_temporal_tiles%d_wide%d" % (tiles, wide), "rm_window_calibrate",
                 ("rm::k_temporal_sym%s<%d, 1>" % ("_px" if wide else "", tiles), "rm::k_temporal_sym%s<%d, 0>" % ("_px" if wide else "", tiles)),
                 lambda bk, tiles=tiles, wide=wide: check_window_tiles(bk.rate, tiles, wide)) for tiles in (2, 3) for wide in (0, 1)]


# ---- the tile kernel of the labelled components at 4 and 8 waves per tile (debug knob ccl_tile_waves; the library picks 16, or 8 from
# 2048 tiles on) ---------------------------------------------------------------------------------------------------------------------
def check_ccl_waves(roi_be, waves):
    """roi_reference.check_product (every path of the contour stage against the border-free reference) with the knob held"""
    roi_be.set("ccl_tile_waves", waves)
    try:
        for case in rr.cases(64, 128):
            if case.name.startswith(("a_noise0.45", "b_blobs_specks", "c_")):
                rr.check_product(roi_be, case, lists=False, clip_labelled=False)
    finally:
        roi_be.set("ccl_tile_waves", 0)


def check_u8_to_float(be):
    """rm_uint8_to_float is transforms.py's uint8_to_float: one multiplication by 1. / 255 per element, exact; every level, a length
    that is no multiple of the workgroup"""
    v = np.random.default_rng(8).permutation(np.arange(3 * 256 + 5) % 256).astype(np.uint8)
    out = be.empty(v.shape, np.float64)
    _capi.check(be.lib, be.lib.rm_uint8_to_float(be.ctx, be.p(be.dev(v)), be.p(out), v.size, be.stream()), "rm_uint8_to_float")
    assert np.array_equal(be.np(out), v * (1.0 / 255))


def _misc_cases():
    return [Case("ccl_tile_waves%d" % w, "rm_heatmap_to_roi", ("rm::k_ccl_tile<%d>" % w,), lambda bk, w=w: check_ccl_waves(bk.roi, w)) for w in (4, 8)] + \
           [Case("uint8_to_float", "rm_uint8_to_float", ("rm::k_u8_to_f64<>",), lambda bk: check_u8_to_float(bk.stream))]


# ---- the clip tracker's wide-window instance and the sequential finish kernels (tests/flow_multi_cases.py) ---------------------------------
def _flow_cases():
    out = [Case("flow_window%dx%d" % w, "rm_flow_multi_clip", ("rm::k_lk_track_multi_clip<16>",), lambda bk, w=w: fm.check_wide_window(bk.flow, w))
           for w in fm.WIDE_WINDOWS]
    out.append(Case("flow_7000_points", "rm_flow_step, rm_flow_multi_clip", ("rm::k_flow_finish_seq<>", "rm::k_flow_finish_multi_seq<>"),
                    lambda bk: fm.check_many_points(bk.flow)))
    return out


# ---- the per-pair tile bounds: a level-S row table beyond 64 KB of LDS even for one tile row ---------------------------------------------
TB = dict(H=10, W=66000, T=4, levels=3, skip=1)      # 1032 tile columns x 16 bytes x the five level-1 rows one tile row touches = 82 560 bytes


def check_tile_bounds(be):
    """geometry_cases.check_chain_calibrate's comparison: the heatmap of rm_calibrate within 1e-12 of the oracle's"""
    kw = gc.CHAIN_KW
    f = gc.chain_frames("u8", TB["H"], TB["W"], TB["T"])
    heat = gc._calibrate(be, be.dev(f), f, TB["levels"], TB["skip"], kw)
    _, mid = gc.oracle().locate(gc.as_read(f), kw["fps"], kw["fmin"], kw["fmax"], kw["amp"], pyramid_levels=TB["levels"], skip_levels_at_top=TB["skip"],
                                return_intermediates=True)
    assert np.abs(mid["avg_frame"]).max() > 0 and gc._rel(heat, mid["avg_frame"]) <= 1e-12, gc._rel(heat, mid["avg_frame"])


def _bounds_cases():
    return [Case("tile_bounds_10x66000", "rm_calibrate", ("rm::k_tile_bounds<>",), lambda bk: check_tile_bounds(bk.rate))]


CASES = _rate_cases() + _pulse_cases() + _filter_cases() + _phase_cases() + _magnify_cases() + _down_chain_cases() + _window_cases() + _misc_cases() + _flow_cases() + _bounds_cases()
assert len({c.id for c in CASES}) == len(CASES)


# ---- the references alone (no library) -------------------------------------------------------------------------------------------
def check_references_alone():
    """the randomised or capped references meet their own caps on the inputs the cases above bring"""
    for F in rc.NH3_FS:
        for T in rc.NH3_TS:
            _, ref = rc._ref_case1(T, F)
            for n in rc.NH3_NPS:
                rc.reference_caps(ref, n, (T, F, n))
    phc.check_reference_alone_meets_the_float_cap(phc.SECTION_CASES)
