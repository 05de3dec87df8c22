"""Shared by tests/test_emu_phase.py and tests/test_gpu_phase.py (not a test module): the clips, thin callers of rm_phase_* on raw
pointers and the checks both builds run against tests/phase_reference.py.  A backend `be` hides where the memory lives:
    be.lib, be.ctx, be.stream()                 the bound library, a context, the stream argument
    be.dev(ndarray) -> buffer                   an array where the library reads it (numpy itself on the host-emulated build)
    be.full(shape, dtype, value) -> buffer      a result area filled with a sentinel;  be.np(buffer) -> its host copy
    be.p(buffer) -> c_void_p                    its address; buffer[a:b] slices frames

Tolerance.  Everything in the rule but atan2, cos and sin is reproducible bit for bit, so the bound comes from the reference alone: D is
the largest deviation of three perturbed runs of the reference (every inexact result of the three functions times 1 + k 2^-52, k in
-4 .. 4) from its unperturbed run, and a build must agree with the unperturbed run within 64 D -- a libm may sit a couple of ulp from
numpy's, systematically; a bias adds up linearly over the running sum where the random perturbation adds up as sqrt(T); sqrt(T) <= 16
here gives x16, and x4 is margin.  D == 0 (nothing processed, T == 1) means bit for bit.  A wrong tap, sign or order shows at 1e-6.

Integer outputs may differ from the converted reference by one level, only where the reference's m * 255 (m * 65535) lies within
64 D * 255 (* 65535) of an integer, and in no more than 1 pixel of 1000.  The uint16 and float64 forms of the clips are built so that
no frame of the INPUT lies on such a boundary (check_reference_alone_meets_the_integer_cap); the uint8 form cannot be: its first frame
comes back as k * (1./255) * 255, next to the integer k, on both sides by the same bit-exact arithmetic.

D as measured on the CPU (numpy 2, glibc), for the record -- the tests compute it afresh:"""
import ctypes
import functools

import numpy as np

from respmon_amd import _capi
from tests import phase_reference as pr

RECORDED_D = {
    "moving_37x45_skip0_nsec1_u8": 4.4e-16, "moving_37x45_skip0_nsec1_u16": 5.6e-16, "moving_37x45_skip0_nsec1_f64": 4.4e-16,
    "moving_37x45_skip0_nsec3_u8": 5.6e-16, "moving_37x45_skip0_nsec3_u16": 4.4e-16, "moving_37x45_skip0_nsec3_f64": 4.4e-16,
    "moving_37x45_skip1_nsec1_u8": 3.3e-16, "moving_37x45_skip1_nsec1_u16": 3.3e-16, "moving_37x45_skip1_nsec1_f64": 4.4e-16,
    "moving_37x45_skip1_nsec3_u8": 3.3e-16, "moving_37x45_skip1_nsec3_u16": 3.3e-16, "moving_37x45_skip1_nsec3_f64": 3.3e-16,
    "moving_37x45_skip0_nsec2_f64": 4.4e-16, "moving_37x45_skip0_nsec4_f64": 4.4e-16, "moving_37x45_skip0_nsec6_f64": 4.4e-16,
    "tiny_5x7_levels3": 3.3e-16, "tiny_5x7_levels4": 3.3e-16, "row_1x9_levels2": 5.6e-16, "column_9x1_levels2": 7.8e-16,
    "degenerate": 2.2e-16, "moving_T1": 0.0, "moving_T2": 3.3e-16, "no_blur": 1.4e-15, "no_blur_nsec3_skip1": 5.6e-16,
    "moving_37x45_skip0_nsec5_f64": 4.4e-16, "moving_37x45_skip0_nsec7_f64": 5.6e-16, "moving_37x45_skip0_nsec8_f64": 4.4e-16,
    "no_blur_nsec2": 1.7e-15, "no_blur_nsec4": 1.0e-15, "no_blur_nsec7": 4.4e-16,
    "nothing_processed": 0.0, "one_level": 0.0, "bars": 6.7e-16, "wide_71x130_f64": 4.4e-16, "wide_71x130_f32": 5.6e-16, "wide_71x130_f16": 4.4e-16,
}

DT = {np.dtype(np.uint8): _capi.RM_U8, np.dtype(np.uint16): _capi.RM_U16, np.dtype(np.float16): _capi.RM_F16,
      np.dtype(np.float32): _capi.RM_F32, np.dtype(np.float64): _capi.RM_F64}
OUT_NP = {_capi.RM_U8: np.uint8, _capi.RM_U16: np.uint16, _capi.RM_F32: np.float32, _capi.RM_F64: np.float64}
FPS, BAND = 10.0, (0.2, 0.8)
FACTOR = 64


def butter_sos(order, fps=FPS, band=BAND):
    import scipy.signal
    return np.ascontiguousarray(scipy.signal.butter(order, [band[0] / (fps / 2), band[1] / (fps / 2)], btype='band', output='sos'))


# ---- the clips -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _moving_u8(T, H, W):
    """a smooth pattern that moves by a fraction of a pixel per frame, plus 1 % noise, quantised to uint8"""
    rng = np.random.default_rng(1000 * H + W)
    t, y, x = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    sh = 0.35 * np.sin(2 * np.pi * 0.4 * t / FPS)
    v = 0.5 + 0.2 * np.sin(2 * np.pi * (x - sh) / 7.3) * np.cos(2 * np.pi * (y + 0.6 * sh) / 9.1) + 0.08 * np.sin(2 * np.pi * (x + y - sh) / 23.0)
    v = v + 0.01 * rng.standard_normal(v.shape)
    k = np.clip(np.round(v * 255), 44, 255).astype(np.uint8)
    k.setflags(write=False)
    return k


def moving(T, H, W, kind):
    """the clip as uint8, as uint16 (256 k + 300: k + (300 - k) / 257 levels of 255, never an integer for k >= 44) or as float64
    ((k + 0.37) / 255; "f32" / "f16": that rounded)"""
    k = _moving_u8(T, H, W)
    if kind == "u8":
        return k
    if kind == "u16":
        return (k.astype(np.uint16) * 256 + 300).astype(np.uint16)
    v = (k + 0.37) / 255
    return v if kind == "f64" else v.astype({"f32": np.float32, "f16": np.float16}[kind])


@functools.lru_cache(maxsize=None)
def degenerate_clip(T=6, H=32, W=56):
    """exactly zero and exactly flat regions (Laplacian exactly 0: hyp == 0, den == 0, m == 0), a static step between them, and a
    small moving blob"""
    v = np.zeros((T, H, W))
    v[:, :, 24:] = 0.5
    y, x = np.mgrid[0:H, 0:W]
    for t in range(T):
        v[t] += 0.25 * np.exp(-((x - 46 - 0.3 * np.sin(1.3 * t)) ** 2 + (y - 20 - 0.2 * t) ** 2) / 8.0) * (x >= 40)
    v[:, :, 40:] = np.round(v[:, :, 40:] * 4096) / 4096
    v.setflags(write=False)
    return v


BARS = dict(H=24, W=96, T=96, fps=10.0, f=0.4, px=0.1, amp=20.0, levels=5, order=1, band=(0.2, 0.8), centres=(30.0, 66.0), sigma=2.0)


@functools.lru_cache(maxsize=None)
def bars_clip():
    """two vertical bars on 0.2, peak 0.8, moving 0.1 px at 0.4 Hz"""
    P = BARS
    x = np.arange(P["W"])[None, None, :]
    d = P["px"] * np.sin(2 * np.pi * P["f"] * np.arange(P["T"]) / P["fps"])[:, None, None]
    v = 0.2 + sum(0.6 * np.exp(-(x - c - d) ** 2 / (2 * P["sigma"] ** 2)) for c in P["centres"])
    v = np.ascontiguousarray(np.broadcast_to(v, (P["T"], P["H"], P["W"])))
    v.setflags(write=False)
    return v


def bar_amplitude(video):
    """the sinusoid-fit amplitude, at the clip's frequency and over its second half, of the sub-pixel position of the first bar's peak
    (the centroid of what rises above half height, in the left half of the frame)"""
    P = BARS
    prof = np.asarray(video, dtype=np.float64).mean(axis=1)[:, :P["W"] // 2]
    wgt = np.maximum(prof - 0.5, 0.0)
    pos = (wgt * np.arange(prof.shape[1])).sum(axis=1) / wgt.sum(axis=1)
    t = np.arange(P["T"] // 2, P["T"])
    ph = 2 * np.pi * P["f"] * t / P["fps"]
    G = np.stack([np.sin(ph), np.cos(ph), np.ones_like(ph)], axis=1)
    a, b, _ = np.linalg.lstsq(G, pos[t], rcond=None)[0]
    return float(np.hypot(a, b))


def purpose_criteria(out, who):
    v = bars_clip()
    gain = bar_amplitude(out) / bar_amplitude(v)
    lo, hi = float(out.min()), float(out.max())
    print("%s: the first bar moves %.2f x the input's (nominal %g), output range [%.3f, %.3f]" % (who, gain, 1 + BARS["amp"], lo, hi))
    assert gain >= 0.6 * (1 + BARS["amp"]), (who, gain)
    assert lo >= v.min() - 0.1 and hi <= v.max() + 0.1, (who, lo, hi)
    return gain, lo, hi


# ---- the case table ----------------------------------------------------------------------------------------------------------------
def _case(name, video, levels, skip, order=1, amp=20.0, blur=True):
    return dict(name=name, video=video, levels=levels, skip=skip, order=order, amp=amp, blur=blur)


SECTIONS_BLUR, SECTIONS_NO_BLUR = (5, 7, 8), (2, 4, 7)      # section counts of k_phase_time that the first table left out


def _cases():
    out = {}
    for skip in (0, 1):
        for order in (1, 3):
            for kind in ("u8", "u16", "f64"):
                c = _case("moving_37x45_skip%d_nsec%d_%s" % (skip, order, kind), ("moving", 12, 37, 45, kind), 4, skip, order)
                out[c["name"]] = c
    for order in (2, 4, 6):    # the other instances of the time kernel; 6: the run-time section count
        c = _case("moving_37x45_skip0_nsec%d_f64" % order, ("moving", 12, 37, 45, "f64"), 4, 0, order)
        out[c["name"]] = c
    for order in SECTIONS_BLUR:       # the rest of the run-time count: 8 never leaves the section loop early, 5 and 7 move the sine planes
        c = _case("moving_37x45_skip0_nsec%d_f64" % order, ("moving", 12, 37, 45, "f64"), 4, 0, order)
        out[c["name"]] = c
    for order in SECTIONS_NO_BLUR:
        c = _case("no_blur_nsec%d" % order, ("moving", 12, 37, 45, "f64"), 4, 0, order, blur=False)
        out[c["name"]] = c
    for name, shape, levels in (("tiny_5x7_levels3", (5, 7), 3), ("tiny_5x7_levels4", (5, 7), 4), ("row_1x9_levels2", (1, 9), 2),
                                ("column_9x1_levels2", (9, 1), 2)):
        out[name] = _case(name, ("moving", 12) + shape + ("f64",), levels, 0, 1)
    for kind in ("f64", "f32", "f16"):     # 71 x 130: three 64-column tiles and waves per row (the last partial), nine 8-row tiles
        out["wide_71x130_" + kind] = _case("wide_71x130_" + kind, ("moving", 5, 71, 130, kind), 3, 0, 2, amp=15.0)
    out["degenerate"] = _case("degenerate", ("degenerate",), 3, 0, 1)
    for T in (1, 2):
        out["moving_T%d" % T] = _case("moving_T%d" % T, ("moving", T, 37, 45, "u8"), 4, 0, 3)
    out["no_blur"] = _case("no_blur", ("moving", 12, 37, 45, "f64"), 4, 0, 1, blur=False)
    out["no_blur_nsec3_skip1"] = _case("no_blur_nsec3_skip1", ("moving", 12, 37, 45, "u16"), 4, 1, 3, blur=False)
    out["nothing_processed"] = _case("nothing_processed", ("moving", 12, 37, 45, "u16"), 4, 3, 1)
    out["one_level"] = _case("one_level", ("moving", 12, 37, 45, "f64"), 1, 0, 1)
    out["bars"] = _case("bars", ("bars",), BARS["levels"], 0, BARS["order"], BARS["amp"])
    return out


CASES = _cases()
REFERENCE_CASES = [n for n in CASES if n != "bars"]           # compared in float64 (the bars clip has its own check)
INTEGER_CASES = ["moving_37x45_skip%d_nsec%d_%s" % (s, o, k) for s in (0, 1) for o in (1, 3) for k in ("u8", "u16", "f64")]   # also with uint8 out
U16_OUT_CASES = ["moving_37x45_skip1_nsec3_f64", "no_blur"]      # float64 in: (k + 0.37) / 255 * 65535 = 257 k + 95.09
CAP_CASES = [(n, 255) for n in INTEGER_CASES if not n.endswith("_u8")] + [(n, 65535) for n in U16_OUT_CASES]


def video_of(case):
    v = case["video"]
    if v[0] == "moving":
        return moving(*v[1:])
    return degenerate_clip() if v[0] == "degenerate" else bars_clip()


def sos_of(case):
    band = BARS["band"] if case["name"] == "bars" else BAND
    return butter_sos(case["order"], band=band)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the unperturbed float64 output, D)"""
    c = CASES[name]
    v, sos = video_of(c), sos_of(c)
    ref = pr.phase_magnify(v, c["levels"], c["skip"], sos, c["amp"], c["blur"])
    D = max(float(np.abs(pr.phase_magnify(v, c["levels"], c["skip"], sos, c["amp"], c["blur"], perturb_seed=seed) - ref).max()) for seed in (11, 12, 13))
    ref.setflags(write=False)
    return ref, D


# ---- thin callers ---------------------------------------------------------------------------------------------------------------
class Phase:
    def __init__(self, be, H, W, levels, skip, sos, amp, flags=0):
        self.be = be
        self.sos = np.ascontiguousarray(sos, dtype=np.float64)
        self.h = ctypes.c_void_p()
        _capi.check(be.lib, be.lib.rm_phase_create(be.ctx, H, W, levels, skip, ctypes.c_void_p(self.sos.ctypes.data), self.sos.shape[0], float(amp),
                                                   flags, ctypes.byref(self.h)), "rm_phase_create")
        self.H, self.W = H, W

    def push_rc(self, frames_dev, dtype, n, out_dev, out_dtype):
        be = self.be
        return be.lib.rm_phase_push(be.ctx, self.h, be.p(frames_dev), dtype, n, be.p(out_dev), out_dtype, be.stream())

    def push(self, frames, out_dtype=_capi.RM_F64):
        be = self.be
        frames = np.ascontiguousarray(frames)
        d = be.dev(frames)
        out = be.full(frames.shape, OUT_NP[out_dtype], 0)
        _capi.check(be.lib, self.push_rc(d, DT[frames.dtype], frames.shape[0], out, out_dtype), "rm_phase_push")
        return be.np(out)

    def info(self):
        seen, n, b = ctypes.c_longlong(-1), ctypes.c_size_t(), ctypes.c_size_t()
        _capi.check(self.be.lib, self.be.lib.rm_phase_info(self.h, ctypes.byref(seen), ctypes.byref(n), ctypes.byref(b)), "rm_phase_info")
        return seen.value, n.value, b.value

    def reset(self):
        _capi.check(self.be.lib, self.be.lib.rm_phase_reset(self.be.ctx, self.h), "rm_phase_reset")

    def close(self):
        if self.h:
            self.be.lib.rm_phase_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def open_case(be, case):
    v = video_of(case)
    return Phase(be, v.shape[1], v.shape[2], case["levels"], case["skip"], sos_of(case), case["amp"], 0 if case["blur"] else _capi.RM_PHASE_NO_BLUR)


def run_case(be, name, out_dtype=_capi.RM_F64, T=None):
    c = CASES[name]
    v = video_of(c)
    with open_case(be, c) as ph:
        return ph.push(v if T is None else v[:T], out_dtype)


def processed_pixels(H, W, levels, skip):
    n = 0
    for l in range(levels):
        if skip <= l <= levels - 2:
            n += H * W
        H, W = (H + 1) // 2, (W + 1) // 2
    return n


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_float(got, ref, D, what):
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - ref).max())
    msg = "%s: max |error| %.3e, D %.3e (recorded %s), bound %.3e" % (what, err, D, RECORDED_D.get(what.split()[0]), FACTOR * D)
    print(msg)
    if D == 0:
        assert np.array_equal(got, ref), msg
    else:
        assert err <= FACTOR * D, msg


def near_integer(ref, D, scale):
    """where the reference's clamped m * scale lies within 64 D * scale of an integer"""
    m = np.clip(ref, 0.0, 1.0) * scale
    return np.abs(m - np.round(m)) <= FACTOR * D * scale


def check_integer(got, ref, D, scale, what):
    want = pr.to_uint(ref, scale)
    diff = got.astype(np.int64) - want.astype(np.int64)
    nd = int((diff != 0).sum())
    msg = "%s: %d of %d pixels differ, largest %d, D %.3e" % (what, nd, diff.size, int(np.abs(diff).max()), D)
    print(msg)
    assert np.abs(diff).max() <= 1, msg
    assert not np.any((diff != 0) & ~near_integer(ref, D, scale)), msg
    assert nd * 1000 <= diff.size, msg


def check_reference_case(be, name, T=None):
    """cases 1-4, 6, 7: float64 out against the reference (T: a shorter push, compared with the reference's first T frames -- the rule
    is causal)"""
    ref, D = reference(name)
    got = run_case(be, name, _capi.RM_F64, T)
    check_float(got, ref[:len(got)], D, name + " float64")


def check_integer_case(be, name, T=None):
    ref, D = reference(name)
    got = run_case(be, name, _capi.RM_U8, T)
    assert got.dtype == np.uint8
    check_integer(got, ref[:len(got)], D, 255, name + " uint8")


def check_reference_alone_meets_the_integer_cap():
    """no more than 1 pixel of 1000 of the reference lies on a truncation boundary, on the inputs chosen for that (uint16, float64)"""
    for name, scale in CAP_CASES:
        ref, D = reference(name)
        n = int(near_integer(ref, D, scale).sum())
        print("%s: %d of %d pixels within 64 D * %d of an integer (D %.3e)" % (name, n, ref.size, scale, D))
        assert D > 0 and n * 1000 <= ref.size, (name, scale, n, ref.size)


def check_u16_out(be):
    for name in U16_OUT_CASES:
        ref, D = reference(name)
        got = run_case(be, name, _capi.RM_U16)
        assert got.dtype == np.uint16
        check_integer(got, ref, D, 65535, name + " uint16")
        got32 = run_case(be, name, _capi.RM_F32)      # one rounding to float32 on top: half an ulp of float32
        assert got32.dtype == np.float32 and np.abs(got32.astype(np.float64) - ref).max() <= FACTOR * D + 2.0 ** -24 * np.abs(ref).max()


def check_first_frame(be, oracle):
    """case 4: T = 1 and T = 2; the first frame is, bit for bit, the oracle's collapse of its own pyramid"""
    for name in ("moving_T1", "moving_T2"):
        c = CASES[name]
        v = video_of(c)
        own = np.array(oracle.collapse_laplacian_video_pyramid(oracle.create_laplacian_video_pyramid(oracle.uint8_to_float(v[:1]), c["levels"])))
        ref, D = reference(name)
        assert np.array_equal(ref[:1], own)
        assert (D == 0) == (len(v) == 1), (name, D)
        got = run_case(be, name)
        assert np.array_equal(got[:1], own), name
        check_float(got, ref, D, name + " float64")
        got8 = run_case(be, name, _capi.RM_U8)
        assert np.array_equal(got8[:1], pr.to_uint(own, 255))
        if len(v) > 1:
            check_integer(got8[1:], ref[1:], D, 255, name + " uint8")


def check_degenerate(be):
    """case 3: hyp == 0, den == 0 and m == 0 occur (by the reference's own intermediate values) and the output stays finite"""
    c = CASES["degenerate"]
    v = video_of(c)
    from oracle import respmon_oracle as oracle
    lvl = oracle.create_laplacian_video_pyramid(np.array(v), c["levels"])[0]
    R1, R2 = pr.riesz(lvl[1])
    A = np.sqrt((lvl[1] * lvl[1] + R1 * R1) + R2 * R2)
    assert (A == 0).sum() > 200 and (pr.blur(A) == 0).sum() > 50 and (A > 0).sum() > 200
    ref, D = reference("degenerate")
    assert D > 0
    got = run_case(be, "degenerate")
    check_float(got, ref, D, "degenerate float64")
    assert np.array_equal(got[:, :, :8], np.zeros_like(got[:, :, :8]))


CHUNKINGS = ((1, 11), (5, 7), (1,) * 12)
CHUNK_CASES = (("moving_37x45_skip0_nsec3_u8", _capi.RM_F64), ("moving_37x45_skip1_nsec1_u16", _capi.RM_U8), ("no_blur", _capi.RM_F64),
               ("moving_37x45_skip0_nsec6_f64", _capi.RM_F64))
SECTION_CASES = ["moving_37x45_skip0_nsec%d_f64" % n for n in SECTIONS_BLUR] + ["no_blur_nsec%d" % n for n in SECTIONS_NO_BLUR]


def check_reference_alone_meets_the_float_cap(names=SECTION_CASES):
    """the 64 D rule tells a wrong tap, sign or order (1e-6) from rounding only while D stays near the rounding of the three functions:
    0 < D < 1e-13 on these inputs, by the reference alone"""
    for name in names:
        D = reference(name)[1]
        print("%s: D %.3e" % (name, D))
        assert 0 < D < 1e-13, (name, D)


def check_chunk_invariance(be, internal=False, cases=CHUNK_CASES):
    """case 5: every cut of the sequence gives the bits of one push; the frame counts agree; after reset the clip gives the same again"""
    for name, out_dtype in cases:
        c = CASES[name]
        v = video_of(c)
        with open_case(be, c) as ph:
            seen, NP, nbytes = ph.info()
            assert seen == 0 and NP == processed_pixels(v.shape[1], v.shape[2], c["levels"], c["skip"])
            assert nbytes == 8 * (5 + 4 * c["order"]) * NP
            whole = ph.push(v, out_dtype)
            assert ph.info()[0] == len(v)
            for cut in CHUNKINGS:
                ph.reset()
                assert ph.info()[0] == 0
                parts, k = [], 0
                for n in cut:
                    parts.append(ph.push(v[k:k + n], out_dtype))
                    k += n
                    assert ph.info()[0] == k
                assert np.array_equal(np.concatenate(parts), whole), (name, cut)
            if internal:      # the library's own split of a large push
                ph.reset()
                _capi.check(be.lib, be.lib.rm_debug_set(be.ctx, b"stream_frames", 5), "rm_debug_set")
                try:
                    assert np.array_equal(ph.push(v, out_dtype), whole), (name, "internal chunks")
                finally:
                    _capi.check(be.lib, be.lib.rm_debug_set(be.ctx, b"stream_frames", 0), "rm_debug_set")
            ph.reset()
            assert np.array_equal(ph.push(v, out_dtype), whole), (name, "after reset")
        with open_case(be, c) as ph2:      # a fresh object: nothing of the first one's state is left anywhere
            assert np.array_equal(ph2.push(v, out_dtype), whole)


def check_nothing_processed(be, oracle):
    """case 7: skip == levels - 1 (and a one-level pyramid): the converted collapse, bit for bit, and no state"""
    for name in ("nothing_processed", "one_level"):
        c = CASES[name]
        v = video_of(c)
        own = np.array(oracle.collapse_laplacian_video_pyramid(oracle.create_laplacian_video_pyramid(pr.to_float(v), c["levels"])))
        ref, D = reference(name)
        assert D == 0 and np.array_equal(ref, own)
        with open_case(be, c) as ph:
            assert ph.info()[1:] == (0, 0)
            assert np.array_equal(ph.push(v), own)
            assert np.array_equal(ph.push(v, _capi.RM_U8), pr.to_uint(own, 255))
            assert np.array_equal(ph.push(v, _capi.RM_U16), pr.to_uint(own, 65535))
            assert ph.info()[0] == 3 * len(v)


def check_purpose(be):
    """case 8: the build matches the reference on the bars clip and meets the two conditions the reference meets"""
    ref, D = reference("bars")
    got = run_case(be, "bars")
    check_float(got, ref, D, "bars float64")
    purpose_criteria(got, "library")


def check_argument_errors(be):
    """case 9: the documented code, and nothing written to out_dev"""
    E, U = _capi.RM_E_BADARG, _capi.RM_E_UNSUPPORTED
    lib = be.lib
    sos = butter_sos(2)
    sp = ctypes.c_void_p(sos.ctypes.data)
    h = ctypes.c_void_p()

    def create(ctx=be.ctx, H=8, W=9, levels=3, skip=0, sos_p=sp, nsec=2, flags=0, out=ctypes.byref(h)):
        return lib.rm_phase_create(ctx, H, W, levels, skip, sos_p, nsec, 10.0, flags, out)
    assert create(ctx=None) == E and create(sos_p=None) == E and create(out=None) == E
    assert create(nsec=0) == E and create(nsec=-1) == E
    nine = np.ascontiguousarray(np.tile(sos[:1], (9, 1)))
    assert create(sos_p=ctypes.c_void_p(nine.ctypes.data), nsec=9) == U
    assert not h
    assert create(sos_p=ctypes.c_void_p(nine.ctypes.data), nsec=8) == _capi.RM_OK and h
    lib.rm_phase_destroy(h)
    h = ctypes.c_void_p()
    bad = sos.copy()
    bad[1, 3] = 2.0
    assert create(sos_p=ctypes.c_void_p(bad.ctypes.data)) == E and b"a0" in lib.rm_last_error_string()
    assert create(H=0) == E and create(W=0) == E and create(levels=0) == E and create(skip=-1) == E and create(flags=2) == E
    assert not h
    assert lib.rm_phase_destroy(None) == _capi.RM_OK
    assert lib.rm_phase_info(None, None, None, None) == E and lib.rm_phase_reset(be.ctx, None) == E

    v = moving(4, 8, 9, "f64")
    with Phase(be, 8, 9, 3, 0, sos, 10.0) as ph:
        assert lib.rm_phase_reset(None, ph.h) == E
        d = be.dev(v)
        out = be.full(v.shape, np.float64, -7.0)
        F64, stream = _capi.RM_F64, be.stream()
        assert lib.rm_phase_push(None, ph.h, be.p(d), F64, 4, be.p(out), F64, stream) == E
        assert lib.rm_phase_push(be.ctx, None, be.p(d), F64, 4, be.p(out), F64, stream) == E
        assert lib.rm_phase_push(be.ctx, ph.h, None, F64, 4, be.p(out), F64, stream) == E
        assert lib.rm_phase_push(be.ctx, ph.h, be.p(d), F64, 4, None, F64, stream) == E
        assert ph.push_rc(d, F64, 0, out, F64) == E and ph.push_rc(d, F64, -1, out, F64) == E
        assert ph.push_rc(d, _capi.RM_BGR8, 1, out, F64) == U
        assert ph.push_rc(d, 5, 4, out, F64) == E and ph.push_rc(d, 99, 4, out, F64) == E
        for od in (_capi.RM_F16, _capi.RM_BGR8, 5, 99, -1):
            assert ph.push_rc(d, F64, 4, out, od) == E, od
        assert ph.push_rc(d, F64, 4, d, F64) == E and b"overlap" in lib.rm_last_error_string()
        assert ph.push_rc(d, F64, 3, d[1:], F64) == E                      # a partial overlap
        assert ph.push_rc(d, F64, 2, d[2:], F64) == _capi.RM_OK            # side by side is no overlap
        assert np.array_equal(be.np(out), np.full(v.shape, -7.0))           # none of the refusals wrote
        assert ph.info()[0] == 2
        # ... and the object still works: the refusals left its state alone
        ph.reset()
        got = ph.push(v)
        assert np.abs(got - pr.phase_magnify(v, 3, 0, sos, 10.0)).max() < 1e-9


def check_declared(lib):
    names = ["rm_phase_create", "rm_phase_destroy", "rm_phase_reset", "rm_phase_info", "rm_phase_push"]
    assert all(n in _capi.SIGNATURES for n in names) and all(hasattr(lib, n) for n in names)
    assert lib.rm_abi_version() == 1 and _capi.RM_PHASE_NO_BLUR == 1
