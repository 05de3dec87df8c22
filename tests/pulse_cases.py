"""Shared by tests/test_emu_pulse.py and tests/test_gpu_pulse.py (not a test module): the pulse path (include/respmon_hip.h
rm_bgr_block_sums / rm_bgr_roi_sums / rm_pulse_pos / rm_pulse_map) against tests/pulse_reference.py, thin callers of the C-ABI on raw
pointers, and the checks both builds run.  The backend `be` is the one of tests/rate_cases.py (lib, ctx, stream, p, out, out_i32, np)
with byte buffers for everything that is not float64:
    be.dev(a, offset=0) -> buffer     a device copy of the bytes of a contiguous array, starting `offset` bytes into its allocation
    be.fill(nbytes)     -> buffer     a result area of nbytes filled with SENTINEL
    be.get(buffer, dtype, shape)      the buffer's bytes as a host array
    be.other_stream()                 a stream handle that is not be.stream()

Integer sums are compared exactly.  POS is compared BIT FOR BIT with the scalar restatement: + - * / sqrt of float64 round once on both
sides and the rule fixes their order, so a differing bit is a finding about the kernel's order of operations.  The spectral stage is
rm_spectral_peak's and is judged by tests/rate_cases.py; here rm_pulse_map only has to equal its three parts bit for bit."""
import ctypes
import functools

import numpy as np

from respmon_amd import _capi, synth
from tests import pulse_reference as pr
from tests import rate_cases as rc

SENTINEL = 0xA5
B, U = _capi.RM_E_BADARG, _capi.RM_E_UNSUPPORTED
ENTRY_POINTS = ("rm_bgr_block_sums", "rm_bgr_roi_sums", "rm_pulse_pos", "rm_pulse_map")
assert all(name in _capi.SIGNATURES for name in ENTRY_POINTS), "the C-ABI does not declare the pulse entry points"


# ---- callers -------------------------------------------------------------------------------------------------------------------
def nblocks(H, W, block):
    return -(-H // block), -(-W // block)


def block_sums_rc(be, fd, N, H, W, block, out):
    return be.lib.rm_bgr_block_sums(be.ctx, be.p(fd) if fd is not None else None, N, H, W, block, be.p(out) if out is not None else None, be.stream())


def block_sums(be, frames, block, offset=0):
    frames = np.ascontiguousarray(frames)
    N, H, W = frames.shape[:3]
    hb, wb = nblocks(H, W, block)
    out = be.fill(4 * N * hb * wb * 3)
    _capi.check(be.lib, block_sums_rc(be, be.dev(frames, offset), N, H, W, block, out), "rm_bgr_block_sums")
    return be.get(out, np.uint32, (N, hb, wb, 3))


def roi_sums_rc(be, fd, N, H, W, rois, K, out):
    r = np.ascontiguousarray(rois, dtype=np.int32) if rois is not None else None
    return be.lib.rm_bgr_roi_sums(be.ctx, be.p(fd) if fd is not None else None, N, H, W, ctypes.c_void_p(r.ctypes.data) if r is not None else None, K,
                                  be.p(out) if out is not None else None, be.stream())


def roi_sums(be, frames, rois):
    frames = np.ascontiguousarray(frames)
    N, H, W = frames.shape[:3]
    out = be.fill(4 * N * len(rois) * 3)
    _capi.check(be.lib, roi_sums_rc(be, be.dev(frames), N, H, W, rois, len(rois), out), "rm_bgr_roi_sums")
    return be.get(out, np.uint32, (N, len(rois), 3))


def pos_rc(be, sd, N, NP, window, out, stream=None):
    return be.lib.rm_pulse_pos(be.ctx, be.p(sd) if sd is not None else None, N, NP, window, be.p(out) if out is not None else None,
                               be.stream() if stream is None else stream)


def pos(be, sums, window):
    s = np.ascontiguousarray(sums, dtype=np.uint32)
    N, NP = s.shape[:2]
    out = be.fill(8 * N * NP)
    _capi.check(be.lib, pos_rc(be, be.dev(s), N, NP, window, out), "rm_pulse_pos")
    return be.get(out, np.float64, (N, NP))


def pulse_map_rc(be, fd, N, H, W, block, window, fps, fmin, fmax, F, outs, stream=None):
    return be.lib.rm_pulse_map(be.ctx, be.p(fd) if fd is not None else None, N, H, W, block, window, fps, fmin, fmax, F, *outs.ptrs(),
                               be.stream() if stream is None else stream)


def pulse_map(be, frames, block, window, fps, fmin, fmax, F, want=(1, 1, 1, 1)):
    frames = np.ascontiguousarray(frames)
    N, H, W = frames.shape[:3]
    hb, wb = nblocks(H, W, block)
    outs = rc.Outs(be, hb * wb, want)
    _capi.check(be.lib, pulse_map_rc(be, be.dev(frames), N, H, W, block, window, fps, fmin, fmax, F, outs), "rm_pulse_map")
    return outs.np()


def untouched(be, buf):
    return bool((be.get(buf, np.uint8, (-1,)) == SENTINEL).all())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- case 1: block sums ---------------------------------------------------------------------------------------------------------
# the shapes of the issue, and two rows wider than one wave of 16-pixel groups (65 groups: a second workgroup column), one that takes
# the 16-byte loads (1040 = 16 * 65) and one that does not
SHAPES = ((1, 1), (3, 5), (16, 16), (17, 37), (33, 64), (40, 129), (5, 1040), (3, 1030))
BLOCKS = (4, 8, 16, 32, 64)       # every size pulse_block_ok takes: NB = 4, 2 and the fold over L = 1, 2, 4 lanes


@functools.lru_cache(maxsize=None)
def block_inputs(N, H, W):
    """(name, frames) pairs: random bytes, all 255 (the accumulators' upper bound), and three frames with one non-zero channel each (a
    channel-phase slip names itself at every x mod 4)"""
    rng = np.random.default_rng(1000 * H + W + N)
    one = np.zeros((3, H, W, 3), np.uint8)
    for c in range(3):
        one[c, :, :, c] = rng.integers(1, 256, (H, W))
    out = (("random", rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)), ("all255", np.full((N, H, W, 3), 255, np.uint8)), ("one_channel", one))
    for _, a in out:
        a.setflags(write=False)
    return out


def check_block_sums(be, H, W, block, N):
    for name, frames in block_inputs(N, H, W):
        got = block_sums(be, frames, block)
        want = pr.block_sums(frames, block)
        assert got.shape == want.shape and np.array_equal(got.astype(np.uint64), want), (H, W, block, N, name)


def check_block_sums_misaligned(be):
    """the frame tensor is a view starting 1 byte into its allocation: at (33, 64) the shape alone would take the 16-byte loads; at
    (17, 37) the rows are 111 bytes, so no row after the first is 16-byte aligned either way"""
    for H, W in ((33, 64), (17, 37)):
        for block in BLOCKS:
            frames = block_inputs(3, H, W)[0][1]
            assert np.array_equal(block_sums(be, frames, block, offset=1).astype(np.uint64), pr.block_sums(frames, block)), (H, W, block)


# ---- case 2: rectangle sums -----------------------------------------------------------------------------------------------------
def check_roi_sums(be):
    N, H, W = 3, 40, 129
    frames = block_inputs(N, H, W)[0][1]
    rois = [(0, 0, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, H), (10, 5, 70, 30), (40, 20, 80, 20), (40, 20, 80, 20), (16, 16, 16, 16), (128, 0, 1, 40),
            (0, 39, 129, 1)]
    got = roi_sums(be, frames, rois)
    assert np.array_equal(got.astype(np.uint64), pr.roi_sums(frames, rois))
    assert np.array_equal(got[:, 4], got[:, 5])                                      # a repeated rectangle
    assert np.array_equal(got[:, 6], block_sums(be, frames, 16)[:, 1, 1])           # a rectangle that coincides with a block
    assert np.array_equal(got[:, 2].astype(np.uint64), pr.block_sums(frames, 64).sum(axis=(1, 2)))
    # K = RM_MAX_ROIS, all 255: the upper bound of every sum
    rng = np.random.default_rng(5)
    many = []
    for _ in range(_capi.RM_MAX_ROIS):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        many.append((x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))))
    for f in (frames, block_inputs(N, H, W)[1][1]):
        assert np.array_equal(roi_sums(be, f, many).astype(np.uint64), pr.roi_sums(f, many))
    one = roi_sums(be, frames[:1], many[:1])
    assert one.shape == (1, 1, 3) and np.array_equal(one.astype(np.uint64), pr.roi_sums(frames[:1], many[:1]))


# ---- case 3: POS ----------------------------------------------------------------------------------------------------------------
POS_NS, POS_LS, POS_NPS, POS_NPMAX = (2, 9, 40), (2, 5, None), (1, 63, 65, 130), 130      # l = None: the whole clip, l = N


@functools.lru_cache(maxsize=None)
def pos_inputs(N, l):
    """uint32 [N, 130, 3] in the range a 16 x 16 block gives (<= 65 280), shaped like what a block of a scene gives: a level per column
    and channel, an intensity change common to the channels (2 %), a chrominance change along one direction per column (the pulse's
    place: 1 - 1.5 %, alternating in sign from frame to frame so that no window, not even one of two frames, is flat), and a count of
    sensor noise.  Independent noise per channel would not do for the comparison with the textbook form: a = |S1| / |S2| of a
    two-frame window is then a ratio of two independent variables, heavy-tailed, and both forms carry a rounding error of about
    8 u (1 + a) in h -- the 1e-12 agreement would then measure the inputs' conditioning, not the forms.  Here S2's swing is at least
    0.2 * 0.02 per window against 1e-4 of noise, so a stays below 10 (check_pos_reference_properties asserts it).
    Column 0 is such a column (NP = 1 must not be a degenerate one); column 1 is constant in time (v2 = 0 -> a = 0 ->
    H == 0.0); column 2 has a zero channel throughout (every window skipped, H == 0.0); column 3 goes black for l - 1 frames -- a
    stretch shorter than l, so every window still holds a lit frame and none is skipped, while its x are 0 inside the stretch; column 4
    goes black for l + 2 frames from frame 2 on where the clip has room (N >= l + 6: two lit frames either side, a window with one lit
    frame has x = l in every channel and projects to 0), so the windows inside the stretch ARE skipped and the others are not."""
    rng = np.random.default_rng(100 * N + l)
    level = rng.integers(8000, 50000, (1, POS_NPMAX, 3)).astype(np.float64)
    inten = 0.02 * rng.standard_normal((N, POS_NPMAX, 1))
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None, None]
    m = 0.01 * sign * (1 + 0.5 * rng.random((N, POS_NPMAX, 1)))
    d = np.stack([rng.uniform(0.4, 0.7, POS_NPMAX), rng.uniform(0.6, 1.0, POS_NPMAX), rng.uniform(0.2, 0.4, POS_NPMAX)], axis=-1)[None]   # B, G, R
    s = np.rint(level * (1 + inten + d * m) + rng.standard_normal((N, POS_NPMAX, 3))).astype(np.uint32)
    assert s.max() <= 65280
    s[:, 1] = s[0, 1]
    s[:, 2, int(rng.integers(0, 3))] = 0
    a = N // 3
    s[a:a + l - 1, 3] = 0
    if N >= l + 6:
        s[2:l + 4, 4] = 0
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _pos_reference(N, l):
    alphas = []
    H = pr.pos_scalar(pos_inputs(N, l), l, alphas)
    H.setflags(write=False)
    return H, max(alphas)


def pos_reference(N, l):
    return _pos_reference(N, l)[0]


def pos_cases():
    """(N, l): N of POS_NS, l of {2, 5, N}, without l > N"""
    return [(N, l) for N in POS_NS for l in sorted({N if l is None else l for l in POS_LS}) if l <= N]


def check_pos_reference_properties(N, l):
    """what the special columns are there for, by the reference alone"""
    s, (H, a_max) = pos_inputs(N, l), _pos_reference(N, l)
    assert a_max < 10, a_max
    assert N == 2 or np.abs(H[:, 0]).max() > 1e-4
    assert not H[:, 1].any() and not H[:, 2].any() and not np.signbit(H[:, 1:3]).any()
    if N > 2:           # (at N = l = 2 the one lit frame of column 3 has x = 2 in every channel: S1 = S2 = 0)
        assert H[:, 3].any()
    if N >= l + 6:
        skipped = [n for n in range(N - l + 1) if not s[n:n + l, 4].any()]
        assert skipped and len(skipped) < N - l + 1 and H[:, 4].any()


def check_pos(be, N, l):
    s, want = pos_inputs(N, l), pos_reference(N, l)
    for n in POS_NPS:
        got = pos(be, s[:, :n], l)
        assert same_bits(got, want[:, :n]), (N, l, n, float(np.abs(got - want[:, :n]).max()))


# ---- case 4: rm_pulse_map equals its three parts ------------------------------------------------------------------------------------
MAP_BAND = dict(fps=20.0, fmin=0.7, fmax=3.0, F=17)
MAP_GEOMS = ((17, 37, 4), (40, 129, 16), (33, 64, 8), (40, 129, 32))


@functools.lru_cache(maxsize=None)
def map_clip(N, H, W):
    """a textured BGR clip whose brightness and colour move in time, with sensor noise"""
    rng = np.random.default_rng(H + W)
    base = rng.integers(40, 200, (1, H, W, 3)).astype(np.float64)
    t = np.arange(N)[:, None, None, None]
    gain = 1 + 0.05 * np.sin(2 * np.pi * 1.3 * t / MAP_BAND["fps"]) * np.array([0.5, 0.8, 0.3])[None, None, None, :]
    clip = np.clip(np.rint(base * gain + rng.standard_normal((N, H, W, 3))), 0, 255).astype(np.uint8)
    clip.setflags(write=False)
    return clip


def check_map_equals_parts(be, geom, N, window=5):
    H, W, block = geom
    kw = MAP_BAND
    frames = map_clip(16, H, W)[:N]
    got = pulse_map(be, frames, block, window, kw["fps"], kw["fmin"], kw["fmax"], kw["F"])
    sums = block_sums(be, frames, block)
    h = pos(be, sums.reshape(N, -1, 3), window)
    want = rc.peak(be, h, kw["fps"], kw["fmin"], kw["fmax"], kw["F"])
    rc.same_outputs(got, want, (geom, N))
    assert (got[3] >= 0).any(), (geom, N)
    for m in (1, 6, 8):           # NULL outputs: what is asked for is what the full call gave
        w = tuple((m >> k) & 1 for k in range(4))
        part = pulse_map(be, frames, block, window, kw["fps"], kw["fmin"], kw["fmax"], kw["F"], w)
        for k in range(4):
            assert (part[k] is None) == (not w[k])
            if w[k]:
                assert np.array_equal(part[k], got[k], equal_nan=(k < 3)), (geom, N, w, k)


# ---- case 5: the purpose ------------------------------------------------------------------------------------------------------------
PURPOSE = dict(N=256, H=64, W=64, fps=20.0, block=16, window=32, fmin=0.7, fmax=3.0, F=64, pulse_hz=1.25, flicker_hz=0.9, skin_rect=(0, 0, 32, 64))
PURPOSE_SEEDS = (0, 3)
STEP = (PURPOSE["fmax"] - PURPOSE["fmin"]) / (PURPOSE["F"] - 1)


@functools.lru_cache(maxsize=None)
def purpose_clip(seed):
    P = PURPOSE
    clip = synth.synth_pulse_bgr(P["N"], P["H"], P["W"], fps=P["fps"], seed=seed)
    clip.setflags(write=False)
    return clip


def purpose_criteria(freq, periodicity, green_freq, tag):
    """(a) every skin block within one step of the pulse, (b) the green sums of the same blocks within one step of the lamp's flicker
    -- the contrast without which (a) shows nothing --, (c) the least periodic skin block beats the most periodic background block.
    freq, periodicity: [4, 4] over the blocks; green_freq: [8] over the skin blocks (block columns 0 and 1)."""
    P = PURPOSE
    assert abs(STEP - 0.0365) < 1e-4
    skin_f, skin_p, bg_p = freq[:, :2], periodicity[:, :2], periodicity[:, 2:]
    assert np.all(np.abs(skin_f - P["pulse_hz"]) <= STEP), (tag, "skin", skin_f)
    assert np.all(np.abs(green_freq - P["flicker_hz"]) <= STEP), (tag, "green", green_freq)
    assert skin_p.min() > bg_p.max(), (tag, "periodicity", float(skin_p.min()), float(bg_p.max()))
    return dict(skin_freq=(float(skin_f.min()), float(skin_f.max())), green_freq=(float(green_freq.min()), float(green_freq.max())),
                skin_periodicity=(float(skin_p.min()), float(skin_p.max())), background_periodicity=float(bg_p.max()))


def purpose_reference(seed):
    """the criteria by the references alone: numpy block sums, scalar POS, the long-double estimator of tests/rate_cases.py"""
    P = PURPOSE
    sums = pr.block_sums(purpose_clip(seed), P["block"])
    h = pr.pos_scalar(sums.reshape(P["N"], -1, 3), P["window"])
    r = rc.Ref(h, P["fps"], P["fmin"], P["fmax"], P["F"])
    per = (r.P.max(axis=0) / r.total).astype(np.float64).reshape(4, 4)
    g = rc.Ref(sums[:, :, :2, 1].reshape(P["N"], -1).astype(np.float64), P["fps"], P["fmin"], P["fmax"], P["F"])
    return purpose_criteria(r.freq.astype(np.float64).reshape(4, 4), per, g.freq.astype(np.float64), ("reference", seed))


def check_purpose(be, seed):
    P = PURPOSE
    clip = purpose_clip(seed)
    freq, power, total, index = pulse_map(be, clip, P["block"], P["window"], P["fps"], P["fmin"], P["fmax"], P["F"])
    assert np.all(index >= 0)
    green = block_sums(be, clip, P["block"])[:, :, :2, 1].reshape(P["N"], -1).astype(np.float64)
    gf = rc.peak(be, green, P["fps"], P["fmin"], P["fmax"], P["F"])[0]
    return purpose_criteria(freq.reshape(4, 4), (power / total).reshape(4, 4), gf, ("library", seed))


# ---- case 6: arguments ----------------------------------------------------------------------------------------------------------
def check_argument_errors(be):
    lib = be.lib
    N, H, W = 3, 17, 37
    frames = be.dev(np.ascontiguousarray(block_inputs(N, H, W)[0][1]))

    def refused(fn, code, what, nbytes=4096):
        out = be.fill(nbytes)
        assert fn(out) == code, what
        assert untouched(be, out), what

    # rm_bgr_block_sums
    for blk in (0, 1, 3, 5, 12, 24, 128, -16):
        refused(lambda o: block_sums_rc(be, frames, N, H, W, blk, o), B, ("block", blk))
    for n, h, w in ((0, H, W), (-1, H, W), (N, 0, W), (N, H, 0), (N, -3, W)):
        refused(lambda o: block_sums_rc(be, frames, n, h, w, 16, o), B, (n, h, w))
    refused(lambda o: block_sums_rc(be, None, N, H, W, 16, o), B, "NULL frames")
    assert block_sums_rc(be, frames, N, H, W, 16, None) == B
    assert lib.rm_bgr_block_sums(None, be.p(frames), N, H, W, 16, be.p(be.fill(64)), be.stream()) == B
    # rm_bgr_roi_sums
    ok = (1, 2, 5, 6)
    for bad in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -2, 4), (30, 0, 8, 4), (0, 10, 4, 8), (W, 0, 1, 1), (0, H, 1, 1),
                (0, 0, W + 1, H), (1, 0, 2 ** 31 - 1, 1)):
        refused(lambda o: roi_sums_rc(be, frames, N, H, W, [ok, bad], 2, o), B, bad)
        refused(lambda o: roi_sums_rc(be, frames, N, H, W, [bad], 1, o), B, bad)
    many = [ok] * (_capi.RM_MAX_ROIS + 1)
    for k in (0, -1, _capi.RM_MAX_ROIS + 1):
        refused(lambda o: roi_sums_rc(be, frames, N, H, W, many, k, o), B, ("K", k))
    for n in (0, -2):
        refused(lambda o: roi_sums_rc(be, frames, n, H, W, [ok], 1, o), B, ("N", n))
    refused(lambda o: roi_sums_rc(be, None, N, H, W, [ok], 1, o), B, "NULL frames")
    refused(lambda o: roi_sums_rc(be, frames, N, H, W, None, 1, o), B, "NULL rectangles")
    assert roi_sums_rc(be, frames, N, H, W, [ok], 1, None) == B
    # (refused before anything is read: the frame of this call exists only as its two sizes)
    refused(lambda o: roi_sums_rc(be, frames, 1, 5000, 5000, [ok, (0, 0, 5000, 5000)], 2, o), U, "w * h * 255 >= 2^32")
    refused(lambda o: roi_sums_rc(be, frames, 1, 4105, 4104, [(0, 0, 4104, 4105)], 1, o), U, "w * h * 255 >= 2^32, barely")
    # rm_pulse_pos
    Np, NP = 9, 20
    s = be.dev(np.ascontiguousarray(pos_inputs(9, 5)[:, :NP]))
    for n, l in ((1, 1), (1, 2), (0, 2), (Np, 1), (Np, 0), (Np, -5), (Np, Np + 1), (2, 3)):
        refused(lambda o: pos_rc(be, s, n, NP, l, o), B, ("N, window", n, l))
    refused(lambda o: pos_rc(be, s, 4097, NP, 5, o), U, "N > 4096")
    refused(lambda o: pos_rc(be, None, Np, NP, 5, o), B, "NULL sums")
    assert pos_rc(be, s, Np, NP, 5, None) == B
    refused(lambda o: 0 if pos_rc(be, s, Np, 0, 5, o) == _capi.RM_OK else -99, 0, "NP == 0 is an empty call")
    # rm_pulse_map
    kw = MAP_BAND
    fps, fmin, fmax, F = kw["fps"], kw["fmin"], kw["fmax"], kw["F"]
    nan = float("nan")

    def map_refused(code, what, fd=frames, n=N, h=H, w=W, block=4, window=2, band=(fps, fmin, fmax), f=F):
        outs = rc.Outs(be, 4096)
        assert pulse_map_rc(be, fd, n, h, w, block, window, band[0], band[1], band[2], f, outs) == code, what
        assert outs.untouched(), what

    for blk in (0, 3, 12, 128):
        map_refused(B, ("block", blk), block=blk)
    for l in (1, 0, -1, N + 1):
        map_refused(B, ("window", l), window=l)
    for n in (1, 0):
        map_refused(B, ("N", n), n=n, window=2)
    map_refused(U, "N > 4096", n=4097, window=5)
    for f in (2, 65, 0):
        map_refused(B, ("nfreq", f), f=f)
    for b in ((fps, 0.0, fmax), (fps, -0.1, fmax), (fps, fmax, fmax), (fps, fmax, fmin), (fps, fmin, fps / 2 + 1e-9), (0.0, fmin, fmax), (nan, fmin, fmax),
              (fps, nan, fmax), (fps, fmin, nan)):
        map_refused(B, b, band=b)
    map_refused(B, "NULL frames", fd=None)
    map_refused(B, "H < 1", h=0)
    map_refused(B, "W < 1", w=0)
    assert lib.rm_pulse_map(be.ctx, be.p(frames), N, H, W, 4, 2, fps, fmin, fmax, F, None, None, None, None, be.stream()) == B
    assert lib.rm_pulse_map(None, be.p(frames), N, H, W, 4, 2, fps, fmin, fmax, F, None, None, None, None, be.stream()) == B
    outs = rc.Outs(be, 5 * 10)
    assert pulse_map_rc(be, frames, N, H, W, 4, 2, fps, fmin, fmax, F, outs) == _capi.RM_OK and not outs.untouched()


def check_busy(be):
    """rm_pulse_pos and rm_pulse_map keep intermediates in the context's workspace: with a rm_locate_submit in flight they take work on
    its stream only (RM_E_BUSY elsewhere, nothing written); the two sum entry points use no workspace and are not concerned"""
    N, H, W = 3, 17, 37
    frames = be.dev(np.ascontiguousarray(block_inputs(N, H, W)[0][1]))
    s = be.dev(np.ascontiguousarray(pos_inputs(9, 5)[:, :20]))
    gray = be.dev(synth.synth_breathing(33, 40, 64, seed=2))
    kw = MAP_BAND
    tk, xywh = ctypes.c_int(-1), np.zeros(4, np.int32)
    side = be.other_stream()
    _capi.check(be.lib, be.lib.rm_locate_submit(be.ctx, be.p(gray), _capi.RM_U8, 33, 40, 64, 10.0, 0.1, 1.0, 500.0, 4, 2, 0.7, 20, 0, be.stream(),
                                                ctypes.byref(tk)), "rm_locate_submit")
    out, outs = be.fill(8 * 9 * 20), rc.Outs(be, 50)
    rc1 = pos_rc(be, s, 9, 20, 5, out, stream=side)
    msg1 = be.lib.rm_last_error_string()
    rc2 = pulse_map_rc(be, frames, N, H, W, 4, 2, kw["fps"], kw["fmin"], kw["fmax"], kw["F"], outs, stream=side)
    rc3 = pos_rc(be, s, 9, 20, 5, out)                 # the submission's own stream: taken
    _capi.check(be.lib, be.lib.rm_locate_result(be.ctx, tk.value, ctypes.c_void_p(xywh.ctypes.data)), "rm_locate_result")
    assert rc1 == _capi.RM_E_BUSY and b"in flight" in msg1 and rc2 == _capi.RM_E_BUSY and outs.untouched()
    assert rc3 == _capi.RM_OK and same_bits(be.get(out, np.float64, (9, 20)), pos_reference(9, 5)[:, :20])
