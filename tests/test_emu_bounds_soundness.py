"""Tile-bound soundness at extreme magnitudes, on the host-emulated build (tests/emu): the twin of test_gpu_bounds_soundness.py
at shapes the emulation runs quickly.  Every bound producer's bounds must contain every full-resolution value of their pair, be
neither NaN nor infinite while those values are finite, and leave the heatmap and extrema of the exhaustive evaluation unchanged
by a bit -- from amplification 1e-300 to 1e300, where the float32 level-1 bounds used to overflow and prune every pair."""
import numpy as np
import pytest

from tests import bounds_soundness as bs


class EmuRunner:
    def __init__(self, emu):
        self.e = emu

    def calibrate(self, v, amp, L, S, flags):
        heat, mm = self.e.calibrate(v, 10.0, amp=amp, levels=L, skip=S, flags=flags)
        return heat, (float(mm[0]), float(mm[1]))

    def set(self, key, value):
        self.e.debug_set(key, value)

    def workspace(self, name, shape):
        return self.e.workspace(name, shape)

    def kept(self):
        return self.e.counters()[2]

    def locate(self, v, amp, L, S):
        return self.e.locate(v, 10.0, amp=amp, levels=L, skip=S)


@pytest.fixture(scope="module")
def r():
    from tests.emu_harness import Emu
    return EmuRunner(Emu())


def test_emu_float32_level1_bounds_at_1e38(r, oracle):
    """the issue's case: 360 x 640, skip 2, default flags (the separate k_frame_bounds_l1f kernel).  At amplification 1e38 the float32
    intermediates (up to 64 max|C_2|) overflowed, top_ub became NaN and every pair was pruned."""
    v = np.random.default_rng(5).random((4, 360, 640))
    bs.run_case(r, oracle, v, 1e38, 4, 2, "360x640", prods=[({}, 0, "default")], sums=False)


def test_emu_bounds_sound_every_producer(r, oracle):
    """every producer of every skip, ragged widths (not a multiple of 16 or 64), a level 2 only two pixels high, at ordinary and
    extreme magnitudes"""
    rng = np.random.default_rng(7)
    for (T, H, W, L, S, amps) in [(4, 70, 200, 4, 2, (500.0, 1e38, -1e300)), (3, 7, 131, 4, 2, (3e37, -1e39)),
                                  (3, 40, 150, 3, 1, (1e40,)), (3, 67, 131, 5, 3, (-1e38, 1e-300)), (3, 48, 200, 6, 4, (1e300,))]:
        v = rng.random((T, H, W))
        v[:, : H // 2, : W // 3] *= 0.05
        for amp in amps:
            bs.run_case(r, oracle, v, amp, L, S, "ragged", sums=amp == amps[0])


def test_emu_magnitude_ladder(r, oracle):
    """amplification over the whole ladder, both signs, the float32 level-1 bounds (flags 512) and the default path, one buffer
    dtype per rung; float64 buffers scaled by 1e+-200 where the oracle's raw stays finite"""
    rng = np.random.default_rng(11)
    base = rng.random((4, 40, 140))
    base[:, :20, :50] *= 0.05
    prods = [({}, 0, "default"), ({}, bs.FLAG_FF_PER_LEVEL, "k_frame_bounds_l1f")]
    kinds = ["f64", "f32", "f16", "u8", "bgr8"]
    for n, amp in enumerate(bs.LADDER):
        for sign in (1, -1):
            v = bs.to_dtype(base, kinds[n % len(kinds)])
            bs.run_case(r, oracle, v, sign * amp, 4, 2, kinds[n % len(kinds)], prods=prods, sums=False)
    for scale, amp in [(1e200, 1e100), (1e200, -1e-30), (1e-200, 1e-100), (1e-200, 1e38)]:
        bs.run_case(r, oracle, base * scale, amp, 4, 2, "scaled %g" % scale, prods=prods, sums=False)


def test_emu_special_frames(r, oracle):
    """mixed scale (neighbouring tiles at 1e30 and 1e-30), one hot pixel of 1e35 in a quiet stream, constant frames (raw all +-0)"""
    rng = np.random.default_rng(13)
    for v, amp, what in [(bs.mixed_scale(rng, 4, 48, 260), 500.0, "mixed scale"), (bs.mixed_scale(rng, 3, 40, 200), 1e8, "mixed scale x1e8"),
                         (bs.hot_pixel(rng, 4, 40, 200), 500.0, "hot pixel"), (np.full((4, 40, 200), 0.25), 500.0, "constant"),
                         (np.zeros((3, 40, 200)), -1e38, "zero")]:
        bs.run_case(r, oracle, v, amp, 4, 2, what)
    for v, amp, what in [(bs.mixed_scale(rng, 3, 67, 131), 500.0, "mixed scale"), (bs.hot_pixel(rng, 3, 67, 131), 1e3, "hot pixel")]:
        bs.run_case(r, oracle, v, amp, 5, 3, what, sums=False)


def test_emu_non_finite_frames(r, oracle):
    """one NaN and one +inf pixel in f64 / f32 / f16 buffers: every producer and every sum path -- the default, the dense and
    store-based sums, the tiny store, k_dense_sum_t -- equals the exhaustive evaluation bit for bit (NaN where it is NaN).  (The
    selection finds no finite threshold here and prunes nothing, so the automatic choice takes the dense sum.)  locate(): the NaN
    reaches the oracle's raw.min(), every heatmap pixel of the oracle is NaN and it finds no contour (None) -- so must the library."""
    rng = np.random.default_rng(17)
    base = rng.random((5, 40, 140))
    for kind in ("f64", "f32", "f16"):
        v = bs.with_non_finite(base, kind)
        for S, L in ((2, 4), (3, 5)):
            bs.run_case(r, oracle, v, 500.0, L, S, "non-finite " + kind, sound=False)
        ref = oracle.locate(v.astype(np.float64), 10, pyramid_levels=4, skip_levels_at_top=2)
        assert ref is None, ref
        assert r.locate(v, 500.0, 4, 2) is None, kind


def test_emu_locate_at_extreme_amplification(r, oracle):
    """locate() against the oracle where the float32 bounds overflowed"""
    from respmon_amd import synth
    frames = oracle.uint8_to_float(synth.synth_breathing(16, 64, 160, seed=3))
    for amp in (1e38, -1e300, 1e-300):
        got = r.locate(frames, amp, 4, 2)
        assert got == oracle.locate(frames, 10, amplification=amp, pyramid_levels=4, skip_levels_at_top=2), amp


def test_emu_history_independence(r, oracle):
    """one context, a mixed sequence of calls: each heatmap bit-identical to a fresh context's (a plan's level-1 flag, the state and
    the bounds of one call must not leak into the next)"""
    from tests.emu_harness import Emu
    rng = np.random.default_rng(19)
    a = rng.random((4, 70, 200)); a[:, :30] *= 0.05
    dense = rng.random((4, 67, 131))
    seq = [(a, 1e38, 4, 2, 0), (dense, 500.0, 5, 3, 0), (a, 500.0, 4, 2, 0), (dense, 500.0, 6, 4, 0), (a, -1e40, 4, 2, bs.FLAG_FF_PER_LEVEL),
           (dense, 1e38, 5, 3, 0), (a, 500.0, 4, 2, bs.FLAG_FF_PER_LEVEL), (dense, 500.0, 3, 1, 0)]
    got = [r.calibrate(v, amp, L, S, fl) for (v, amp, L, S, fl) in seq]
    for (v, amp, L, S, fl), (heat, mm) in zip(seq, got):
        fresh = EmuRunner(Emu())
        want, mm2 = fresh.calibrate(v, amp, L, S, fl)
        assert bs.same(heat, want) and bs.same_mm(mm, mm2), (amp, L, S, fl)
