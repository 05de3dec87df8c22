"""Tile-bound soundness at extreme magnitudes on the MI355X (tests/bounds_soundness.py; the emulated twin is
test_emu_bounds_soundness.py).  Every bound producer's bounds must contain every full-resolution value of their pair, be neither NaN
nor infinite while those values are finite, and leave the heatmap and extrema of the exhaustive evaluation unchanged by a bit --
from amplification 1e-300 to 1e300, where the float32 level-1 bounds (k_frame_bounds_l1f) used to overflow and prune every pair."""
import numpy as np
import pytest

from tests import bounds_soundness as bs


@pytest.fixture(scope="module")
def r():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from respmon_amd import _capi
    _capi.load()   # raises if the HIP extension is missing: no fallback
    return GpuRunner()


class GpuRunner:
    def calibrate(self, v, amp, L, S, flags):
        import torch
        from respmon_amd import dist
        buf = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        heat, mm = dist.hip_calibrate(buf, 10, amplification=amp, pyramid_levels=L, skip_levels_at_top=S, flags=flags, return_minmax=True)
        return heat.cpu().numpy(), (float(mm[0]), float(mm[1]))

    def set(self, key, value):
        from respmon_amd import device
        device.debug_set(key, value)

    def workspace(self, name, shape):
        from respmon_amd import device
        return device.debug_workspace(name, shape)

    def kept(self):
        from respmon_amd import device
        return device.debug_counters()[2]

    def locate(self, v, amp, L, S):
        import torch
        from respmon_amd.base import RespiratoryMonitor
        return RespiratoryMonitor.locate(torch.from_numpy(np.ascontiguousarray(v)).cuda(), 10, amplification=amp, pyramid_levels=L,
                                         skip_levels_at_top=S)


@pytest.mark.gpu
def test_float32_level1_bounds_at_extreme_magnitudes(r, oracle):
    """shapes that take the separate bounds kernels by default (360 x 640, 720p, 4K wide with few frames): k_frame_bounds_l1f at
    amplification 1e38 overflowed float32, top_ub became NaN and every pair was pruned"""
    rng = np.random.default_rng(5)
    for (T, H, W, amps) in [(4, 360, 640, (500.0, 1e38, -1e40, 1e300)), (6, 720, 1280, (3e37, -1e39)), (3, 270, 3840, (1e38, 1e-300))]:
        v = rng.random((T, H, W))
        v[:, : H // 2, : W // 3] *= 0.05
        for amp in amps:
            bs.run_case(r, oracle, v, amp, 4, 2, "default geometry", prods=[({}, 0, "default"), ({}, bs.FLAG_FF_PER_LEVEL, "k_frame_bounds_l1f")],
                        sums=amp == amps[0])


@pytest.mark.gpu
def test_bounds_sound_every_producer(r, oracle):
    """every producer of every skip, ragged widths, a level 2 only two pixels high, ordinary and extreme magnitudes"""
    rng = np.random.default_rng(7)
    for (T, H, W, L, S, amps) in [(4, 70, 200, 4, 2, (500.0, 1e38, -1e300)), (3, 7, 131, 4, 2, (3e37, -1e39)), (5, 203, 1100, 5, 2, (1e40, -500.0)),
                                  (3, 40, 150, 3, 1, (1e40, -1e-30)), (3, 67, 131, 5, 3, (-1e38, 1e-300)), (4, 300, 2000, 6, 3, (1e100,)),
                                  (3, 48, 200, 6, 4, (1e300, 500.0)), (5, 270, 480, 7, 4, (-1e38,))]:
        v = rng.random((T, H, W))
        v[:, : H // 2, : W // 3] *= 0.05
        for amp in amps:
            bs.run_case(r, oracle, v, amp, L, S, "ragged", sums=True)


@pytest.mark.gpu
def test_magnitude_ladder_every_dtype(r, oracle):
    """the whole ladder, both signs, through every buffer dtype; float64 buffers scaled by 1e+-200 where the oracle's raw stays finite"""
    rng = np.random.default_rng(11)
    base = rng.random((6, 90, 330))
    base[:, :40, :120] *= 0.05
    prods = [({}, 0, "default"), ({}, bs.FLAG_FF_PER_LEVEL, "k_frame_bounds_l1f"), (dict(bounds_l1=0, bounds_scalar=2), bs.FLAG_FF_PER_LEVEL, "level-2")]
    for kind in ("f64", "f32", "f16", "u8", "bgr8"):
        v = bs.to_dtype(base, kind)
        for amp in bs.LADDER:
            for sign in (1, -1):
                bs.run_case(r, oracle, v, sign * amp, 4, 2, kind, prods=prods, sums=kind == "f64")
    for scale, amp in [(1e200, 1e100), (1e200, -1e-30), (1e-200, 1e-100), (1e-200, 1e38), (1e200, 1e-300)]:
        bs.run_case(r, oracle, base * scale, amp, 4, 2, "scaled %g" % scale, prods=prods)
        bs.run_case(r, oracle, base * scale, amp, 6, 4, "scaled %g" % scale)


@pytest.mark.gpu
def test_special_frames(r, oracle):
    """mixed scale (neighbouring tiles at 1e30 and 1e-30), one hot pixel of 1e35 in a quiet stream, constant frames (raw all +-0)"""
    rng = np.random.default_rng(13)
    for (T, H, W, L, S) in [(4, 48, 260, 4, 2), (4, 360, 640, 4, 2), (3, 67, 131, 5, 3), (4, 135, 240, 6, 4)]:
        for v, amp, what in [(bs.mixed_scale(rng, T, H, W), 500.0, "mixed scale"), (bs.mixed_scale(rng, T, H, W), 1e8, "mixed scale x1e8"),
                             (bs.hot_pixel(rng, T, H, W), 500.0, "hot pixel"), (np.full((T, H, W), 0.25), 500.0, "constant"),
                             (np.zeros((T, H, W)), -1e38, "zero")]:
            bs.run_case(r, oracle, v, amp, L, S, what)


@pytest.mark.gpu
def test_non_finite_frames(r, oracle):
    """one NaN and one +inf pixel in f64 / f32 / f16 buffers: every producer and every sum path -- the default, the dense and
    store-based sums, the tiny store, k_dense_sum_t -- equals the exhaustive evaluation bit for bit (NaN where it is NaN).  (The
    selection finds no finite threshold here and prunes nothing, so the automatic choice takes the dense sum.)  locate(): the NaN
    reaches the oracle's raw.min(), every heatmap pixel of the oracle is NaN and it finds no contour (None) -- so must the library."""
    rng = np.random.default_rng(17)
    base = rng.random((5, 40, 140))
    for kind in ("f64", "f32", "f16"):
        v = bs.with_non_finite(base, kind)
        for S, L in ((2, 4), (3, 5), (4, 6)):
            bs.run_case(r, oracle, v, 500.0, L, S, "non-finite " + kind, sound=False)
        ref = oracle.locate(v.astype(np.float64), 10, pyramid_levels=4, skip_levels_at_top=2)
        assert ref is None, ref
        assert r.locate(v, 500.0, 4, 2) is None, kind


@pytest.mark.gpu
def test_locate_at_extreme_amplification(r, oracle):
    """locate() against the oracle where the float32 bounds overflowed"""
    from respmon_amd import synth
    for (T, H, W, L, S) in [(32, 360, 640, 4, 2), (16, 64, 160, 5, 3)]:
        frames = oracle.uint8_to_float(synth.synth_breathing(T, H, W, seed=3))
        for amp in (1e38, -1e300, 1e-300, 1e300):
            got = r.locate(frames, amp, L, S)
            assert got == oracle.locate(frames, 10, amplification=amp, pyramid_levels=L, skip_levels_at_top=S), (T, H, W, amp)


def _fresh_calibrate(v, amp, L, S, flags):
    """rm_calibrate on a context of its own, created for this call and destroyed after it"""
    import ctypes
    import torch
    from respmon_amd import _capi, device
    lib = _capi.load()
    h = ctypes.c_void_p()
    _capi.check(lib, lib.rm_ctx_create(0, ctypes.byref(h)), "rm_ctx_create")
    try:
        buf = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        T, H, W = device.buffer_shape(buf)
        heat = torch.empty((H, W), dtype=torch.float64, device=buf.device)
        mm = (ctypes.c_double * 2)()
        _capi.check(lib, lib.rm_calibrate(h, device.ptr(buf), device.buffer_dtype_code(buf), T, H, W, 10.0, 0.1, 1.0, float(amp), L, S, 0.7,
                                          flags, device.ptr(heat), mm, device.stream_ptr()), "rm_calibrate")
        torch.cuda.synchronize()
        return heat.cpu().numpy(), (mm[0], mm[1])
    finally:
        torch.cuda.synchronize()
        lib.rm_ctx_destroy(h)


@pytest.mark.gpu
def test_history_independence(r, oracle):
    """one context, a mixed sequence of calls (S = 2 at 1e38, S = 3 on a dense stream, S = 2 at 500, S = 4, ...): each heatmap
    bit-identical to a fresh context's result for the same call (a plan's level-1 flag, the state and the bounds of one call must
    not leak into the next)"""
    rng = np.random.default_rng(19)
    a = rng.random((4, 360, 640)); a[:, :150] *= 0.05
    dense = rng.random((8, 270, 480))
    seq = [(a, 1e38, 4, 2, 0), (dense, 500.0, 5, 3, 0), (a, 500.0, 4, 2, 0), (dense, 500.0, 6, 4, 0), (a, -1e40, 4, 2, bs.FLAG_FF_PER_LEVEL),
           (dense, 1e38, 5, 3, 0), (a, 500.0, 4, 2, bs.FLAG_FF_PER_LEVEL), (dense, 500.0, 3, 1, 0), (a, 1e38, 4, 2, 0), (dense, 500.0, 6, 4, 0)]
    for k, call in enumerate(seq):
        heat, mm = r.calibrate(*call)
        want, mm2 = _fresh_calibrate(*call)
        assert bs.same(heat, want) and bs.same_mm(mm, mm2), (k, call[1:])
