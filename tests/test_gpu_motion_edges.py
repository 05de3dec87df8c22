"""The motion-extraction path (reference base.py:354-407) at the inputs a webcam session rarely produces but locate() can return:
crops from 1x1 to 23x23 and whole 1080p / 4K frames, more tracked points than k_flow_finish stages (FLOW_FINISH_MAX), every
frame dtype of the ROI mean and crop, and PCA inputs that are collinear, degenerate or far from 1 in magnitude.  Each case is
held to the oracle, to a high-precision reference (tests/motion_reference.py), or both.  The host-emulated twin of the small-crop
and PCA sweeps is tests/test_emu_motion_edges.py."""
import numpy as np
import pytest

from respmon_amd import synth
from tests import motion_reference as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd.base import _Backend
    return _Backend()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _GpuAdapter:
    """The sweep drivers' backend interface on the product's C-ABI (device inputs)."""

    def __init__(self, be):
        self.be = be
        self.state = be.flow_state()
        self.h = self.w = 0

    def gftt(self, img, bs):
        return self.be.good_features_to_track(_dev(img), mr.FEATURE["maxCorners"], mr.FEATURE["qualityLevel"], mr.FEATURE["minDistance"], bs)

    def begin(self, img, bs):
        return self.begin_pts(img, mr.FEATURE["maxCorners"], mr.FEATURE["qualityLevel"], mr.FEATURE["minDistance"], bs)

    def begin_pts(self, img, n, q, md, bs):
        self.h, self.w = img.shape
        self.cap = n
        return self.be.flow_begin(self.state, _dev(img), 0, 0, self.w, self.h, n, q, md, bs)

    def lk(self, a, b, pts, win, lvl, crit):
        return self.be.calc_optical_flow_pyr_lk(_dev(a), _dev(b), pts, win, lvl, crit)

    def step(self, b, win, lvl, crit):
        mean, ng = self.be.flow_step(self.state, _dev(b), 0, 0, self.w, self.h, win, lvl, crit)
        return mean, ng, self.be.flow_points(self.state, self.cap)


def _smooth_noise(H, W, seed, sigma=2.0):
    """Band-limited random texture [H, W] float64 and a renderer of it shifted by (dx, dy) to uint8: many Shi-Tomasi corners
    (about one local maximum per few sigma^2), smooth enough for the float64 brute-force LK to agree with the fixed-point one."""
    import scipy.ndimage as ndi
    f = ndi.gaussian_filter(np.random.default_rng(seed).standard_normal((H, W)), sigma, mode="wrap")
    f = 127.5 + 60.0 * f / f.std()

    def render(dx=0.0, dy=0.0):
        g = ndi.shift(f, (dy, dx), order=3, mode="wrap") if (dx or dy) else f
        return np.clip(np.round(g), 0, 255).astype(np.uint8)
    return render


def test_corners_on_every_small_crop(be, oracle):
    """(a) h, w in {1..23}^2, textured and flat, blockSize 3, 5 and 7, both entry points: None exactly when the oracle says so."""
    n = mr.sweep_corners(_GpuAdapter(be), oracle, synth.synth_texture(64, 64, seed=23))
    print("motion-edges: %d corner cases" % n)
    assert n == len(mr.SMALL) ** 2 * 2 * 3 * 2


def test_lk_on_every_small_crop(be, oracle):
    """(b) six winSizes, maxLevel 0-4 and a clamped 9, probe points inside / on / 0.5 px and 5 px outside every small crop; the
    four-call path and the resident path."""
    n = mr.sweep_lk(_GpuAdapter(be), oracle, synth.synth_texture(64, 64, seed=23))
    print("motion-edges: %d LK cases" % n)
    assert n >= len(mr.SMALL) ** 2 * 4


def test_lk_limits_are_refused_not_crashed(be, oracle):
    """(b) a window over LK_MAX_WIN taps, and a pyramid that still needs more than LK_MAX_LEVELS levels after lk_max_level's
    clamping (winSize 3, maxLevel 9 on a 1080p crop), are RM_E_UNSUPPORTED from both paths."""
    from respmon_amd import _capi
    img = _smooth_noise(1080, 1920, seed=3)()
    pts = np.array([[[960.0, 540.0]], [[100.5, 80.25]]], np.float32)
    gp = _GpuAdapter(be)
    assert gp.begin_pts(img, 100, 0.3, 7, 7) is not None
    for win, lvl in (((33, 33), 2), ((64, 17), 0), ((3, 3), 9)):
        assert mr.lk_expect_unsupported(1080, 1920, win, lvl)
        with pytest.raises(_capi.RespmonError, match=r"\(%d\)" % _capi.RM_E_UNSUPPORTED):
            gp.lk(img, img, pts, win, lvl, (3, 10, 0.03))
        with pytest.raises(_capi.RespmonError, match=r"\(%d\)" % _capi.RM_E_UNSUPPORTED):
            gp.step(img, win, lvl, (3, 10, 0.03))
    assert not mr.lk_expect_unsupported(1080, 1920, (3, 3), 7)    # 8 levels: the largest pyramid that is tracked
    nxt = _smooth_noise(1080, 1920, seed=3)(0.4, -0.3)
    p1, st = gp.lk(img, nxt, pts, (3, 3), 7, (3, 10, 0.03))
    r1, rs, _ = oracle.calcOpticalFlowPyrLK(img, nxt, pts, None, winSize=(3, 3), maxLevel=7, criteria=(3, 10, 0.03))
    assert np.array_equal(st, rs) and np.array_equal(p1[rs == 1], r1[rs == 1])


@pytest.mark.parametrize("max_corners", [6000, 6001, 20000])
def test_point_counts_across_flow_finish_max(be, oracle, max_corners):
    """(c) 1080-row crop, qualityLevel 0.001, minDistance 1: corners, three resident steps (k_flow_finish up to 6000 points,
    k_flow_finish_seq above) against the oracle and the four-call path; the float64 brute-force LK on the largest case."""
    from tests import lk_bruteforce as bf
    H, W = 1080, 1440
    render = _smooth_noise(H, W, seed=11)
    frames = [render(0.3 * t, -0.2 * t) for t in range(4)]
    crops = [mr.reference_crop(oracle, f) for f in frames]
    ref0 = oracle.goodFeaturesToTrack(crops[0], max_corners, 0.001, 1, blockSize=7)
    # the texture fills every cap, so more than FLOW_FINISH_MAX points are tracked and k_flow_finish_seq cannot be skipped
    assert len(ref0) == max_corners and (max_corners > 6001 or len(oracle.goodFeaturesToTrack(crops[0], 6002, 0.001, 1, blockSize=7)) == 6002)
    st_ = be.flow_state()
    pts = be.flow_begin(st_, _dev(frames[0]), 0, 0, W, H, max_corners, 0.001, 1, 7)
    assert np.array_equal(pts, ref0)
    lk = dict(winSize=(15, 15), maxLevel=2, criteria=(3, 10, 0.03))
    cur = ref0
    for t in range(1, 4):
        mean, ng = be.flow_step(st_, _dev(frames[t]), 0, 0, W, H, **lk)
        r1, rs, _ = oracle.calcOpticalFlowPyrLK(crops[t - 1], crops[t], cur, None, **lk)
        good = rs.ravel() == 1
        assert ng == int(good.sum()) and ng > 0.5 * len(cur)
        assert np.array_equal(mean, np.mean(cur.reshape(-1, 2)[good] - r1.reshape(-1, 2)[good], axis=0))   # base.py:388
        p4, s4 = be.calc_optical_flow_pyr_lk(_dev(crops[t - 1]), _dev(crops[t]), cur, **lk)            # the four-call path
        left = be.flow_points(st_, max_corners)
        assert np.array_equal(s4, rs) and np.array_equal(left.reshape(-1, 2), p4.reshape(-1, 2)[s4.ravel() == 1])
        if max_corners > 6001 and t == 1:
            # the float64 tracker on interior points, 4000 of them spread over the whole list (the brute force is slow)
            p0 = cur.reshape(-1, 2)
            inner = np.flatnonzero(good & (p0[:, 0] > 32) & (p0[:, 0] < W - 33) & (p0[:, 1] > 32) & (p0[:, 1] < H - 33))
            sel = inner[np.linspace(0, len(inner) - 1, 4000).astype(int)]
            ref = bf.lk_float(crops[0], crops[1], p0[sel])
            err = np.linalg.norm(p4.reshape(-1, 2)[sel] - ref, axis=1)
            assert err.max() <= 1e-2 and np.median(err) <= 3e-3, (err.max(), np.median(err))
        cur = r1[rs == 1].reshape(-1, 1, 2)
    print("motion-edges: maxCorners %d -> %d corners, %d tracked after 3 steps" % (max_corners, len(ref0), len(cur)))


def _frame(dtype, H, W, seed):
    """A frame of `dtype` holding random values and, in every fourth row, values next to k/255 boundaries (the nearest value of
    the dtype to k/255 and its two neighbours), where float_to_uint8's truncation changes its result."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    f = rng.random((H, W)).astype(dtype)
    k = rng.integers(1, 255, (H // 4, W))
    near = (k / 255.0).astype(dtype)
    step = rng.integers(-1, 2, near.shape)
    near = np.where(step > 0, np.nextafter(near, dtype(2)), np.where(step < 0, np.nextafter(near, dtype(0)), near))
    f[::4][:H // 4] = near
    return f


def _rois(H, W):
    return ([(0, 0, W, H), (0, 0, W, 1), (0, H - 1, W, 1), (0, 0, 1, H), (W - 1, 0, 1, H)] +
            [(x, y, 1, 1) for x in (0, W - 1) for y in (0, H - 1)] +
            [(W - 37, H - 29, 37, 29), (101, 53, W - 101, H - 53), (0, H - 200, 300, 200)])


@pytest.mark.parametrize("HW", [(1080, 1920), (2160, 3840)], ids=["1080p", "4K"])
def test_roi_mean_and_crop_every_dtype(be, oracle, HW):
    """(d) rm_roi_mean within roi_mean_bound of the exact mean (and within twice that of np.average); rm_roi_to_uint8 equal to
    float_to_uint8 bit for bit -- whole frame, one-pixel edge strips, corner pixels, crops that end on the frame's edge."""
    import torch
    H, W = HW
    worst = 0.0
    for i, dt in enumerate((np.uint8, np.float16, np.float32, np.float64)):
        f = _frame(dt, H, W, seed=100 + i)
        d = _dev(f)
        for (x, y, w, h) in _rois(H, W):
            got = be.roi_mean(d, x, y, w, h)
            v = mr.roi_values(f, x, y, w, h)
            exact = mr.roi_mean_exact(f, x, y, w, h)
            bound = mr.roi_mean_bound(w * h, float(np.abs(v).sum(dtype=np.float64)) * (1 + 1e-12))
            from fractions import Fraction
            err = abs(Fraction(got) - exact)
            assert err <= bound, (dt, (x, y, w, h), got, float(exact))
            assert abs(got - np.average(v)) <= 2 * float(bound), (dt, (x, y, w, h))
            worst = max(worst, float(err / bound) if bound else 0.0)
            crop = be.roi_to_uint8(d, x, y, w, h).cpu().numpy()
            assert np.array_equal(crop, oracle.float_to_uint8(v)), (dt, (x, y, w, h))
        del d
        torch.cuda.synchronize()
    print("motion-edges: ROI mean %dx%d worst |got - exact| / bound = %.3g" % (W, H, worst))


def test_pca_against_exact_arithmetic(be, oracle):
    """(e) k_pca_reduce against base.py:396-405 in exact arithmetic: within 64 u (|x| + |y|)(1 + 1/g) when the eigen-gap is
    not tiny, exactly y_last on covariances c*I (PCA)."""
    worst, cases = 0.0, mr.pca_families(np.random.default_rng(2024))
    for name, m in cases:
        worst = max(worst, mr.check_pca(be.pca_reduce(m), m, oracle))
    print("motion-edges: %d PCA cases, worst |got - exact| / bound = %.3g" % (len(cases), worst))
    assert worst <= 1.0


def _run_flow(frames, roi, fused):
    from respmon_amd.base import RespiratoryMonitor
    mon = RespiratoryMonitor(capture_target=synth.FakeCapture(frames, fps=10), visualize=None, save_all_data=False,
                             motion_extraction_method="flow", run_on_init=False)
    mon.fused_flow_step = fused
    mon.sync_to_fps = lambda: None
    mon.skip_calibration(*roi)
    mon.run()
    return mon


@pytest.mark.parametrize("fused", [True, False], ids=["resident", "four-call"])
def test_state_machine_on_extreme_rois(oracle, fused):
    """(f) a 2-pixel-wide ROI takes base.py's "No motion key points found." path instead of raising; a ROI that is the whole
    1080p frame gives the oracle's data trace."""
    render = _smooth_noise(1080, 1920, seed=5, sigma=3.0)
    frames = np.stack([render(1.2 * np.sin(0.6 * t), 0.7 * np.sin(0.6 * t + 1.0)) for t in range(8)])
    mon = _run_flow(frames[:4], (700, 300, 2, 64), fused)
    assert mon.state == "error" and mon.error_message == "No motion key points found."
    mon = _run_flow(frames, (0, 0, 1920, 1080), fused)
    state = oracle.FlowState()
    ref = np.array([oracle.extract_motion_flow(state, oracle.uint8_to_float(f)) for f in frames])
    got = np.array(mon.data, dtype=np.float64)
    assert len(got) == len(frames) and np.allclose(got, ref, rtol=1e-9, atol=1e-12, equal_nan=True)
