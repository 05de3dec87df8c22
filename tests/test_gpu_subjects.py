"""Several subjects per frame on the GPU: rm_heatmap_to_rois on the heat-map table of tests/subjects_cases.py against the oracle's
ranking, rm_roi_mean_multi_clip against per-call rm_roi_mean bit for bit, rm_locate_multi and RespiratoryMonitor.locate_all on a
three-subject calibration buffer, and the isolation of the multi calls from the single-ROI stage.  The host-emulated twin is
tests/test_emu_subjects.py.
UNVERIFIED: the isolation sequence on its present pair of buffers, the locate_all tests and the tracker test have not been run on an
MI355X yet; the same calls pass on the host-emulated build."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import subjects_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device

    class G:
        lib = _capi.load()
        ctx = device.ctx()
        stream = staticmethod(device.stream_ptr)
        code = staticmethod(device.dtype_code)

        @staticmethod
        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).cuda()

        @staticmethod
        def p(t):
            return ctypes.c_void_p(t.data_ptr())
    return G


@pytest.fixture(scope="module")
def three(oracle):
    """the pinned three-subject buffer, a second one, and the oracle's ranked lists (with and without the clipped frame), made once"""
    a = sc.three_subject_clip(sc.THREE_SEED, sc.THREE_AMPS)
    b = sc.three_subject_clip(sc.OTHER_SEED, sc.OTHER_AMPS)
    want = {False: sc.oracle_ranking(oracle, a, clip=False), True: sc.oracle_ranking(oracle, a, clip=True)}
    assert [x for x, _ in want[False]] == sc.THREE_AREAS
    return a, b, want


def _single(gpu, heat_dev, H, W, clip):
    xywh = np.zeros(4, np.int32)
    gpu.lib.rm_set_contour_clip_frame(gpu.ctx, 1 if clip else 0)
    try:
        rc = _capi.check(gpu.lib, gpu.lib.rm_heatmap_to_roi(gpu.ctx, gpu.p(heat_dev), H, W, sc.THRESHOLD, ctypes.c_void_p(xywh.ctypes.data), None,
                                                            None, gpu.stream()), "rm_heatmap_to_roi")
    finally:
        gpu.lib.rm_set_contour_clip_frame(gpu.ctx, 0)
    return None if rc == _capi.RM_NO_CONTOUR else tuple(int(v) for v in xywh)


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_heatmap_to_rois_equals_oracle_ranking(gpu, oracle, case):
    H, W = case.heat.shape
    heat = gpu.dev(case.heat)

    def call(K, min_area):
        return sc.heatmap_to_rois(gpu.lib, gpu.ctx, gpu.p(heat), H, W, K, min_area, clip=case.clip, stream=gpu.stream())

    sc.check_case(oracle, case, call, lambda: _single(gpu, heat, H, W, case.clip))


def _check_means(gpu, frames, rois):
    N, H, W = frames.shape
    d = gpu.dev(frames)
    rc, out = sc.roi_mean_multi_clip(gpu.lib, gpu.ctx, gpu.p(d), gpu.code(d), N, H, W, rois, stream=gpu.stream())
    assert rc == _capi.RM_OK
    want = np.empty((N, len(rois)))
    one = ctypes.c_double()
    for i in range(N):
        for k, (x, y, w, h) in enumerate(rois):
            _capi.check(gpu.lib, gpu.lib.rm_roi_mean(gpu.ctx, gpu.p(d[i]), gpu.code(d), H, W, x, y, w, h, ctypes.byref(one), gpu.stream()), "rm_roi_mean")
            want[i, k] = one.value
    assert np.array_equal(out, want)
    return d, out


@pytest.mark.parametrize("dtype", sc.CLIP_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("K", [1, 3, 64])
def test_roi_mean_multi_clip_equals_per_call_means(gpu, dtype, K):
    frames = sc.small_clip(dtype)
    rois = sc.small_rois(K)
    d, out = _check_means(gpu, frames, rois)
    if K == 1:
        N, H, W = frames.shape
        clip = np.empty(N)
        _capi.check(gpu.lib, gpu.lib.rm_roi_mean_clip(gpu.ctx, gpu.p(d), gpu.code(d), N, H, W, *rois[0], ctypes.c_void_p(clip.ctypes.data),
                                                      gpu.stream()), "rm_roi_mean_clip")
        assert np.array_equal(out[:, 0], clip)


def test_roi_mean_multi_clip_float16_33_frames_7_subjects(gpu):
    frames = sc.small_clip(np.float16, N=33, H=64, W=128, seed=17)
    rois = [(0, 0, 128, 64), (5, 3, 100, 50), (64, 0, 64, 64), (64, 0, 64, 64), (127, 63, 1, 1), (1, 1, 3, 60), (20, 30, 97, 1)]
    _check_means(gpu, frames, rois)


def test_roi_mean_multi_clip_refuses_the_whole_call(gpu):
    frames = sc.small_clip(np.float32)
    N, H, W = frames.shape
    d = gpu.dev(frames)
    good = sc.small_rois(5)
    for bad in ((0, 0, W + 1, 1), (-1, 0, 2, 2), (3, 3, 0, 4), (0, H - 1, 1, 2)):
        rc, out = sc.roi_mean_multi_clip(gpu.lib, gpu.ctx, gpu.p(d), gpu.code(d), N, H, W, good[:2] + [bad] + good[2:], stream=gpu.stream())
        assert rc == _capi.RM_E_BADARG and np.all(out == -7.0), bad


def test_locate_multi_equals_oracle_ranking(gpu, three):
    a, _, want = three
    T, H, W = a.shape
    for frames in (gpu.dev(a), gpu.dev(a).double() * (1. / 255)):
        args = (gpu.lib, gpu.ctx, gpu.p(frames), gpu.code(frames), T, H, W)
        rc, rois, areas = sc.locate_multi(*args, 8, stream=gpu.stream())
        assert rc == _capi.RM_OK and rois == [r for _, r in want[False]] and areas == sc.THREE_AREAS
        one = sc.locate(*args, stream=gpu.stream())
        assert one == rois[0]                                                               # entry 0 equals rm_locate
        assert sc.locate_multi(*args, 1, stream=gpu.stream())[1] == [one]                   # max_rois == 1 is rm_locate
        rc, rois, areas = sc.locate_multi(*args, 2, stream=gpu.stream())
        assert rc == _capi.RM_OK and areas == sc.THREE_AREAS[:2]
        rc, rois, areas = sc.locate_multi(*args, 8, flags=_capi.RM_FLAG_CONTOUR_CLIP_FRAME, stream=gpu.stream())
        assert rois == [r for _, r in want[True]] and areas == [x for x, _ in want[True]]
        assert sc.locate_multi(*args, 8, min_area=sc.THREE_AREAS[0] + 1, stream=gpu.stream()) == (_capi.RM_NO_CONTOUR, [], [])


def test_multi_calls_leave_the_single_roi_stage_alone(gpu, three):
    """rm_locate, rm_locate_multi, rm_locate, rm_locate_multi, rm_locate on two alternating buffers, each run on a context of its
    own: every rm_locate ROI with its (components, labelled, path) triple equals the ones of the sequence without the multi calls."""
    a, b, want = three
    T, H, W = a.shape
    da, db = gpu.dev(a), gpu.dev(b)

    def run(with_multi, labelling):
        ctx = ctypes.c_void_p()
        _capi.check(gpu.lib, gpu.lib.rm_ctx_create(0, ctypes.byref(ctx)), "rm_ctx_create")
        try:
            _capi.check(gpu.lib, gpu.lib.rm_set_contour_labelling(ctx, labelling), "labelling")
            out = []
            for frames, other in ((da, db), (db, da), (da, db)):
                roi = sc.locate(gpu.lib, ctx, gpu.p(frames), gpu.code(frames), T, H, W, stream=gpu.stream())
                n, lab, path = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
                _capi.check(gpu.lib, gpu.lib.rm_contour_stats(ctx, ctypes.byref(n), ctypes.byref(lab)), "rm_contour_stats")
                _capi.check(gpu.lib, gpu.lib.rm_debug_roi_path(ctx, ctypes.byref(path)), "rm_debug_roi_path")
                out.append((roi, n.value, lab.value, path.value))
                if with_multi and len(out) < 3:
                    rc, rois, _ = sc.locate_multi(gpu.lib, ctx, gpu.p(other), gpu.code(other), T, H, W, 4, stream=gpu.stream())
                    assert rc == _capi.RM_OK and len(rois) >= 3
            return out
        finally:
            gpu.lib.rm_ctx_destroy(ctx)

    for labelling in (-1, 1):
        plain = run(False, labelling)
        assert plain[0] == plain[2] and plain[0][0] == want[False][0][1] and plain[1][0] == sc.OTHER_ROI      # two different answers
        assert run(True, labelling) == plain


@pytest.mark.parametrize("clip", [False, True])
def test_locate_all_numpy_and_device_input(gpu, three, clip):
    from respmon_amd.base import RespiratoryMonitor
    a, _, want = three
    kw = dict(pyramid_levels=5, skip_levels_at_top=2)
    RespiratoryMonitor.opencv_contours_clip_frame = clip
    try:
        for frames in (a, gpu.dev(a), a * (1. / 255)):
            rois = RespiratoryMonitor.locate_all(frames, 10, max_rois=4, **kw)
            assert rois == [r for _, r in want[clip]][:4]
            assert rois[0] == RespiratoryMonitor.locate(frames, 10, **kw)
            assert RespiratoryMonitor.locate_all(frames, 10, max_rois=2, min_area=100.0, **kw) == rois[:2]
            assert RespiratoryMonitor.locate_all(frames, 10, max_rois=4, min_area=1e9, **kw) == []
    finally:
        RespiratoryMonitor.opencv_contours_clip_frame = False


def test_subject_tracker_on_the_device(gpu, three):
    """SubjectTracker over the located regions: one rm_roi_mean_multi_clip per clip, the values of per-frame rm_roi_mean."""
    from respmon_amd.base import RespiratoryMonitor, _Backend
    from respmon_amd.subjects import SubjectTracker
    a, _, want = three
    rois = RespiratoryMonitor.locate_all(gpu.dev(a), 10, pyramid_levels=5, skip_levels_at_top=2)
    assert len(rois) == 3
    tracker = SubjectTracker(rois, 10)
    assert tracker.step_clip(gpu.dev(a[:20])) == 20 and tracker.step_clip(a[20:48]) == 28
    be = _Backend()
    d = gpu.dev(a)
    for k, (x, y, w, h) in enumerate(rois):
        assert list(tracker[k].data) == [be.roi_mean(d[i], x, y, w, h) for i in range(48)]
    assert all(b is not None and 15 < b < 35 for b in tracker.bpm), tracker.bpm        # 0.4 Hz = 24 breaths per minute
