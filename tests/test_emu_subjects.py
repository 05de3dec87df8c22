"""Several subjects per frame on the host-emulated build (tests/emu): rm_heatmap_to_rois against the ranking the oracle's cv2
stand-ins give (tests/subjects_cases.py), rm_roi_mean_multi_clip against per-call rm_roi_mean bit for bit, and SubjectTracker against
RespiratoryMonitor objects fed the same frames.  The GPU twin is tests/test_gpu_subjects.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import subjects_cases as sc
from tests.emu_harness import DT, ptr


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


# ---- rm_heatmap_to_rois ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_emu_heatmap_to_rois_equals_oracle_ranking(emu, oracle, case):
    """Rectangles and areas of every K and min_area equal the oracle's list exactly; entry 0 is the single-ROI function's answer."""
    H, W = case.heat.shape

    def call(K, min_area):
        return sc.heatmap_to_rois(emu.lib, emu.ctx, ptr(case.heat), H, W, K, min_area, clip=case.clip)

    sc.check_case(oracle, case, call, lambda: emu.heatmap_to_roi(case.heat, sc.THRESHOLD, clip_frame=case.clip)[0])


def test_emu_cases_reach_what_they_are_for(oracle):
    """The table itself: more than 64 contours in the random images, exact ties, contours of area 0, an island that is not listed."""
    by = {c.name: c for c in sc.CASES}
    for g in ("33x70", "48x100", "40x64", "64x128"):
        assert len(by["random30_" + g].all_contours(oracle)) > _capi.RM_MAX_ROIS
        assert [a for a, _ in by["tie_two_a_" + g].all_contours(oracle)] == [15.0, 15.0]
        assert [a for a, _ in by["tie_two_shapes_" + g].all_contours(oracle)] == [8.0, 8.0]
        assert sorted(a for a, _ in by["tie_three_" + g].all_contours(oracle)) == [1.0, 6.0, 6.0, 6.0, 21.0]
        assert len(by["ring_island_" + g].all_contours(oracle)) == 2
        assert len(by["checker_" + g].all_contours(oracle)) == 51
        assert sum(a == 0.0 for a, _ in by["pixels_lines_" + g].all_contours(oracle)) == 5
        assert len(by["edges_" + g].all_contours(oracle)) == 7 and len(by["edges_" + g + "_clip"].all_contours(oracle)) == 6
    # the two blobs of a tie swap their rank with their raster order
    a, b = by["tie_two_a_33x70"].expected(oracle, 2, 0.0), by["tie_two_b_33x70"].expected(oracle, 2, 0.0)
    assert a[0][1][0] > a[1][1][0] and b[0][1][0] < b[1][1][0]
    assert len(by["five_blobs_3x200"].all_contours(oracle)) == 5 and by["empty_1x1"].all_contours(oracle) == []


def test_emu_heatmap_to_rois_without_area_array(emu, oracle):
    case = next(c for c in sc.CASES if c.name == "five_blobs_48x100")
    rc, rois, _, n = sc.heatmap_to_rois(emu.lib, emu.ctx, ptr(case.heat), 48, 100, 5, 0.0, want_area=False)
    assert rc == _capi.RM_OK and n == 5 and rois == [r for _, r in case.expected(oracle, 5, 0.0)]


def test_emu_heatmap_to_rois_argument_errors(emu):
    heat = next(c for c in sc.CASES if c.name == "one_blob_33x70").heat
    H, W = heat.shape
    xywh = np.zeros((64, 4), np.int32); area = np.zeros(64); n = ctypes.c_int(5)
    lib, ctx = emu.lib, emu.ctx

    def rc(h=ptr(heat), H=H, W=W, K=4, min_area=0.0, x=ptr(xywh), a=ptr(area), nn=ctypes.byref(n)):
        return lib.rm_heatmap_to_rois(ctx, h, H, W, sc.THRESHOLD, K, min_area, x, a, nn, None)

    assert rc() == _capi.RM_OK and n.value == 1
    for kw in (dict(K=0), dict(K=-1), dict(K=_capi.RM_MAX_ROIS + 1), dict(min_area=-1.0), dict(min_area=-1e-300),
               dict(min_area=float("nan")), dict(x=None), dict(nn=None), dict(H=0), dict(W=0), dict(h=None)):
        n.value = 5
        assert rc(**kw) == _capi.RM_E_BADARG, kw
        if "nn" not in kw:
            assert n.value == 0, kw
    assert rc(K=_capi.RM_MAX_ROIS) == _capi.RM_OK
    assert rc(min_area=float("inf")) == _capi.RM_NO_CONTOUR and n.value == 0
    assert lib.rm_heatmap_to_rois(None, ptr(heat), H, W, sc.THRESHOLD, 4, 0.0, ptr(xywh), ptr(area), ctypes.byref(n), None) == _capi.RM_E_BADARG


@pytest.mark.parametrize("labelling", [-1, 1])
def test_emu_multi_call_leaves_the_single_roi_stage_alone(emu, oracle, labelling):
    """rm_heatmap_to_roi on two alternating images with rm_heatmap_to_rois calls (other images, another geometry too) in between:
    every ROI and every rm_contour_stats pair equals the sequence without them."""
    by = {c.name: c for c in sc.CASES}
    seq = [by["random30_40x64"], by["five_blobs_40x64"], by["random30_40x64"], by["one_blob_40x64"], by["random30_40x64"]]
    between = [by["checker_40x64"], by["random30_33x70"], by["empty_40x64"], by["edges_40x64_clip"]]

    def run(with_multi):
        out = []
        for i, c in enumerate(seq):
            out.append((emu.heatmap_to_roi(c.heat, sc.THRESHOLD, labelling=labelling)[0], emu.contour_stats(), emu.roi_path()))
            if with_multi and i < len(between):
                m = between[i]
                rc, rois, _, _ = sc.heatmap_to_rois(emu.lib, emu.ctx, ptr(m.heat), *m.heat.shape, 5, 0.0, clip=m.clip)
                assert rois == [r for _, r in m.expected(oracle, 5, 0.0)]
        return out

    def restart():      # an extraction at another geometry: both runs start from the same counters of the labelling rule
        emu.heatmap_to_roi(by["empty_48x100"].heat)
        return emu.contour_stats(), emu.roi_path()

    start = restart()
    plain = run(False)
    assert restart() == start
    assert run(True) == plain


def test_emu_locate_multi_equals_oracle_ranking(emu, oracle):
    """rm_locate_multi on the pinned three-subject buffer: the oracle's ranked list; entry 0 and max_rois == 1 are rm_locate."""
    v = sc.three_subject_clip(sc.THREE_SEED, sc.THREE_AMPS)
    want = sc.oracle_ranking(oracle, v)
    assert [a for a, _ in want] == sc.THREE_AREAS
    T, H, W = v.shape
    rc, rois, areas = sc.locate_multi(emu.lib, emu.ctx, ptr(v), _capi.RM_U8, T, H, W, 8)
    assert rc == _capi.RM_OK and rois == [r for _, r in want] and areas == sc.THREE_AREAS
    one = sc.locate(emu.lib, emu.ctx, ptr(v), _capi.RM_U8, T, H, W)
    assert sc.locate_multi(emu.lib, emu.ctx, ptr(v), _capi.RM_U8, T, H, W, 1)[1] == [one] == rois[:1]
    for bad in (dict(K=0), dict(K=65), dict(min_area=-1.0), dict(min_area=float("nan"))):
        assert sc.locate_multi(emu.lib, emu.ctx, ptr(v), _capi.RM_U8, T, H, W, **{"K": 4, **bad})[0] == _capi.RM_E_BADARG, bad


# ---- rm_roi_mean_multi_clip ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.CLIP_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("K", [1, 3, 64])
def test_emu_roi_mean_multi_clip_equals_per_call_means(emu, dtype, K):
    frames = sc.small_clip(dtype)
    N, H, W = frames.shape
    rois = sc.small_rois(K)
    rc, out = sc.roi_mean_multi_clip(emu.lib, emu.ctx, ptr(frames), DT[frames.dtype], N, H, W, rois)
    assert rc == _capi.RM_OK
    want = np.array([[emu.roi_mean(frames[i], *r) for r in rois] for i in range(N)])
    assert np.array_equal(out, want)
    if K == 1:      # ... which is rm_roi_mean_clip
        clip = np.empty(N)
        emu.ck(emu.lib.rm_roi_mean_clip(emu.ctx, ptr(frames), DT[frames.dtype], N, H, W, *rois[0], ptr(clip), None), "roi_mean_clip")
        assert np.array_equal(out[:, 0], clip)


def test_emu_roi_mean_multi_clip_refuses_the_whole_call(emu):
    frames = sc.small_clip(np.uint8)
    N, H, W = frames.shape
    good = sc.small_rois(5)
    code = DT[frames.dtype]
    for bad in ((0, 0, W + 1, 1), (-1, 0, 2, 2), (3, 3, 0, 4), (3, 3, 4, 0), (W - 2, 0, 3, 1), (0, H - 1, 1, 2)):
        for pos in (0, 2, 5):
            rois = good[:pos] + [bad] + good[pos:]
            rc, out = sc.roi_mean_multi_clip(emu.lib, emu.ctx, ptr(frames), code, N, H, W, rois)
            assert rc == _capi.RM_E_BADARG and np.all(out == -7.0), (bad, pos)
    out = np.full((N, 70), -7.0)
    r65 = np.array(sc.small_rois(64) + [good[0]], np.int32)
    assert emu.lib.rm_roi_mean_multi_clip(emu.ctx, ptr(frames), code, N, H, W, ptr(r65), 65, ptr(out), None) == _capi.RM_E_BADARG
    assert emu.lib.rm_roi_mean_multi_clip(emu.ctx, ptr(frames), code, N, H, W, ptr(r65), 0, ptr(out), None) == _capi.RM_E_BADARG
    assert emu.lib.rm_roi_mean_multi_clip(emu.ctx, ptr(frames), code, 0, H, W, ptr(r65), 3, ptr(out), None) == _capi.RM_E_BADARG
    assert emu.lib.rm_roi_mean_multi_clip(emu.ctx, ptr(frames), _capi.RM_BGR8, N, H, W, ptr(r65), 3, ptr(out), None) == _capi.RM_E_BADARG
    assert emu.lib.rm_roi_mean_multi_clip(emu.ctx, ptr(frames), code, N, H, W, None, 3, ptr(out), None) == _capi.RM_E_BADARG
    assert np.all(out == -7.0)


# ---- SubjectTracker --------------------------------------------------------------------------------------------------------------
class MeanBackend:
    """Stand-in for the device backend: numpy means, the same expression for the one-region and the several-region call."""

    def __init__(self):
        self.multi_calls = 0

    def alloc_buffer(self, T, H, W, dtype):
        raise AssertionError("a tracker (or a monitor past skip_calibration in this test) allocates no calibration buffer")

    def bgr_to_gray(self, frame):
        return np.ascontiguousarray(frame[..., 0])

    @staticmethod
    def _mean(frame, x, y, w, h):
        return float(np.average(frame[y:y + h, x:x + w] * (1. / 255)))

    def roi_mean_clip(self, frames, x, y, w, h):
        return np.array([self._mean(f, x, y, w, h) for f in frames])

    def roi_mean_multi_clip(self, frames, rois):
        self.multi_calls += 1
        return np.array([[self._mean(f, *r) for r in rois] for f in frames])


class _NoBufferBackend(MeanBackend):
    def alloc_buffer(self, T, H, W, dtype):
        return np.zeros((1, 1, 1))


def test_subject_tracker_equals_one_monitor_per_subject():
    """A 40-frame clip split at frames 1 | 13 | 26: data, t, freq and peak_indices of every subject equal those of a RespiratoryMonitor
    (skip_calibration at that ROI, 'average') fed the same frames through step_clip -- with deques short enough that the pop-left
    rule acts."""
    from respmon_amd import synth
    from respmon_amd.base import RespiratoryMonitor
    from respmon_amd.measure import BreathSignal
    from respmon_amd.subjects import Subject, SubjectTracker
    fps, n, H, W = 5, 40, 30, 50
    rois = [(2, 3, 12, 10), (20, 5, 9, 14), (34, 12, 15, 16), (20, 5, 9, 14)]
    t = np.arange(n) / fps
    frames = np.full((n, H, W), 90, np.uint8)
    for (x, y, w, h), f, a in zip(rois[:3], (0.45, 0.40, 0.35), (60, 35, 80)):
        frames[:, y:y + h, x:x + w] = (128 + a * np.sin(2 * np.pi * f * t + 0.3))[:, None, None].astype(np.uint8)
    cuts = [(0, 1), (1, 13), (13, 26), (26, 40)]
    be = MeanBackend()
    tracker = SubjectTracker(rois, fps, measure_buffer_length=32, backend=be)
    assert tracker.bpm == [None] * 4 and len(tracker) == 4 and tracker.rois == rois
    for a, b in cuts:
        assert tracker.step_clip(frames[a:b]) == b - a
    assert be.multi_calls == len(cuts)                      # one device call per clip, whatever the number of subjects
    for k, roi in enumerate(rois):
        mon = RespiratoryMonitor(capture_target=synth.FakeCapture(frames[:1], fps=fps), visualize=None, save_all_data=False,
                                 run_on_init=False, backend=_NoBufferBackend(), motion_extraction_method="average")
        mon.measure_buffer_length = 32
        mon.skip_calibration(*roi)
        for a, b in cuts:
            assert mon.step_clip(frames[a:b]) == b - a
        s = tracker[k]
        assert len(s.data) == 32 and list(s.data) == list(mon.data) and list(s.t) == list(mon.t)
        assert list(s.freq) == list(mon.freq) and list(s.peak_indices) == list(mon.peak_indices)
        assert np.array_equal(s.filtered_data, mon.filtered_data) and np.array_equal(s.peak_times, mon.peak_times)
        assert tracker.bpm[k] == (mon.freq[-1] if len(mon.freq) else None)
    assert all(b is not None for b in tracker.bpm[:3])      # every breathing region has produced an estimate
    assert list(tracker[1].data) == list(tracker[3].data)   # the repeated rectangle
    # the same code, not a copy of it
    assert Subject.measure is BreathSignal.measure and RespiratoryMonitor.measure is BreathSignal.measure
    assert Subject.find_peaks is RespiratoryMonitor.find_peaks and Subject._record_value is RespiratoryMonitor._record_value
    assert not any(hasattr(s, "calibration_buffer") for s in tracker.subjects)
