"""Several subjects by optical flow in one call per clip (rm_flow_multi_clip, rm_pca_reduce_windows_multi,
SubjectTracker(motion_extraction_method='flow')) on the host-emulated build (tests/emu): each against the per-subject calls it stands
for, bit for bit (np.array_equal, NaN at the same positions).  The flow reference is the per-frame loop of rm_flow_step; rm_flow_clip,
the K = 1 entry of the same driver, is compared with it as rm_flow_multi_clip is.  The cases are those of tests/flow_multi_cases.py; the GPU twin is
tests/test_gpu_flow_multi.py."""
import numpy as np
import pytest

from respmon_amd import _capi
from tests import flow_multi_cases as fm
from tests.flow_multi_cases import BEGIN, ROIS_EMU


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


@pytest.fixture(scope="module")
def api(emu):
    return fm.EmuApi(emu)


@pytest.fixture(scope="module")
def frames():
    return fm.frames_emu(1.0)


@pytest.fixture(scope="module")
def want(api, frames):
    """the loop every test compares with: 7 rm_flow_step calls on each of four states (computed once and left as it is)"""
    w = fm.run(api, frames, ROIS_EMU, [("step", 7)])
    assert [fm.lk_levels(r[3], r[2]) for r in ROIS_EMU] == [1, 2, 3, 2]
    assert all(p is not None and len(p) > 0 for p in w["pts0"]) and (w["n_good"][-1] > 0).all()     # every subject tracks to the end
    return w


def test_emu_flow_multi_equals_the_loop(api, frames, want):
    got, clips = fm.run(api, frames, ROIS_EMU, [("multi", 7)]), fm.run(api, frames, ROIS_EMU, [("clip", 7)])
    fm.assert_same(got, want, "multi")
    fm.assert_same(clips, want, "clip")
    assert np.array_equal(got["mean"][:, 1], got["mean"][:, 3]) and np.array_equal(got["n_good"][:, 1], got["n_good"][:, 3])
    assert np.array_equal(got["points"][1], got["points"][3])
    fresh = fm.run(api, frames, ROIS_EMU, [("step", 7)])
    fm.assert_same_next_step(api, frames[8], ROIS_EMU, [got, clips], fresh)


@pytest.mark.parametrize("per_chunk", [0, 2, 1])
def test_emu_flow_multi_any_grouping(api, frames, want, per_chunk):
    rois = ROIS_EMU[:3]
    w3 = dict(mean=want["mean"][:, :3], n_good=want["n_good"][:, :3], points=want["points"][:3])
    api.set_bytes(fm.chunk_bytes(rois, per_chunk) if per_chunk else 0)
    try:
        for schedule in ([("multi", 3), ("multi", 4)], [("multi", 1), ("multi", 6)], [("step", 1), ("multi", 3), ("clip", 2), ("multi", 1)]):
            got = fm.run(api, frames, rois, schedule)
            fm.assert_same(got, w3, (per_chunk, schedule))
        clips = fm.run(api, frames, rois, [("clip", 7)])
        fm.assert_same(clips, w3, (per_chunk, "clip"))
        fm.assert_same_next_step(api, frames[8], rois, [got, clips], fm.run(api, frames, rois, [("step", 7)]), per_chunk)
    finally:
        api.set_bytes(0)


def test_emu_flow_multi_unequal_lives(api):
    f = fm.frames_unequal_lives()
    rois = [ROIS_EMU[0], ROIS_EMU[2], ROIS_EMU[1]]
    begins = [BEGIN, BEGIN, np.full_like(f[0], 9)]          # the third state's corners come from a flat frame: it enters without points
    loop = fm.run(api, f, rois, [("step", 7)], begins)
    assert loop["pts0"][2] is None and loop["pts0"][0] is not None
    ng = loop["n_good"]
    # frame 4 of the video is flat inside the small rectangle: nothing can be tracked FROM it, so the step behind it loses every point
    assert ng[0, 0] > 0 and ng[3, 0] > 0 and not ng[4:, 0].any()
    assert ng[-1, 1] > 0 and not ng[:, 2].any()                         # the large one keeps some
    for per_chunk in (0, 2):
        api.set_bytes(fm.chunk_bytes(rois[:2], per_chunk) if per_chunk else 0)
        try:
            for schedule in ([("multi", 7)], [("multi", 2), ("multi", 5)], [("multi", 4), ("multi", 3)]):
                got = fm.run(api, f, rois, schedule, begins)
                fm.assert_same(got, loop, (per_chunk, schedule))
                assert not got["n_good"][4:, 0].any() and not got["mean"][4:, 0].any() and len(got["points"][0]) == 0
        finally:
            api.set_bytes(0)
    clips = fm.run(api, f, rois, [("clip", 7)], begins)
    fm.assert_same(clips, loop, "clip")
    fm.assert_same_next_step(api, f[8], rois, [got, clips], loop)
    again = api.multi(got["states"], f[7:9], rois)            # the dead states go on taking clips
    assert not again[1][:, 0].any() and not again[1][:, 2].any() and again[1][-1, 1] > 0


def test_emu_flow_multi_every_frame_dtype(api, frames, want):
    f64 = frames.astype(np.float64) * (1. / 255)
    rois = ROIS_EMU[:3]
    for f in (f64, f64.astype(np.float32), f64.astype(np.float16)):
        # (a float frame is cropped as float_to_uint8(crop): equal crops for float64; float32 / float16 round k / 255 and may differ)
        got = fm.run(api, f, rois, [("multi", 7)])
        loop = fm.run(api, f, rois, [("step", 7)])
        fm.assert_same(got, loop, (f.dtype, "multi"))
        fm.assert_same(fm.run(api, f, rois, [("clip", 7)]), loop, (f.dtype, "clip"))
        if f.dtype == np.float64:
            fm.assert_same(got, dict(mean=want["mean"][:, :3], n_good=want["n_good"][:, :3], points=want["points"][:3]), "float64 against uint8")


def test_emu_flow_multi_refusals(api, emu, frames, want):
    rois = ROIS_EMU[:3]
    B, U = _capi.RM_E_BADARG, _capi.RM_E_UNSUPPORTED
    states, _ = fm.begin_all(api, frames[0], rois)
    unbegun, other_size = api.state(), api.state()
    api.begin(other_size, frames[0], (12, 9, 60, 51))
    f = frames[1:8]

    def refused(code, name=None, sts=None, r=None, **kw):
        rc, m, ng = api.multi_rc(states if sts is None else sts, f, rois if r is None else r, **kw)
        assert rc == code, (rc, code, kw)
        assert (m == 7).all() and (ng == -7).all(), kw
        if name is not None:
            assert name in emu.lib.rm_last_error_string().decode(), emu.lib.rm_last_error_string()

    refused(B, k=0)
    refused(B, k=_capi.RM_MAX_ROIS + 1)
    refused(B, n=0)
    for null in ("states", "frames", "rois", "mean", "n_good"):
        refused(B, null=(null,))
    refused(B, "subject 1", sts=[states[0], None, states[2]])
    refused(B, dtype=_capi.RM_BGR8)
    refused(B, dtype=9)
    refused(B, win=(2, 15))
    refused(B, win=(15, 2))
    refused(B, lvl=-1)
    refused(B, n=0x7fffffff // 2)                                   # N * K overflows int (K = 3; nothing is read)
    for bad in ((-1, 9, 70, 51), (12, 9, 70, 72), (40, 9, 70, 51), (12, 9, 0, 51)):
        refused(B, "rectangle 1", r=[rois[0], bad, rois[2]])
    refused(B, "subject 2", sts=[states[0], states[1], unbegun])
    refused(B, "subject 1", sts=[states[0], other_size, states[2]])
    refused(B, "subject 2", sts=[states[0], states[1], states[1]], r=[rois[0], rois[1], rois[1]])
    refused(U, "subject 0", win=(33, 33))
    # more than LK_MAX_LEVELS levels: an 800 x 800 rectangle at winSize 3 has nine, the small rectangles beside it fit
    big = np.zeros((2, 800, 800), np.uint8)
    big[:, :80, :100] = frames[:2]
    deep = api.state()
    assert api.begin(deep, big[0], (0, 0, 800, 800), (4, 0.3, 7, 7)) is not None
    rc, m, ng = api.multi_rc([states[0], deep], big[1:], [rois[0], (0, 0, 800, 800)], win=(3, 3), lvl=9)
    assert rc == U and (m == 7).all() and (ng == -7).all() and "subject 1" in emu.lib.rm_last_error_string().decode()
    # a state without points is not subject to the tracking limits, as in rm_flow_clip
    dead = api.state()
    assert api.begin(dead, np.full_like(frames[0], 9), rois[0]) is None
    rc, m, ng = api.multi_rc([dead], f[:2], [rois[0]], win=(33, 33))
    assert rc == _capi.RM_OK and not m.any() and not ng.any()
    # every state is as it was: the valid call equals the loop
    m, ng = api.multi(states, f, rois)
    assert np.array_equal(m, want["mean"][:, :3]) and np.array_equal(ng, want["n_good"][:, :3])
    assert all(np.array_equal(api.points(states[k]), want["points"][k]) for k in range(3))


def test_emu_flow_multi_k_bounds(api, frames, want):
    one = fm.run(api, frames, ROIS_EMU[1:2], [("multi", 7)])
    fm.assert_same(one, dict(mean=want["mean"][:, 1:2], n_good=want["n_good"][:, 1:2], points=want["points"][1:2]))
    rois = [(4 + 9 * (k % 8), 3 + 7 * (k // 8), 24, 20) for k in range(64)]
    got = fm.run(api, frames[:3], rois, [("multi", 2)])
    loop = fm.run(api, frames[:3], rois, [("step", 2)])
    assert sum(p is not None for p in loop["pts0"]) >= 32 and (loop["n_good"][-1] > 0).sum() >= 32
    fm.assert_same(got, loop, "multi")
    fm.assert_same(fm.run(api, frames[:3], rois, [("clip", 2)]), loop, "clip")


def test_emu_flow_clip_alternating_states_share_the_context(api, frames):
    fm.check_alternating_one_subject_clips(api, frames)


def test_emu_pca_reduce_windows_multi(api):
    lists = fm.check_pca_windows_multi(api)
    allrows = np.concatenate([lists[5], lists[129]])
    B = _capi.RM_E_BADARG
    ok = [(0, 5, 0), (5, 129, 2)]
    assert api.pca_multi_rc(allrows, ok, 128)[0] == _capi.RM_OK
    for seg in ([(0, 5, 6), (5, 129, 2)], [(0, 5, -1), (5, 129, 2)], [(0, -5, 0), (5, 129, 2)], [(-1, 5, 0), (5, 129, 2)],
                [(0, 6, 0), (5, 129, 2)], [(5, 129, 2), (0, 6, 0)], [(0, 5, 0), (0, 5, 0)]):
        rc, out = api.pca_multi_rc(allrows, seg, 128)
        assert rc == B and (out == -7).all(), seg
    assert api.pca_multi_rc(allrows, ok, 0)[0] == B
    assert api.pca_multi_rc(allrows, ok, 128, k=0)[0] == B
    assert api.pca_multi_rc(allrows, [(0, 1, 0)] * (_capi.RM_MAX_ROIS + 1), 128, k=_capi.RM_MAX_ROIS + 1)[0] == B


# ---- SubjectTracker('flow') against stand-alone monitors ------------------------------------------------------------------------------
class _Backend:
    """the tracker's backend interface on the emulated C-ABI"""

    def __init__(self, api):
        self.api = api

    def flow_state(self):
        return self.api.state()

    def flow_begin(self, state, g, x, y, w, h, maxCorners, qualityLevel, minDistance, blockSize):
        return self.api.begin(state, g, (x, y, w, h), (maxCorners, qualityLevel, minDistance, blockSize))

    def flow_points(self, state, cap):
        return self.api.points(state, cap)

    def flow_multi_clip(self, states, frames, rois, winSize, maxLevel, criteria):
        assert (tuple(winSize), maxLevel, tuple(criteria)) == (fm.WIN, fm.LVL, fm.CRIT)
        return self.api.multi(states, frames, [tuple(int(v) for v in r) for r in rois])

    def pca_reduce_windows_multi(self, rows_list, firsts, window):
        return self.api.pca_multi(rows_list, firsts, window)

    def roi_mean_multi_clip(self, frames, rois):
        from tests.emu_harness import DT, ptr
        f = np.ascontiguousarray(frames)
        r = np.ascontiguousarray(rois, np.int32).reshape(-1, 4)
        out = np.empty((len(f), len(r)))
        emu = self.api.emu
        emu.ck(emu.lib.rm_roi_mean_multi_clip(emu.ctx, ptr(f), DT[f.dtype], *f.shape, ptr(r), len(r), ptr(out), None), "roi_mean_multi_clip")
        return out


@pytest.fixture(scope="module")
def monitors(emu):
    """three stand-alone monitors on the 30 frames, each in one clip: what every grouping of the tracker is compared with"""
    from tests import test_emu_flow_clip as fc
    frames = fm.tracker_frames()
    mons = []
    for roi in ROIS_EMU[:3]:
        mon = fc._monitor(emu, frames, "flow", measure_buffer_length=16)
        mon.skip_calibration(*roi)
        mon.step_clip(frames)
        mons.append(mon)
    assert mons[0].state == 'error' and len(mons[0].all_data) == 22 and mons[0].data[-1] is np.nan     # lost on the step FROM the flat frame 20 ...
    assert mons[1].state == mons[2].state == 'measure' and len(mons[1].all_data) == 30                 # ... the others are not
    return frames, mons


@pytest.mark.parametrize("sizes", [[30], [1, 7, 22], [1] * 30])
def test_emu_tracker_flow_equals_monitors(emu, api, monitors, sizes):
    from respmon_amd.subjects import SubjectTracker
    from tests import test_emu_flow_clip as fc
    frames, mons = monitors
    tr = SubjectTracker(ROIS_EMU[:3], 10, measure_buffer_length=16, save_all_data=True, backend=_Backend(api), motion_extraction_method='flow')
    fm.step_in_clips(tr, frames, sizes)
    assert tr.lost == [True, False, False] and tr[0].error_message == "error detection found poor signal"
    for k in range(3):
        fm.assert_subject_equals_monitor(tr[k], tr.motion_key_points(k), mons[k], (sizes, k))
    # the lost subject begins again on further frames: a fresh monitor on the same frames
    more = fm.tracker_frames(30, lost_at=29)[:12]
    kept = len(tr[0].all_data)
    tr.restart(0)
    assert tr.lost == [False, False, False] and len(tr[0].data) == 0 and len(tr[0].motion_data) == 0
    fm.step_in_clips(tr, more, [5, 7])
    mon = fc._monitor(emu, more, "flow", measure_buffer_length=16)
    mon.skip_calibration(*ROIS_EMU[0])
    mon.step_clip(more)
    sub = tr[0]
    for name in fm.SIGNALS:
        assert np.array_equal(np.array(getattr(sub, name), float), np.array(getattr(mon, name), float), equal_nan=True), name
    assert np.array_equal(np.array(sub.all_data[kept:], float), np.array(mon.all_data, float))
    assert np.array_equal(np.array(sub.motion_data, np.float32), np.array(mon.motion_data, np.float32)) and len(sub.motion_data) == 11
    assert np.array_equal(tr.motion_key_points(0), mon.motion_key_points)
    # the other two went on through the restart without a gap
    assert len(tr[1].all_data) == 42 and not tr[1].lost


def test_emu_tracker_no_key_points_and_all_lost(emu, api):
    """a subject whose first frame has no corners is lost at once (value 0.0, as the monitor records it); with every subject lost
    step_clip makes no device call"""
    from respmon_amd.subjects import SubjectTracker
    from tests import test_emu_flow_clip as fc
    frames = fm.tracker_frames()[:6].copy()
    x, y, w, h = ROIS_EMU[0]
    frames[0, y:y + h, x:x + w] = 9
    be = _Backend(api)
    tr = SubjectTracker(ROIS_EMU[:1], 10, save_all_data=True, backend=be, motion_extraction_method='flow')
    assert tr.step_clip(frames) == 6
    mon = fc._monitor(emu, frames, "flow")
    mon.skip_calibration(*ROIS_EMU[0])
    assert mon.step_clip(frames) == 1
    assert tr.lost == [True] and tr[0].error_message == mon.error_message == "No motion key points found."
    assert list(tr[0].data) == list(mon.data) == [0.0] and tr[0].all_data == mon.all_data
    be.flow_multi_clip = be.flow_begin = None                    # any device call would raise
    assert tr.step_clip(frames) == 6 and list(tr[0].data) == [0.0]
    tr.restart(0, ROIS_EMU[1])                                  # a new rectangle: tracking begins again there
    be = tr._backend = _Backend(api)
    tr.step_clip(frames)
    mon = fc._monitor(emu, frames, "flow")
    mon.skip_calibration(*ROIS_EMU[1])
    mon.step_clip(frames)
    assert tr.rois == [ROIS_EMU[1]] and not tr[0].lost
    assert np.array_equal(np.array(tr[0].data), np.array(mon.data)) and np.array_equal(tr.motion_key_points(0), mon.motion_key_points)


def test_emu_tracker_average_is_unchanged(api):
    from respmon_amd.subjects import SubjectTracker
    frames = fm.tracker_frames()
    be = _Backend(api)
    tr = SubjectTracker(ROIS_EMU[:3], 10, measure_buffer_length=16, save_all_data=True, backend=be)
    assert tr.motion_extraction_method == 'average' and tr.step_clip(frames[:11]) == 11 and tr.step_clip(frames[11:]) == 19
    means = be.roi_mean_multi_clip(frames, np.array(ROIS_EMU[:3], np.int32))
    for k in range(3):
        assert np.array_equal(np.array([v for _, v in tr[k].all_data]), means[:, k])
        assert len(tr[k].data) == 16 and tr[k].buffers == [tr[k].data, tr[k].t, tr[k].freq] and tr[k].disable_error_detection
    assert tr.lost == [False, False, False]
