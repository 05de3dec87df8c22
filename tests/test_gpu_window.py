"""The sliding-window calibration (include/respmon_hip.h rm_window_*, respmon_amd/window.py) on the MI355X: all eight cases of
tests/window_cases.py -- every head position at every form of the temporal kernels, push granularity, dtypes, flags, the multi-ROI
call, isolation from other calls on the context, argument errors, and the Python layer with RespiratoryMonitor(relocate_every=...).
Every comparison with the contiguous-buffer calls is exact.  The host-emulated twin (cases 1-4 and 7) is tests/test_emu_window.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import subjects_cases as sc
from tests import window_cases as wc

pytestmark = pytest.mark.gpu

MULTI_KW = dict(fps=10.0, fmin=0.1, fmax=1.0, amp=500.0, thr=0.7, threshold=sc.THRESHOLD)      # subjects_cases.LOCATE_KW in this module's terms


def _backend(ctx=None):
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device

    class B:
        lib = _capi.load()
        stream = staticmethod(device.stream_ptr)
        dev = staticmethod(lambda a: torch.from_numpy(np.array(a)).cuda())      # (a copy: the shared streams are read-only arrays)
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        out = staticmethod(lambda shape: torch.full(tuple(shape), float("nan"), dtype=torch.float64, device="cuda"))
        np = staticmethod(lambda t: t.cpu().numpy())
    B.ctx = ctx if ctx is not None else device.ctx()
    return B


@pytest.fixture(scope="module")
def be():
    return _backend()


@pytest.mark.parametrize("geom", wc.GEOMS, ids=str)
@pytest.mark.parametrize("T,knobs", [(T, k) for T in wc.TS for k in wc.knob_cases(T)], ids=str)
def test_window_every_head_position(be, geom, T, knobs):
    wc.check_every_head(be, geom, T, knobs)


@pytest.mark.parametrize("geom", wc.GEOMS, ids=str)
@pytest.mark.parametrize("T", wc.TS)
def test_window_push_granularity(be, geom, T):
    wc.check_granularity(be, geom, T)


@pytest.mark.parametrize("geom", wc.GEOMS, ids=str)
def test_window_dtypes(be, geom):
    wc.check_dtypes(be, geom, 10)


@pytest.mark.parametrize("geom", wc.GEOMS, ids=str)
@pytest.mark.parametrize("flag", wc.FLAGS)
def test_window_flags(be, geom, flag):
    wc.check_flag(be, geom, 10, flag)


def test_window_argument_errors(be):
    wc.check_argument_errors(be)


# ---- case 5 -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three():
    a = sc.three_subject_clip(sc.THREE_SEED, sc.THREE_AMPS)
    b = sc.three_subject_clip(sc.OTHER_SEED, sc.OTHER_AMPS)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


def _fill_wrapped(win, v, n=7):
    """sixteen frames that will be overwritten, then the clip in pushes of n: the ring ends holding exactly `v`, wrapped (head = 16)"""
    v = np.concatenate([v[-16:], v])
    for k in range(0, len(v), n):
        win.push_np(v[k:k + n])


def test_window_locate_multi_equals_locate_multi(be, three):
    a, _ = three
    N, H, W = a.shape
    T = N
    L, S = sc.LOCATE_KW["pyramid_levels"], sc.LOCATE_KW["skip_levels_at_top"]
    tail = be.dev(a)
    with wc.Window(be, T, H, W, L, S) as win:
        _fill_wrapped(win, a)
        assert win.info()[:2] == (T, 16)
        for K, min_area in ((8, 0.0), (2, 0.0), (1, 0.0), (8, 150.0), (8, 1e9)):
            want = sc.locate_multi(be.lib, be.ctx, be.p(tail), _capi.RM_U8, T, H, W, K, min_area=min_area, stream=be.stream())
            assert win.locate_multi(K, min_area, kw=MULTI_KW) == want, (K, min_area)
        rc, rois, areas = win.locate_multi(8, kw=MULTI_KW)
        assert rc == _capi.RM_OK and areas == sc.THREE_AREAS and len(rois) == 3
        assert win.locate(kw=MULTI_KW) == (_capi.RM_OK, rois[0])


def test_window_locate_multi_leaves_the_single_roi_stage_alone(three):
    """rm_locate on two alternating buffers, each run on a context of its own, with and without rm_window_locate_multi calls between
    them: ROI, rm_contour_stats and the path of the host stage are the same."""
    a, b = three
    N, H, W = a.shape
    L, S = sc.LOCATE_KW["pyramid_levels"], sc.LOCATE_KW["skip_levels_at_top"]
    lib = _capi.load()

    def run(with_multi, labelling):
        ctx = ctypes.c_void_p()
        _capi.check(lib, lib.rm_ctx_create(0, ctypes.byref(ctx)), "rm_ctx_create")
        be = _backend(ctx)
        da, db = be.dev(a), be.dev(b)
        try:
            _capi.check(lib, lib.rm_set_contour_labelling(ctx, labelling), "labelling")
            out = []
            with wc.Window(be, N, H, W, L, S) as win:
                for frames, other in ((da, b), (db, a), (da, b)):
                    _fill_wrapped(win, other)
                    roi = sc.locate(lib, ctx, be.p(frames), _capi.RM_U8, N, H, W, stream=be.stream())
                    n, lab, path = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
                    _capi.check(lib, lib.rm_contour_stats(ctx, ctypes.byref(n), ctypes.byref(lab)), "rm_contour_stats")
                    _capi.check(lib, lib.rm_debug_roi_path(ctx, ctypes.byref(path)), "rm_debug_roi_path")
                    out.append((roi, n.value, lab.value, path.value))
                    if with_multi:
                        rc, rois, _ = win.locate_multi(4, kw=MULTI_KW)
                        assert rc == _capi.RM_OK and len(rois) >= 3
            return out
        finally:
            lib.rm_ctx_destroy(ctx)

    for labelling in (-1, 1):
        plain = run(False, labelling)
        assert plain[0] == plain[2] and plain[1][0] == sc.OTHER_ROI and plain[0][0] != plain[1][0]
        assert run(True, labelling) == plain


# ---- case 6 -------------------------------------------------------------------------------------------------------------------
def test_window_is_isolated_from_other_calls_on_the_context(be):
    import torch
    H, W, L, S = wc.GEOMS[0]
    T = 10
    v = wc.stream(T, H, W)
    other = be.dev(wc.stream(16, 33, 47)[:16])
    with wc.Window(be, T, H, W, L, S) as win:
        for k in range(T + 4):
            win.push_np(v[k:k + 1])
            if k >= T - 2:
                # another geometry's rm_locate and an rm_magnify between two pushes: they use the context's workspace, not the ring
                sc_roi = np.zeros(4, np.int32)
                _capi.check(be.lib, be.lib.rm_locate(be.ctx, be.p(other), _capi.RM_U8, 16, 33, 47, 2.5, 0.25, 0.9, 500.0, 3, 1, 0.7, 20, 0,
                                                     ctypes.c_void_p(sc_roi.ctypes.data), be.stream()), "rm_locate")
                mag = torch.empty((16, 33, 47), dtype=torch.float64, device="cuda")
                _capi.check(be.lib, be.lib.rm_magnify(be.ctx, be.p(other), _capi.RM_U8, 16, 33, 47, 2.5, 0.25, 0.9, 20.0, 3, 1, be.p(mag), _capi.RM_F64,
                                                      be.stream()), "rm_magnify")
                m = min(k + 1, T)
                wc.same(win, v[k + 1 - m:k + 1], L, S, tag=k)
        # reset, then m pushes: a fresh window fed the same frames
        win.reset()
        assert win.info()[:2] == (0, 0)
        with wc.Window(be, T, H, W, L, S) as fresh:
            for m in (1, 4, T, T + 3):
                win.reset(); fresh.reset()
                for k in range(m):
                    win.push_np(v[10 + k:11 + k]); fresh.push_np(v[10 + k:11 + k])
                assert win.info() == fresh.info()
                assert np.array_equal(win.calibrate(), fresh.calibrate(), equal_nan=True)
                assert win.locate() == fresh.locate()
                wc.same(win, v[10 + max(0, m - T):10 + m], L, S, tag=("reset", m))


# ---- case 8 -------------------------------------------------------------------------------------------------------------------
def test_sliding_calibration_equals_locate_on_the_stacked_window(be, three):
    import torch
    from respmon_amd import dist as rdist
    from respmon_amd.base import RespiratoryMonitor
    from respmon_amd.window import SlidingCalibration
    a, _ = three
    N, H, W = a.shape
    T = 48
    kw = dict(pyramid_levels=5, skip_levels_at_top=2)
    win = SlidingCalibration(T, H, W, **kw)
    try:
        assert win.count == 0
        for k in range(0, N, 5):                                    # numpy and device tensors, uint8 and float64, mixed
            chunk = a[k:k + 5]
            win.push(chunk if k % 2 == 0 else torch.from_numpy(chunk * (1. / 255)).cuda())
        assert win.count == T and win.head == N % T and win.ring_bytes > 0
        stacked = torch.from_numpy(a[N - T:].copy()).cuda()
        assert win.locate(10) == RespiratoryMonitor.locate(stacked, 10, **kw)
        assert win.locate_all(10, max_rois=4) == RespiratoryMonitor.locate_all(stacked, 10, max_rois=4, **kw)
        assert win.locate_all(10, max_rois=2, min_area=150.0) == RespiratoryMonitor.locate_all(stacked, 10, max_rois=2, min_area=150.0, **kw)
        assert torch.equal(win.heatmap(10), rdist.hip_calibrate(stacked, 10, **kw))
        win.push(a[0])                                              # a single [H,W] frame
        assert win.count == T and win.head == (N + 1) % T
        win.reset()
        assert win.count == 0
        with pytest.raises(_capi.RespmonError):
            win.locate(10)
        with pytest.raises(ValueError):
            win.push(a[:, :10])
    finally:
        win.close()


def test_monitor_without_relocation_leaves_the_g6_trace(golden):
    """relocate_every = 0 (the default, given explicitly): the scripted run() of the G6 trace, exactly"""
    from respmon_amd import synth
    from respmon_amd.base import RespiratoryMonitor
    g = golden("g6_run_trace.npz")
    vid = synth.synth_breathing(150, 48, 64, seed=11)
    mon = RespiratoryMonitor(capture_target=synth.FakeCapture(vid, fps=30), visualize=None, save_all_data=False,
                             motion_extraction_method="average", run_on_init=False, relocate_every=0)
    mon.sync_to_fps = lambda: None
    trace = []
    real_next = mon.next_frame

    def traced():
        trace.append((["initialize", "calibration", "measure", "error"].index(mon.state), mon.calibration_buffer_idx))
        return real_next()
    mon.next_frame = traced
    mon.run()
    assert mon._window is None
    assert np.array_equal(np.array(trace, dtype=np.int32), g["c2_trace"])
    assert [mon.x, mon.y, mon.w, mon.h] == [int(v) for v in g["c2_roi"]]
    assert np.allclose(np.array(mon.data), g["c2_data"], rtol=1e-13, atol=0)
    assert np.array_equal(np.array(mon.t), g["c2_t"])


@pytest.mark.parametrize("bdt", ["float64", "uint8", "bgr8"])
def test_monitor_relocates_from_the_ring_and_needs_no_refill_after_reset(bdt):
    import torch
    from respmon_amd import synth
    from respmon_amd.base import RespiratoryMonitor
    T, H, W = 128, 48, 64
    vid = np.concatenate([synth.synth_breathing(T, H, W, seed=70 + i, center=c, sigma=(0.16, 0.14), amplitude=0.3)
                          for i, c in enumerate(wc.CENTRES)])
    mon = RespiratoryMonitor(capture_target=synth.FakeCapture(vid, fps=10), visualize=None, save_all_data=False,
                             motion_extraction_method="average", run_on_init=False, buffer_dtype=bdt, relocate_every=4)
    assert mon.calibration_buffer_target_length == T
    pushed, refreshed = [], []
    real_push, real_locate = mon._window_push, mon._locate_window

    def push(frames):
        pushed.append(frames.clone())
        real_push(frames)

    def locate():
        roi = real_locate()
        assert roi == RespiratoryMonitor.locate(torch.cat(pushed[-T:]), mon.fps), len(pushed)
        refreshed.append((len(pushed), roi))
        return roi
    mon._window_push, mon._locate_window = push, locate
    mon._add_benchmark_tags()                                   # (run() does; this test drives step() itself)
    steps_after_reset = None
    for i in range(len(vid)):
        frame = mon.next_frame()
        assert frame is not False
        mon.step(frame)
        if refreshed and refreshed[-1][0] == len(pushed) and refreshed[-1][1] is not None and mon.state == 'measure':
            assert (mon.x, mon.y, mon.w, mon.h) == refreshed[-1][1]          # the ROI the monitor holds is the refreshed one
        if i == 300:
            assert mon.state == 'measure'
            mon.reset()
            steps_after_reset = 0
        elif steps_after_reset is not None and steps_after_reset >= 0:
            steps_after_reset += 1
            if steps_after_reset == 2:
                # 'initialize', then ONE calibration frame: the ring is still full, the ROI is there without a refill
                assert mon.state == 'measure' and mon.calibration_buffer_idx == 1, (mon.state, mon.calibration_buffer_idx)
                assert refreshed[-1][0] == len(pushed) and (mon.x, mon.y, mon.w, mon.h) == refreshed[-1][1]
                steps_after_reset = -1
    assert steps_after_reset == -1
    rois = [r for _, r in refreshed]
    assert len(rois) >= (len(vid) - T) // 4 - 3 and None not in rois and len(set(rois)) > 1, rois
    # measured frames between two refreshes: relocate_every (the first refresh follows the first locate() by that many)
    gaps = {b[0] - a[0] for a, b in zip(refreshed, refreshed[1:])}
    assert gaps <= {1, 2, 3, 4} and 4 in gaps, gaps          # (shorter once: the ROI that follows the reset)


# ---- the monitor's refresh in 'flow' mode and under step_clip() ------------------------------------------------------------------
_MOVING = {}


def _moving_video(T=128, H=96, W=128):
    """three segments of T frames, the breathing blob somewhere else in each (made once, read-only)"""
    if not _MOVING:
        from respmon_amd import synth
        v = np.concatenate([synth.synth_breathing(T, H, W, seed=80 + i, center=c, sigma=(0.16, 0.14), amplitude=0.3)
                            for i, c in enumerate(wc.CENTRES)])
        v.setflags(write=False)
        _MOVING["v"] = v
    return _MOVING["v"]


def _relocating_monitor(method, check_against_locate=True):
    """a monitor with relocate_every = 4 over the moving video; -> (monitor, refreshes [(frames pushed, roi)], flow calls
    [(name, rectangle)]).  Every refresh is checked against locate() of the last T frames pushed, however they were grouped."""
    import torch
    from respmon_amd import synth
    from respmon_amd.base import RespiratoryMonitor
    vid = _moving_video()
    mon = RespiratoryMonitor(capture_target=synth.FakeCapture(vid, fps=10), visualize=None, save_all_data=False, error_reset_delay=0,
                             motion_extraction_method=method, run_on_init=False, relocate_every=4)
    T = mon.calibration_buffer_target_length
    pushed, refreshed, flow_calls = [], [], []
    real_push, real_locate = mon._window_push, mon._locate_window

    def push(frames):
        pushed.extend(f.clone() for f in frames)
        real_push(frames)

    def locate():
        roi = real_locate()
        if check_against_locate:
            assert roi == RespiratoryMonitor.locate(torch.stack(pushed[-T:]), mon.fps), len(pushed)
        refreshed.append((len(pushed), roi))
        return roi
    mon._window_push, mon._locate_window = push, locate
    be = mon._backend
    for name in ("flow_begin", "flow_step", "flow_clip"):
        def spy(state, frames, x, y, w, h, _real=getattr(be, name), _name=name, **kw):
            flow_calls.append((_name, (x, y, w, h)))
            return _real(state, frames, x, y, w, h, **kw)
        setattr(be, name, spy)
    mon._add_benchmark_tags()
    return mon, refreshed, flow_calls


def _tracking_follows_the_roi(flow_calls):
    """every rm_flow_step / rm_flow_clip runs on the rectangle of the rm_flow_begin before it; -> the rectangles tracking began on"""
    begun, current = [], None
    for name, rect in flow_calls:
        if name == "flow_begin":
            current = rect
            begun.append(rect)
        else:
            assert rect == current, (name, rect, current)
    return begun


def test_monitor_in_flow_mode_restarts_tracking_on_a_refreshed_roi():
    """relocate_every with motion_extraction_method='flow': a refresh that changes the ROI begins the tracking session again on the
    new rectangle instead of stepping the old session with another crop (RM_E_BADARG when the size changed, stale points when only
    the position did)."""
    vid = _moving_video()
    mon, refreshed, flow_calls = _relocating_monitor("flow")
    held, measured = [], 0
    for i in range(len(vid)):
        frame = mon.next_frame()
        was = (mon.state, (mon.x, mon.y, mon.w, mon.h))
        mon.step(frame)
        now = (mon.x, mon.y, mon.w, mon.h)
        if was[0] == 'measure':
            measured += 1
            if now != was[1]:                                   # a refresh moved the ROI: nothing of the old session is left
                held.append(now)
                assert mon.previous_cropped_image is None and mon.motion_key_points is None and len(mon.motion_data) == 0
    rois = [r for _, r in refreshed]
    assert None not in rois and len(set(rois)) > 1, rois
    assert len({r[2:] for r in rois}) > 1, rois                 # the size changed too: the case rm_flow_step refuses
    assert measured > 0 and len(held) > 1
    begun = _tracking_follows_the_roi(flow_calls)
    assert len(set(begun)) > 1 and set(held) <= set(begun) | {held[-1]}, (held, begun)
    assert any(name == "flow_step" for name, _ in flow_calls)


@pytest.mark.parametrize("method", ["average", "flow"])
def test_monitor_driven_by_clips_refreshes_like_the_frame_by_frame_monitor(method):
    """step_clip() == `for f in frames: step(f)` with relocate_every > 0: the clips' frames reach the ring, the ROI is refreshed behind
    the same frames with the same result (each refresh is locate() of the last T frames, the clips' among them), and the ROI that
    follows a reset() comes from a ring that holds the clips' frames."""
    import torch
    vid = _moving_video()
    RESET_AT = 300
    runs = []
    for clip in (1, 5):                                          # 5: no multiple of relocate_every = 4, so clips are cut
        mon, refreshed, flow_calls = _relocating_monitor(method)
        k = 0
        while k < len(vid):
            stop = RESET_AT if k < RESET_AT else len(vid)        # both runs reset behind the same frame
            n = min(clip, stop - k) if mon.state == 'measure' else 1
            chunk = torch.stack([mon.next_frame() for _ in range(n)])
            if clip == 1:
                mon.step(chunk[0])
            else:
                done = 0
                while done < n:                                  # (step_clip stops behind the frame that leaves 'measure')
                    done += mon.step_clip(chunk[done:])
            k += n
            if k == RESET_AT:
                assert mon.state == 'measure'
                mon.reset()
                before = len(refreshed)
            elif k == RESET_AT + 2:                              # 'initialize', then ONE calibration frame: the ring is still full
                assert mon.state == 'measure' and len(refreshed) == before + 1 and refreshed[-1][1] is not None
        _tracking_follows_the_roi(flow_calls)
        runs.append((refreshed, np.array(mon.data, dtype=np.float64), (mon.x, mon.y, mon.w, mon.h), mon.state))
    (ref1, data1, roi1, state1), (ref5, data5, roi5, state5) = runs
    assert len(ref1) > 10 and len({r for _, r in ref1}) > 1, ref1
    assert ref5 == ref1 and roi5 == roi1 and state5 == state1
    if method == "average":
        # the same pixels averaged per frame or per clip: float64 sums of at most H * W values below 256, so within H * W ulps
        assert data1.shape == data5.shape and np.allclose(data5, data1, rtol=96 * 128 * 2.3e-16, atol=0)
