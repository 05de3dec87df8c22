"""Whole-clip motion extraction on the GPU (rm_roi_mean_clip, rm_flow_clip, rm_pca_reduce_windows, RespiratoryMonitor.step_clip,
run() with measure_clip_length > 1) at real sizes, against the per-frame entry points bit for bit (np.array_equal, NaN at the same
positions).  The host-emulated twin with the edge cases and the oracle comparison is tests/test_emu_flow_clip.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LK = ((15, 15), 2, (3, 10, 0.03))


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd.base import _Backend
    return _Backend()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _slot_bytes(h, w, win=(15, 15), lvl=2):
    """include/respmon_hip_debug.h "flow_clip_bytes": 5 bytes per pixel of every LK pyramid level of the ROI"""
    top, sh, sw = lvl, h, w
    for l in range(lvl + 1):
        sw, sh = (sw + 1) // 2, (sh + 1) // 2
        if sw <= win[0] or sh <= win[1]:
            top = l
            break
    n, sh, sw = 0, h, w
    for _ in range(top + 1):
        n += sh * sw * 5
        sh, sw = (sh + 1) // 2, (sw + 1) // 2
    return n


def _steps(be, frames, roi, begin):
    st = be.flow_state()
    pts = be.flow_begin(st, frames[0], *roi, *begin)
    out = [be.flow_step(st, frames[i], *roi, *LK) for i in range(1, len(frames))]
    return pts, np.array([m for m, _ in out], np.float32), np.array([n for _, n in out]), be.flow_points(st, begin[0]), st


def _clips(be, frames, roi, begin, sizes):
    st = be.flow_state()
    pts = be.flow_begin(st, frames[0], *roi, *begin)
    means, ngs, t = [], [], 1
    for k in sizes:
        m, ng = be.flow_clip(st, frames[t:t + k], *roi, *LK)
        means.append(m); ngs.append(ng)
        t += k
    return pts, np.concatenate(means), np.concatenate(ngs), be.flow_points(st, begin[0]), st


def _check_clip_equals_steps(be, frames, roi, begin, min_points):
    from respmon_amd import device
    n = len(frames) - 2                    # the last frame is kept for one further step from each state
    want = _steps(be, frames[:n + 1], roi, begin)
    assert want[0] is not None and len(want[0]) >= min_points and want[2][-1] > 0
    nxt = be.flow_step(want[4], frames[n + 1], *roi, *LK)
    for chunk_frames, sizes in ((0, [n]), (0, [n // 3, n - n // 3]), (5, [n]), (1, [n])):
        device.debug_set("flow_clip_bytes", (chunk_frames + 1) * _slot_bytes(roi[3], roi[2]) if chunk_frames else 0)
        try:
            got = _clips(be, frames[:n + 1], roi, begin, sizes)
        finally:
            device.debug_set("flow_clip_bytes", 0)
        assert np.array_equal(got[0], want[0]), (chunk_frames, sizes)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (chunk_frames, sizes)
        assert np.array_equal(got[3], want[3]), (chunk_frames, sizes)
        m, ng = be.flow_step(got[4], frames[n + 1], *roi, *LK)
        assert np.array_equal(m, nxt[0]) and ng == nxt[1], (chunk_frames, sizes)
    return want


def test_flow_clip_on_the_located_roi_1080p(be):
    """64 frames, the reference's 100 corners on the ROI locate() finds on the 1080p synthetic stream, uint8 and float64 frames."""
    import torch
    from respmon_amd import synth
    from respmon_amd.base import RespiratoryMonitor
    v8 = synth.synth_breathing(256, 1080, 1920, seed=1234)
    roi = RespiratoryMonitor.locate(torch.from_numpy(v8).cuda(), 10)
    assert roi is not None and roi[2] > 200 and roi[3] > 150
    u8 = _dev(v8[:66])
    a = _check_clip_equals_steps(be, u8, roi, (100, 0.3, 7, 7), 20)
    f64 = u8.double() * (1. / 255)
    b = _check_clip_equals_steps(be, f64, roi, (100, 0.3, 7, 7), 20)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])      # base.py:231 then :364: the same crops
    # the ROI mean of the same clips
    for frames in (u8, f64, f64.float(), f64.half()):
        for r in (roi, (0, 0, 1920, 1080), (1919, 1079, 1, 1)):
            want = np.array([be.roi_mean(frames[i], *r) for i in range(0, len(frames), 7)])
            assert np.array_equal(be.roi_mean_clip(frames, *r)[::7], want), (frames.dtype, r)


def test_flow_clip_1000_points(be):
    """BASELINE config 3 (bench.py config F): 256x256, 1 000 points (qualityLevel 0.01, minDistance 3)."""
    from respmon_amd import synth
    render = synth.synth_texture(256, 256, seed=4321)
    frames = _dev(np.stack([render(1.5 * np.sin(2 * np.pi * 0.4 * t / 30), 0.5 * np.sin(2 * np.pi * 0.4 * t / 30 + np.pi / 3)) for t in range(66)]))
    want = _check_clip_equals_steps(be, frames, (0, 0, 256, 256), (1000, 0.01, 3, 7), 1000)
    assert want[2][0] >= 950


def test_flow_clip_while_points_are_lost(be):
    """Large shifts push corners out of a small ROI, then a flat frame loses the rest: n_good falls to 0 inside the clip and stays
    there although textured frames follow."""
    from respmon_amd import synth
    render = synth.synth_texture(120, 160, seed=11)
    frames = np.stack([render(40.0 * np.sin(2 * np.pi * 0.4 * t / 10), 24.0 * np.sin(2 * np.pi * 0.4 * t / 10 + 1.0)) for t in range(36)])
    frames[20] = 9
    frames = _dev(frames)
    roi, begin = (50, 40, 24, 20), (100, 0.3, 7, 7)
    want = _steps(be, frames, roi, begin)
    assert want[2][0] > 0 and want[2][18] > 0 and not want[2][22:].any()
    for sizes in ([35], [10, 25]):
        got = _clips(be, frames, roi, begin, sizes)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and len(got[3]) == 0


def test_pca_reduce_windows(be, golden):
    rng = np.random.default_rng(5)
    for n in (1, 2, 5, 128, 129, 300):
        md = (rng.standard_normal((n, 2)) * rng.uniform(0.01, 2, 2) + rng.uniform(-1, 1, 2)).astype(np.float32)
        for first, window in ((0, 128), (0, 5), (n // 2, 128), (n // 2, 5)):
            want = np.array([be.pca_reduce(md[max(0, j + 1 - window):j + 1]) if j >= 1 else 0.0 for j in range(first, n)])
            assert np.array_equal(be.pca_reduce_windows(md, first, window), want), (n, first, window)
    g = golden("g5_extract_motion.npz")
    md, vals = g["motion_data_f32"], g["values"]
    got = be.pca_reduce_windows(md, 1, len(md))
    for k in range(2, len(md) + 1):
        assert abs(got[k - 2] - vals[k]) <= 1e-9 * max(1.0, abs(vals[k]))


def _monitor(frames, method, roi, **attrs):
    from respmon_amd import synth
    from respmon_amd.base import RespiratoryMonitor
    mon = RespiratoryMonitor(capture_target=synth.FakeCapture(frames, fps=10), visualize=None, save_all_data=True,
                             motion_extraction_method=method, run_on_init=False)
    mon.sync_to_fps = lambda: None
    for k, v in attrs.items():
        setattr(mon, k, v)
    mon.skip_calibration(*roi)
    return mon


def _assert_same_monitor(a, b):
    def arr(v):
        return np.array(v, dtype=np.float64)
    for name in ("data", "t", "freq", "filtered_data", "peak_indices", "peak_times"):
        assert np.array_equal(arr(getattr(a, name)), arr(getattr(b, name)), equal_nan=True), name
    assert [x is np.nan for x in a.data] == [x is np.nan for x in b.data]
    assert np.array_equal(np.array(a.motion_data, np.float32), np.array(b.motion_data, np.float32))
    assert np.array_equal(arr(a.all_data), arr(b.all_data), equal_nan=True)
    assert a.state == b.state and a.error_message == b.error_message
    assert a.previous_cropped_image is b.previous_cropped_image
    pa, pb = a.motion_key_points, b.motion_key_points
    assert (pa is None) == (pb is None) and (pa is None or np.array_equal(pa, pb))


@pytest.mark.parametrize("method", ["average", "flow"])
def test_step_clip_equals_the_step_loop(be, method):
    from respmon_amd import synth
    render = synth.synth_texture(480, 640, seed=7)
    frames = np.stack([render(1.5 * np.sin(2 * np.pi * 0.4 * t / 10), 0.5 * np.sin(2 * np.pi * 0.4 * t / 10 + 1.0)) for t in range(60)])
    roi = (120, 90, 351, 235)
    loop = _monitor(frames, method, roi, measure_buffer_length=16)
    loop.run()
    assert len(loop.data) == 16 and len(loop.all_data) == 60
    one = _monitor(frames, method, roi, measure_buffer_length=16)
    assert one.step_clip(frames) == 60                                  # a numpy clip goes to the device
    _assert_same_monitor(one, loop)
    split = _monitor(frames, method, roi, measure_buffer_length=16)
    dev = _dev(frames)
    assert split.step_clip(dev[:1]) == 1 and split.step_clip(dev[1:23]) == 22 and split.step_clip(dev[23:]) == 37
    _assert_same_monitor(split, loop)
    clips = _monitor(frames, method, roi, measure_buffer_length=16, measure_clip_length=8)
    clips.run()
    _assert_same_monitor(clips, loop)


def test_step_clip_stops_where_tracking_is_lost(be):
    from respmon_amd import synth
    render = synth.synth_texture(120, 160, seed=11)
    frames = np.stack([render(1.5 * np.sin(0.5 * t), 0.7 * np.cos(0.4 * t)) for t in range(30)])
    frames[20] = 9
    roi = (30, 20, 90, 70)
    loop = _monitor(frames, "flow", roi)
    loop.run()
    n = len(loop.data)
    assert loop.state == 'error' and 20 < n < 30 and loop.data[-1] is np.nan
    clip = _monitor(frames, "flow", roi)
    assert clip.step_clip(frames) == n
    _assert_same_monitor(clip, loop)


def test_run_with_clips_leaves_the_g6_trace(be, golden):
    """run() with measure_clip_length = 8 on the scripted capture of the G6 trace: the same data / t as frame by frame."""
    from respmon_amd import synth
    from respmon_amd.base import RespiratoryMonitor
    g = golden("g6_run_trace.npz")
    vid = synth.synth_breathing(150, 48, 64, seed=11)
    mons = []
    for k in (1, 8):
        mon = RespiratoryMonitor(capture_target=synth.FakeCapture(vid, fps=30), visualize=None, save_all_data=False,
                                 motion_extraction_method="average", run_on_init=False)
        mon.sync_to_fps = lambda: None
        mon.measure_clip_length = k
        mon.run()
        mons.append(mon)
        assert [mon.x, mon.y, mon.w, mon.h] == [int(v) for v in g["c2_roi"]]
        assert np.allclose(np.array(mon.data), g["c2_data"], rtol=1e-13, atol=0) and np.array_equal(np.array(mon.t), g["c2_t"])
    assert np.array_equal(np.array(mons[0].data), np.array(mons[1].data)) and np.array_equal(np.array(mons[0].t), np.array(mons[1].t))
