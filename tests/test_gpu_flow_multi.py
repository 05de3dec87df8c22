"""Several subjects by optical flow in one call per clip on the GPU (rm_flow_multi_clip, rm_pca_reduce_windows_multi,
SubjectTracker(motion_extraction_method='flow')) at real sizes, against the per-subject calls bit for bit: the per-frame
rm_flow_step loop is the reference, rm_flow_clip (the K = 1 entry of the same driver) is compared with it as the multi call is;
the windowed PCA of several lists against rm_pca_reduce window by window.  The cases and the comparison are those of
tests/flow_multi_cases.py; the host-emulated twin with the refusals is tests/test_emu_flow_multi.py."""
import numpy as np
import pytest

from tests import flow_multi_cases as fm
from tests.flow_multi_cases import BEGIN, ROIS_EMU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd.base import _Backend
    return fm.GpuApi(_Backend())


def _texture_clip(H, W, n, seed):
    from respmon_amd import synth
    render = synth.synth_texture(H, W, seed=seed)
    return np.stack([render(1.5 * np.sin(2 * np.pi * 0.4 * t / 30), 0.5 * np.sin(2 * np.pi * 0.4 * t / 30 + np.pi / 3)) for t in range(n)])


@pytest.mark.parametrize("dtype", ["uint8", "float64"])
def test_flow_multi_real_sizes(api, dtype):
    """480 x 640, 24 frames, four subjects with 3, 3, 3 and 1 LK levels, 100 corners and 1 000 points: one call against the
    per-subject clips and the per-frame steps, unchunked and with 5 and 1 frames per chunk."""
    frames = api.dev(_texture_clip(480, 640, 26, seed=4321))
    if dtype == "float64":
        frames = frames.double() * (1. / 255)
    rois = [(140, 120, 351, 235), (20, 30, 90, 70), (380, 10, 256, 256), (300, 400, 24, 20)]
    begins = [BEGIN, BEGIN, (1000, 0.01, 3, 7), BEGIN]
    caps = [100, 100, 1000, 100]
    assert [fm.lk_levels(r[3], r[2]) for r in rois] == [3, 3, 3, 1]
    steps = fm.run(api, frames, rois, [("step", 24)], begins, caps)
    assert len(steps["pts0"][0]) == 100 and len(steps["pts0"][2]) >= 950 and all(p is not None for p in steps["pts0"])
    assert (steps["n_good"][-1] > 0).all()
    clips = fm.run(api, frames, rois, [("clip", 24)], begins, caps)
    fm.assert_same(clips, steps, "clips against steps")
    for per_chunk, schedule in ((0, [("multi", 24)]), (0, [("multi", 9), ("step", 1), ("multi", 14)]), (5, [("multi", 24)]), (1, [("multi", 24)])):
        api.set_bytes(fm.chunk_bytes(rois, per_chunk) if per_chunk else 0)
        try:
            got = fm.run(api, frames, rois, schedule, begins, caps)
        finally:
            api.set_bytes(0)
        fm.assert_same(got, steps, (per_chunk, schedule))
    fm.assert_same_next_step(api, frames[25], rois, [got, clips], steps)


def test_flow_multi_1080p_16_subjects(api):
    """the stride arithmetic at frame scale: 1080p uint8, 12 frames, 16 overlapping rectangles of 351 x 235"""
    frames = api.dev(_texture_clip(1080, 1920, 13, seed=7))
    rois = fm.grid_rois(16, 1080, 1920)
    loop = fm.run(api, frames, rois, [("step", 12)])
    assert all(p is not None and len(p) >= 20 for p in loop["pts0"]) and (loop["n_good"][-1] > 0).all()
    fm.assert_same(fm.run(api, frames, rois, [("multi", 12)]), loop, "multi")
    fm.assert_same(fm.run(api, frames, rois, [("clip", 12)]), loop, "clip")


def test_flow_multi_both_finish_paths(api):
    """a subject with more points than the LDS staging of the finish holds (FLOW_FINISH_MAX = 6000) beside a 100-corner subject"""
    from tests import test_gpu_motion_edges as me
    H, W = 1080, 1440
    render = me._smooth_noise(H, W, seed=11)
    frames = api.dev(np.stack([render(0.3 * t, -0.2 * t) for t in range(4)]))
    rois = [(0, 0, W, H), (100, 200, 351, 235)]
    begins, caps = [(6100, 0.001, 1, 7), BEGIN], [6100, 100]
    loop = fm.run(api, frames, rois, [("step", 3)], begins, caps)
    assert len(loop["pts0"][0]) == 6100 and len(loop["pts0"][1]) == 100 and (loop["n_good"][-1] > [3000, 50]).all()
    fm.assert_same(fm.run(api, frames, rois, [("multi", 3)], begins, caps), loop, "multi")
    fm.assert_same(fm.run(api, frames, rois, [("multi", 1), ("multi", 2)], begins, caps), loop, "multi 1 + 2")
    fm.assert_same(fm.run(api, frames, rois, [("clip", 3)], begins, caps), loop, "clip")


def test_flow_multi_unequal_lives(api):
    f = fm.frames_unequal_lives()
    rois = [ROIS_EMU[0], ROIS_EMU[2], ROIS_EMU[1]]
    frames = api.dev(f)
    begins = [BEGIN, BEGIN, api.dev(np.full_like(f[0], 9))]
    loop = fm.run(api, frames, rois, [("step", 7)], begins)
    ng = loop["n_good"]
    assert loop["pts0"][2] is None and ng[3, 0] > 0 and not ng[4:, 0].any() and ng[-1, 1] > 0 and not ng[:, 2].any()
    for per_chunk in (0, 2):
        api.set_bytes(fm.chunk_bytes(rois[:2], per_chunk) if per_chunk else 0)
        try:
            for schedule in ([("multi", 7)], [("multi", 4), ("multi", 3)]):
                got = fm.run(api, frames, rois, schedule, begins)
                fm.assert_same(got, loop, (per_chunk, schedule))
        finally:
            api.set_bytes(0)
    clips = fm.run(api, frames, rois, [("clip", 7)], begins)
    fm.assert_same(clips, loop, "clip")
    fm.assert_same_next_step(api, frames[8], rois, [got, clips], loop)


def test_flow_clip_alternating_states_share_the_context(api):
    fm.check_alternating_one_subject_clips(api, api.dev(fm.frames_emu(1.0)))


def test_pca_reduce_windows_multi(api):
    fm.check_pca_windows_multi(api)


def _monitor(frames, roi):
    from respmon_amd import synth
    from respmon_amd.base import RespiratoryMonitor
    mon = RespiratoryMonitor(capture_target=synth.FakeCapture(frames, fps=10), visualize=None, save_all_data=True,
                             motion_extraction_method="flow", run_on_init=False)
    mon.sync_to_fps = lambda: None
    mon.measure_buffer_length = 16
    mon.skip_calibration(*roi)
    return mon


@pytest.mark.parametrize("on_device", [False, True])
def test_tracker_flow_equals_monitors(api, on_device):
    from respmon_amd.subjects import SubjectTracker
    frames = fm.tracker_frames()
    clip = api.dev(frames) if on_device else frames
    mons = []
    for roi in ROIS_EMU[:3]:
        mon = _monitor(frames, roi)
        mon.step_clip(clip)
        mons.append(mon)
    assert mons[0].state == 'error' and len(mons[0].all_data) == 22 and mons[1].state == mons[2].state == 'measure'
    for sizes in ([30], [1, 7, 22]):
        tr = SubjectTracker(ROIS_EMU[:3], 10, measure_buffer_length=16, save_all_data=True, motion_extraction_method='flow')
        fm.step_in_clips(tr, clip, sizes)
        assert tr.lost == [True, False, False]
        for k in range(3):
            fm.assert_subject_equals_monitor(tr[k], tr.motion_key_points(k), mons[k], (sizes, k))
    more = fm.tracker_frames(30, lost_at=29)[:12]
    tr.restart(0)
    fm.step_in_clips(tr, api.dev(more) if on_device else more, [5, 7])
    mon = _monitor(more, ROIS_EMU[0])
    mon.step_clip(api.dev(more) if on_device else more)
    assert not tr[0].lost and np.array_equal(np.array(tr[0].data), np.array(mon.data)) and len(tr[0].data) == 12
    assert np.array_equal(tr.motion_key_points(0), mon.motion_key_points) and len(tr[1].all_data) == 42
