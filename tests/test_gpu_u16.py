"""uint16 frame buffers (RM_U16, include/respmon_hip.h) on the MI355X: the checks of tests/u16_cases.py on the device at the shapes of
test_fused_down_chain_equals_per_level / test_bgr_frame_buffer_equals_its_gray_buffer (tests/test_gpu_calibration.py), and the Python
layer -- locate, the monitor with buffer_dtype='uint16', the sliding window, the live magnifier, the rate map, several subjects --
against the same calls on the float64 frames k * (1./65535).  Every comparison is exact.  The host-emulated twin is
tests/test_emu_u16.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import u16_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device

    class B:
        lib = _capi.load()
        ctx = device.ctx()
        stream = staticmethod(device.stream_ptr)
        dev = staticmethod(lambda a: torch.from_numpy(np.array(a, order="C")).cuda())      # (a copy: the shared videos are read-only arrays)
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        np = staticmethod(lambda t: t.cpu().numpy())
    return B


@pytest.fixture(scope="module")
def identity(be):
    return uc.check_conversions(be)


def same(a, b):
    """torch.equal for tensors whose dtype it may refuse on the device: uint16 compares through its bits"""
    import torch
    if a.dtype == torch.uint16:
        return b.dtype == torch.uint16 and torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a, b)


def test_u16_conversions(be, identity):
    import torch
    from respmon_amd import transforms
    k = np.arange(65536, dtype=np.uint16)
    f = transforms.uint16_to_float(k)
    assert f.dtype == np.float64 and np.array_equal(f, k * uc.SCALE)
    back = transforms.float_to_uint16(f)
    assert back.dtype == np.uint16 and np.array_equal(back, identity)
    assert same(transforms.float_to_uint16(torch.from_numpy(f).cuda()), torch.from_numpy(identity).cuda())


SHAPES = [(3, 64, 96, 4, 2), (2, 67, 131, 5, 3), (2, 135, 240, 6, 4), (8, 360, 640, 4, 2), (4, 540, 1936, 8, 4), (3, 300, 2000, 6, 3),
          (5, 97, 1936, 4, 1), (16, 1080, 1920, 9, 4)]      # the last: the headline geometry at 16 frames


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_u16_calibration_equals_the_f64_buffer(be, shape):
    uc.check_calibration(be, *shape)


def test_u16_every_level_at_depth_1(be):
    uc.check_calibration(be, 1, 256, 256, 3, 1, frames=uc.every_level())


@pytest.mark.parametrize("shape", SHAPES[:3] + [(9, 32, 48, 4, 2)], ids=str)
def test_u16_flags_against_one_another(be, shape):
    uc.check_flags_against_one_another(be, *shape)


def test_u16_locate_oracle_and_sample_alignment(be):
    uc.check_locate_oracle(be, 32, 96, 128, 4, 2)


def test_u16_roi_means_crops_and_flow_clip(be):
    uc.check_motion(be)
    uc.check_flow_clip(be)


@pytest.mark.parametrize("shape", [(5, 40, 80, 5, 3), (4, 70, 70, 7, 5), (6, 135, 240, 6, 2)], ids=str)
def test_u16_magnify(be, identity, shape):
    uc.check_magnify(be, *shape, identity=identity)


def test_u16_magnify_clamps_and_stream_pushes(be):
    uc.check_magnify_clamp(be)
    uc.check_stream(be)


def test_u16_arguments(be):
    uc.check_arguments(be)


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_u16_locate_on_a_device_tensor_and_a_host_array_equals_the_oracle():
    import torch
    from oracle import respmon_oracle as oracle
    from respmon_amd import device
    from respmon_amd.base import RespiratoryMonitor
    v = uc.breathing16(64, 270, 480, 16, seed=7).copy()
    kw = dict(pyramid_levels=6, skip_levels_at_top=2)
    ref = oracle.locate(uc.widen(v), 10, **kw)
    assert ref is not None
    d = torch.from_numpy(v.copy()).cuda()
    assert d.dtype == torch.uint16 and device.dtype_code(d) == _capi.RM_U16
    assert RespiratoryMonitor.locate(d, 10, **kw) == tuple(ref)
    assert RespiratoryMonitor.locate(v, 10, **kw) == tuple(ref)             # a numpy uint16 array uploads as it is
    assert RespiratoryMonitor.locate_all(d, 10, max_rois=3, **kw)[0] == tuple(ref)


def _monitor(video, bdt, method, T=32):
    from respmon_amd import synth
    from respmon_amd.base import RespiratoryMonitor
    mon = RespiratoryMonitor(capture_target=synth.FakeCapture(video, fps=10), visualize=None, save_all_data=False, error_reset_delay=0,
                             motion_extraction_method=method, run_on_init=False, buffer_dtype=bdt)
    mon.calibration_buffer_target_length = T
    mon.calibration_buffer = mon._alloc_buffer()
    mon._add_benchmark_tags()
    return mon


@pytest.mark.parametrize("method", ["average", "flow"])
def test_u16_monitor_equals_the_f64_monitor_fed_the_same_capture(method):
    import torch
    T = 32
    v = uc.breathing16(1 + T + 1 + 40, 96, 128, 16, seed=31).copy()
    runs = {}
    for bdt in ("uint16", "float64"):
        mon = _monitor(v, bdt, method, T)
        states = []
        for _ in range(len(v)):
            frame = mon.next_frame()
            assert frame.dtype == torch.uint16 and frame.dim() == 2 and frame.is_cuda        # Y16: no cvtColor, uint16 on the device
            states.append(mon.state)
            mon.step(frame)
        assert mon.calibration_buffer.dtype == (torch.uint16 if bdt == "uint16" else torch.float64)
        assert np.array_equal(mon.current_frame, v[-1] * uc.SCALE)
        runs[bdt] = (states, (mon.x, mon.y, mon.w, mon.h), np.array(mon.data, dtype=np.float64), mon.state, mon.calibration_buffer)
    a, b = runs["uint16"], runs["float64"]
    assert a[0] == b[0] and a[0].count("measure") == 40 and a[3] == "measure"
    assert a[1] == b[1] and None not in a[1]
    assert len(a[2]) == 40 and np.array_equal(a[2], b[2], equal_nan=True) and np.isfinite(a[2]).any()
    assert np.array_equal(a[4].cpu().numpy() * uc.SCALE, b[4].cpu().numpy())                 # the two buffers hold the same frames
    if method == "average":
        assert np.ptp(a[2]) > 0


def test_u16_monitor_clip_steps_rate_map_magnified_video_and_locate_all():
    import torch
    from respmon_amd.base import RespiratoryMonitor
    T = 32
    v = uc.breathing16(1 + T + 1 + 40, 96, 128, 16, seed=31).copy()
    mons = {bdt: _monitor(v, bdt, "average", T) for bdt in ("uint16", "float64")}
    for mon in mons.values():
        for _ in range(1 + T + 1):
            mon.step(mon.next_frame())
        assert mon.state == "measure"
        clip = torch.stack([mon.next_frame().view(torch.int16) for _ in range(12)]).view(torch.uint16)     # (stacked through the bits)
        assert clip.dtype == torch.uint16 and mon.step_clip(clip) == 12
    m16, m64 = mons["uint16"], mons["float64"]
    assert np.array_equal(np.array(m16.data), np.array(m64.data)) and len(m16.data) == 12
    r16, r64 = m16.rate_map(level=2), m64.rate_map(level=2)
    for name in ("freq", "power", "total", "index"):
        x, y = getattr(r16, name).cpu().numpy(), getattr(r64, name).cpu().numpy()
        assert np.array_equal(x, y, equal_nan=True), name
    assert (r16.index.cpu().numpy() >= 0).any()
    mag = m16.magnified_calibration_video()
    assert mag.dtype == torch.uint16                                                      # uint16 out for a uint16 buffer
    assert np.array_equal(mag.cpu().numpy(), uc.u16_of(m64.magnified_calibration_video().cpu().numpy()))
    assert RespiratoryMonitor.locate_all(m16.calibration_buffer, 10, max_rois=3) == RespiratoryMonitor.locate_all(m64.calibration_buffer, 10, max_rois=3)


def test_u16_frames_and_8_bit_buffers_refuse_each_other():
    from respmon_amd import synth
    v16 = uc.breathing16(4, 96, 128, 16, seed=31).copy()
    v8 = synth.synth_breathing(4, 96, 128, seed=31)
    for video, bdt in ((v16, "uint8"), (v16, "bgr8"), (v8, "uint16")):
        mon = _monitor(video, bdt, "average")
        mon.step(mon.next_frame())                       # 'initialize'
        with pytest.raises(TypeError) as e:
            mon.step(mon.next_frame())
        assert "uint16" in str(e.value) and ("uint8" in str(e.value) or "bgr8" in str(e.value)), str(e.value)
    for bdt in ("float32",):                             # a narrower float buffer takes the frame, rounded once from the float64 value
        import torch
        mon = _monitor(v16, bdt, "average")
        mon.step(mon.next_frame())
        mon.step(mon.next_frame())
        want = torch.from_numpy(v16[1] * uc.SCALE).to(mon.calibration_buffer.dtype)
        assert torch.equal(mon.calibration_buffer[0].cpu(), want)


def test_u16_sliding_window_live_magnifier_and_rate_map():
    import torch
    from respmon_amd import rate
    from respmon_amd.live import LiveMagnifier
    from respmon_amd.window import SlidingCalibration
    H, W, T = 135, 240, 16
    v = uc.breathing16(40, H, W, 16, seed=33).copy()
    f = uc.widen(v)
    kw = dict(pyramid_levels=5, skip_levels_at_top=2)
    wins = [SlidingCalibration(T, H, W, **kw) for _ in range(2)]
    try:
        for k in range(0, len(v), 5):                                # groups of 5: the ring wraps inside a push
            wins[0].push(v[k:k + 5] if k % 2 == 0 else torch.from_numpy(v[k:k + 5].copy()).cuda())
            wins[1].push(f[k:k + 5])
        assert wins[0].count == T and wins[0].head == wins[1].head
        assert torch.equal(wins[0].heatmap(10), wins[1].heatmap(10))
        assert wins[0].locate(10) == wins[1].locate(10) is not None
        ra, rb = wins[0].rate_map(10), wins[1].rate_map(10)
        for name in ("freq", "power", "total", "index"):
            assert np.array_equal(getattr(ra, name).cpu().numpy(), getattr(rb, name).cpu().numpy(), equal_nan=True), name
    finally:
        for w in wins:
            w.close()
    r16, r64 = rate.buffer_rate_map(v[:T], 10, level=2), rate.buffer_rate_map(f[:T], 10, level=2)
    for name in ("freq", "power", "total", "index"):
        assert np.array_equal(getattr(r16, name).cpu().numpy(), getattr(r64, name).cpu().numpy(), equal_nan=True), name
    with LiveMagnifier(H, W, 10, **kw) as m16, LiveMagnifier(H, W, 10, out_dtype="float64", **kw) as m64:
        out16 = np.concatenate([m16.push(v[a:b]) for a, b in ((0, 3), (3, 4), (4, 17))])
        out64 = np.concatenate([m64.push(f[a:b]) for a, b in ((0, 9), (9, 17))])
        assert out16.dtype == np.uint16 and np.array_equal(out16, uc.u16_of(out64))
        one = m16.push(torch.from_numpy(v[17].copy()).cuda())          # a single device frame: uint16 in, uint16 out
        assert one.dtype == torch.uint16 and tuple(one.shape) == (H, W)
        assert np.array_equal(one.cpu().numpy(), uc.u16_of(m64.push(f[17])))


@pytest.mark.parametrize("method", ["average", "flow"])
def test_u16_subject_tracker_equals_the_f64_clip(method):
    from respmon_amd.subjects import SubjectTracker
    v = uc.flow_clip_video()
    clip = np.concatenate([v, v[::-1][1:4]])                             # 8 frames (a writable copy)
    assert len(clip) == 8
    rois = [(21, 13, 80, 64), (3, 40, 41, 33)]
    out = []
    for frames in (clip, uc.widen(clip)):
        tr = SubjectTracker(rois, 10, motion_extraction_method=method)
        assert tr.step_clip(frames) == 8
        out.append(([np.array(s.data, dtype=np.float64) for s in tr.subjects], tr.lost,
                    [tr.motion_key_points(k) for k in range(2)] if method == "flow" else None))
    (d16, lost16, p16), (d64, lost64, p64) = out
    assert lost16 == lost64
    for a, b in zip(d16, d64):
        assert len(a) == 8 and np.array_equal(a, b, equal_nan=True)
    if method == "flow":
        for a, b in zip(p16, p64):
            assert a is not None and len(a) >= 4 and np.array_equal(a, b)
