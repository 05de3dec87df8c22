"""The pulse path (include/respmon_hip.h rm_bgr_block_sums / rm_bgr_roi_sums / rm_pulse_pos / rm_pulse_map, respmon_amd/pulse.py) on
the MI355X: the cases of tests/pulse_cases.py -- exact block and rectangle sums in both forms of the kernel, POS bit for bit against the
scalar restatement, rm_pulse_map against its three parts, the pulse under a flickering lamp, every refusal -- and the Python layer.
The host-emulated twin, with the library-free checks of the references, is tests/test_emu_pulse.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import pulse_cases as pc
from tests import pulse_reference as pr
from tests import rate_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device
    side = torch.cuda.Stream()

    def dev(a, offset=0):
        a = np.ascontiguousarray(a)
        raw = torch.empty(a.nbytes + offset, dtype=torch.uint8, device="cuda")     # (allocations are 256-byte aligned)
        view = raw[offset:]
        view.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
        assert view.data_ptr() % 16 == offset % 16
        return view

    class B:
        lib = _capi.load()
        ctx = device.ctx()
        stream = staticmethod(device.stream_ptr)
        other_stream = staticmethod(lambda: ctypes.c_void_p(side.cuda_stream))
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        out = staticmethod(lambda shape: torch.full(tuple(shape), float("nan"), dtype=torch.float64, device="cuda"))
        out_i32 = staticmethod(lambda shape: torch.full(tuple(shape), -7, dtype=torch.int32, device="cuda"))
        np = staticmethod(lambda t: t.cpu().numpy())
        fill = staticmethod(lambda nbytes: torch.full((nbytes,), pc.SENTINEL, dtype=torch.uint8, device="cuda"))
        get = staticmethod(lambda buf, dtype, shape: buf.cpu().numpy().view(dtype).reshape(shape))
    B.dev = staticmethod(dev)
    return B


@pytest.mark.parametrize("N", (1, 3))
@pytest.mark.parametrize("block", pc.BLOCKS)
@pytest.mark.parametrize("shape", pc.SHAPES, ids=str)
def test_block_sums_exact(be, shape, block, N):
    pc.check_block_sums(be, shape[0], shape[1], block, N)


@pytest.mark.parametrize("block", (8, 32))
def test_block_sums_exact_at_the_other_block_sizes(be, block):
    for H, W in ((17, 37), (33, 64), (5, 1040)):
        pc.check_block_sums(be, H, W, block, 3)


def test_block_sums_of_a_view_one_byte_into_its_allocation(be):
    pc.check_block_sums_misaligned(be)


def test_roi_sums_exact(be):
    pc.check_roi_sums(be)


@pytest.mark.parametrize("N,l", pc.pos_cases())
def test_pos_bit_for_bit(be, N, l):
    pc.check_pos(be, N, l)


@pytest.mark.parametrize("N", (9, 16))
@pytest.mark.parametrize("geom", pc.MAP_GEOMS, ids=str)
def test_pulse_map_equals_its_three_parts(be, geom, N):
    pc.check_map_equals_parts(be, geom, N)


@pytest.mark.parametrize("seed", pc.PURPOSE_SEEDS)
def test_purpose_pulse_under_a_flickering_lamp(be, seed):
    print("purpose, library, seed %d: %s" % (seed, pc.check_purpose(be, seed)))


def test_pulse_argument_errors(be):
    pc.check_argument_errors(be)


def test_pulse_is_refused_while_a_submission_is_in_flight_on_another_stream(be):
    pc.check_busy(be)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_python_sums_and_pos(be):
    import torch
    from respmon_amd import pulse
    frames = pc.block_inputs(3, 40, 129)[0][1]
    dev = torch.from_numpy(np.array(frames)).cuda()
    for src in (np.array(frames), dev):
        s = pulse.block_sums(src, block=16)
        assert isinstance(s, torch.Tensor) and s.is_cuda and s.dtype == torch.uint32 and tuple(s.shape) == (3, 3, 9, 3)
        assert np.array_equal(s.cpu().numpy().astype(np.uint64), pr.block_sums(frames, 16))
    assert tuple(pulse.block_sums(dev).shape) == (3, 3, 9, 3)                     # block defaults to 16
    rois = [(0, 0, 129, 40), (16, 16, 16, 16), (128, 39, 1, 1)]
    r = pulse.roi_sums(dev, rois)
    assert r.is_cuda and r.dtype == torch.uint32 and np.array_equal(r.cpu().numpy().astype(np.uint64), pr.roi_sums(frames, rois))
    sums = pc.pos_inputs(9, 5)
    h = pulse.pos(torch.from_numpy(np.array(sums)).cuda(), 5)
    assert h.is_cuda and h.dtype == torch.float64 and pc.same_bits(h.cpu().numpy(), pc.pos_reference(9, 5))
    h4 = pulse.pos(np.array(sums).reshape(9, 10, 13, 3), 5)                        # [N, ..., 3] -> [N, ...]
    assert tuple(h4.shape) == (9, 10, 13) and pc.same_bits(h4.cpu().numpy().reshape(9, 130), pc.pos_reference(9, 5))
    with pytest.raises(ValueError):
        pulse.block_sums(dev, block=12)
    with pytest.raises(ValueError, match="gray"):
        pulse.block_sums(dev[..., 0])
    with pytest.raises(_capi.RespmonError):
        pulse.roi_sums(dev, [(100, 0, 40, 4)])


def test_python_pulse_map_signal_and_rate(be):
    import torch
    from respmon_amd import pulse, rate
    from respmon_amd.base import RespiratoryMonitor
    P = pc.PURPOSE
    clip = np.array(pc.purpose_clip(pc.PURPOSE_SEEDS[0]))
    want = pc.pulse_map(be, clip, P["block"], P["window"], P["fps"], P["fmin"], P["fmax"], P["F"])
    pm = pulse.pulse_map(clip, P["fps"], window=P["window"])
    assert isinstance(pm, rate.RateMap) and pm.level == 4 and tuple(pm.freq.shape) == (4, 4) and pm.index.dtype == torch.int32
    rc.same_outputs([v.cpu().numpy().reshape(-1) for v in (pm.freq, pm.power, pm.total, pm.index)], want, "pulse_map")
    assert pulse.pulse_map(clip, P["fps"], block=8, window=P["window"]).level == 3
    # window=None is the paper's 1.6 s
    assert pulse.default_window(20) == 32 and pulse.default_window(29.97) == 48 and pulse.default_window(10) == 16
    rc.same_outputs([v.cpu().numpy().reshape(-1) for v in (lambda m: (m.freq, m.power, m.total, m.index))(pulse.pulse_map(clip, P["fps"]))], want,
                    "default window")
    # criterion (a) through PulseMap.roi_bpm on the skin rectangle, (c) through periodicity
    bpm = pm.roi_bpm(P["skin_rect"])
    assert abs(bpm - 60 * P["pulse_hz"]) <= 60 * pc.STEP
    per = pm.periodicity.cpu().numpy()
    assert per[:, :2].min() > per[:, 2:].max()
    # one signal per rectangle, and its rate
    rois = [P["skin_rect"], (32, 0, 32, 64), (0, 0, 16, 16)]
    sig = pulse.pulse_signal(clip, rois, P["fps"], window=P["window"])
    assert sig.is_cuda and sig.dtype == torch.float64 and tuple(sig.shape) == (P["N"], 3)
    assert pc.same_bits(sig.cpu().numpy(), pr.pos_scalar(pr.roi_sums(clip, rois), P["window"]))
    rates = pulse.pulse_rate(clip, rois, P["fps"], window=P["window"])
    assert len(rates) == 3 and abs(rates[0][0] - 75.0) <= 60 * pc.STEP and abs(rates[2][0] - 75.0) <= 60 * pc.STEP
    assert rates[0][1] > rates[1][1] and 0 <= rates[1][1] <= 1
    # the monitor: static form, its own bgr8 buffer, and a gray buffer refused with the reason
    st = RespiratoryMonitor.pulse_map(clip, P["fps"], window=P["window"])
    rc.same_outputs([v.cpu().numpy().reshape(-1) for v in (st.freq, st.power, st.total, st.index)], want, "static")
    mon = RespiratoryMonitor.__new__(RespiratoryMonitor)
    mon.calibration_buffer = torch.from_numpy(clip).cuda()
    mon.fps, mon.freq_min, mon.freq_max = P["fps"], 0.1, 1.0
    inst = mon.pulse_map(window=P["window"])
    rc.same_outputs([v.cpu().numpy().reshape(-1) for v in (inst.freq, inst.power, inst.total, inst.index)], want, "instance")
    mon.calibration_buffer = torch.from_numpy(np.ascontiguousarray(clip[..., 1])).cuda()
    with pytest.raises(ValueError, match="gray buffer holds no pulse signal"):
        mon.pulse_map()
    with pytest.raises(TypeError):
        RespiratoryMonitor.pulse_map()
