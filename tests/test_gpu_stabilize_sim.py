"""The similarity stabiliser (include/respmon_hip.h rm_stab_sim_*, rm_warp_similarity; respmon_amd/stabilize.py model='similarity') on
the MI355X: the checks of tests/stabilize_sim_cases.py on the shipped kernels -- the warp bit for bit on every dtype pair, the four frame
corners within max(64 D, 2^-40) px of the numpy restatement, the structural equalities and every cut bit for bit, the degenerate and far
inputs, the purpose, the crop, the refusals -- and the Python layer.  The host-emulated twin is tests/test_emu_stabilize_sim.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi, synth
from tests import stabilize_cases as shift_cases
from tests import stabilize_sim_cases as sc

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
        dev = staticmethod(lambda a: torch.from_numpy(np.array(a, order="C")).cuda())      # (a copy: the shared clips are read-only arrays)
        full = staticmethod(lambda shape, dtype, value: torch.from_numpy(np.full(shape, value, dtype=dtype)).cuda())
        np = staticmethod(lambda t: t.cpu().numpy())
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        debug_set = staticmethod(device.debug_set)
    return B


@pytest.mark.parametrize("out_dtype", sc.WARP_OUTS, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind", sc.WARP_KINDS)
def test_warp_bit_for_bit(be, kind, out_dtype):
    sc.check_warp(be, kind, out_dtype)


def test_warp_bgr_bit_for_bit(be):
    sc.check_warp(be, "bgr", np.uint8)


def test_warp_with_zero_linear_part_is_warp_shift(be):
    sc.check_warp_zero_linear_is_warp_shift(be)


@pytest.mark.parametrize("name", list(sc.ESTIMATE_CASES))
def test_estimate_against_restatement(be, name):
    sc.check_estimate_case(be, name)


def test_no_linear_level_is_the_shift_model(be):
    sc.check_no_linear_level_is_the_shift_model(be)


def test_push_is_warp_of_the_reported_parameters(be):
    sc.check_composition(be)


@pytest.mark.parametrize("name,out_dtype", [("45x67_odd", np.uint8), ("48x64_f32", np.float64), ("45x67_bgr", np.uint8)])
def test_does_not_depend_on_the_cut(be, name, out_dtype):
    sc.check_cuts(be, name, out_dtype)


def test_constant_reference(be):
    sc.check_constant_reference(be)


def test_far_frame_raises_the_linear_clamp_flag(be):
    sc.check_far_frame(be)


def test_purpose(be):
    sc.check_purpose(be)


def test_crop(be):
    sc.check_crop(be)


def test_valid_rect_on_warped_frames(be):
    sc.check_valid_rect_on_warped_frames(be)


def test_refusals(be):
    sc.check_refusals(be)


def test_stab_sim_is_declared(be):
    sc.check_declared(be.lib)


def test_stab_sim_is_refused_while_a_submission_is_in_flight_on_another_stream(be):
    """the rule of every entry point that uses the context's workspace (rm_stream_push): RM_E_BUSY, nothing written, state untouched"""
    import torch
    side = ctypes.c_void_p(torch.cuda.Stream().cuda_stream)
    f = be.dev(sc.clip(48, 64, 4.0)[:4])
    out = be.full((4, 48, 64), np.uint8, sc.SENTINEL)
    frames = be.dev(synth.synth_breathing(33, 40, 64, seed=2))
    with sc.Session(be, 48, 64, 2, 0, 1, 2, 4.0) as s:
        par, flags = np.full((4, 4), float(sc.SENTINEL)), np.full(4, sc.SENTINEL, np.int32)
        zero = np.zeros((4, 4))
        pp, fp, zp = (ctypes.c_void_p(a.ctypes.data) for a in (par, flags, zero))
        tk, xywh = ctypes.c_int(-1), np.zeros(4, np.int32)
        _capi.check(be.lib, be.lib.rm_locate_submit(be.ctx, be.p(frames), _capi.RM_U8, 33, 40, 64, 10.0, 0.1, 1.0, 500.0, 4, 2, 0.7, 20, 0, be.stream(),
                                                    ctypes.byref(tk)), "rm_locate_submit")
        rc1 = be.lib.rm_stab_sim_push(be.ctx, s.handle, be.p(f), _capi.RM_U8, 4, be.p(out), _capi.RM_U8, pp, fp, side)
        msg1 = be.lib.rm_last_error_string()
        rc2 = be.lib.rm_warp_similarity(be.ctx, be.p(f), _capi.RM_U8, 4, 48, 64, zp, be.p(out), _capi.RM_U8, side)
        rc3 = be.lib.rm_stab_sim_set_reference(be.ctx, s.handle, be.p(f), _capi.RM_U8, side)
        _capi.check(be.lib, be.lib.rm_locate_result(be.ctx, tk.value, ctypes.c_void_p(xywh.ctypes.data)), "rm_locate_result")
        assert rc1 == _capi.RM_E_BUSY and b"in flight" in msg1 and rc2 == _capi.RM_E_BUSY and rc3 == _capi.RM_E_BUSY
        assert s.info()[:2] == (0, 0)
        assert (par == sc.SENTINEL).all() and (flags == sc.SENTINEL).all() and (be.np(out) == sc.SENTINEL).all()
        assert be.lib.rm_stab_sim_push(be.ctx, s.handle, be.p(f), _capi.RM_U8, 4, be.p(out), _capi.RM_U8, pp, fp, be.stream()) == _capi.RM_OK
        assert s.info()[:2] == (4, 1) and not flags.any()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["45x67_odd", "48x64_u16", "45x67_bgr"])
def test_stabilizer_on_tensors_equals_numpy_and_the_c_abi(be, name):
    from respmon_amd import stabilize
    from respmon_amd.stabilize import Stabilizer
    H, W, lc, lf, ll, ms, kind, scale = sc.ESTIMATE_CASES[name]
    f = np.array(sc.frames_of(name))
    kw = dict(max_shift=ms, levels=(lc, lf), model="similarity", max_linear=sc.MAX_LINEAR, linear_level=ll)
    with sc.session_for(be, name) as s:
        want = s.push(f, f.dtype)
    with Stabilizer(H, W, **kw) as a, Stabilizer(H, W, **kw) as b:
        on_np = a.push(f)
        on_t = b.push(_cuda(f))
        assert isinstance(on_np[0], np.ndarray) and on_t[0].is_cuda and a.frames_seen == sc.N and a.has_reference and a.state_bytes > 0
        assert on_np[1].shape == (sc.N, 4) and all(sc.same(x, y) for x, y in zip(on_np, want))
        assert sc.same(on_t[0].cpu().numpy(), want[0]) and sc.same(on_t[1], want[1]) and sc.same(on_t[2], want[2])
        assert a.valid_rect == stabilize.valid_rect(H, W, ms, sc.MAX_LINEAR)
        # pieces, single frames, estimate(), warp(), set_reference(), reset()
        b.reset()
        assert not b.has_reference
        one = b.push(f[0])
        assert one[0].shape == f[0].shape and sc.same(one[0], want[0][0]) and sc.same(one[1], want[1][:1])
        rest = b.estimate(_cuda(f[1:]))
        assert sc.same(rest[0], want[1][1:]) and sc.same(rest[1], want[2][1:])
        assert sc.same(b.warp(f, want[1]), want[0]) and sc.same(b.warp(f[3], want[1][3]), want[0][3])
        b.reset()
        b.set_reference(f[0])
        assert sc.same(b.push(f[4:])[0], want[0][4:])
        if kind != "bgr":
            assert sc.same(a.warp(f, want[1], out_dtype="float64"), sc.warp(be, f, want[1], np.float64))
            with pytest.raises(TypeError):
                a.push(f, out_dtype="float16")
        with pytest.raises(ValueError):
            a.push(np.zeros((2, H + 1, W), np.uint8))
        with pytest.raises(ValueError):
            a.warp(f, np.zeros((sc.N, 2)))
    # the helpers read the parameters
    true = sc.truth_of(name)
    assert np.abs(stabilize.rotation_deg(want[1]) - stabilize.rotation_deg(true)).max() < 0.2 and np.abs(stabilize.zoom(want[1]) - stabilize.zoom(true)).max() < 0.005
    assert np.abs(stabilize.rotation_deg(true)).max() <= 1.0 and stabilize.rotation_deg(true[3]).shape == ()
    with pytest.raises(ValueError):
        Stabilizer(H, W, model="affine")


def test_default_model_is_the_shift_model():
    from respmon_amd.stabilize import Stabilizer
    f = np.array(shift_cases.frames_of("45x67_odd"))
    with Stabilizer(45, 67, max_shift=4.0, levels=(2, 0)) as a, Stabilizer(45, 67, max_shift=4.0, levels=(2, 0), model="shift") as b:
        x, y = a.push(f), b.push(f)
        assert a.model == "shift" and x[1].shape == (shift_cases.N, 2) and all(sc.same(p, q) for p, q in zip(x, y))
        assert a.valid_rect == (4, 4, 59, 37)


def test_stabilize_video_equals_a_push_and_crops():
    from respmon_amd import stabilize, transforms
    from respmon_amd.stabilize import Stabilizer
    name = "96x128_l20_all"
    H, W, lc, lf, ll, ms, kind, scale = sc.ESTIMATE_CASES[name]
    f = np.array(sc.frames_of(name))
    kw = dict(max_shift=ms, levels=(lc, lf), model="similarity", max_linear=sc.MAX_LINEAR, linear_level=ll)
    with Stabilizer(H, W, **kw) as s:
        want = s.push(f)
    got = transforms.stabilize_video(f, return_shifts=True, **kw)
    assert all(sc.same(a, b) for a, b in zip(got, want))
    assert sc.same(transforms.stabilize_video(_cuda(f), **kw).cpu().numpy(), want[0])
    with Stabilizer(H, W, model="similarity") as s:                                        # the defaults: levels (3, 0), max_shift 8, max_linear 0.03, level 1
        assert sc.same(transforms.stabilize_video(f, out_dtype="float32", model="similarity"), s.push(f, out_dtype="float32")[0])
    # crop=True: the frames cut to valid_rect, for both models; the default changes nothing
    x, y, w, h = stabilize.valid_rect(H, W, ms, sc.MAX_LINEAR)
    cut = transforms.stabilize_video(f, crop=True, **kw)
    assert cut.shape == (sc.N, h, w) and sc.same(cut, np.ascontiguousarray(want[0][:, y:y + h, x:x + w]))
    assert sc.same(transforms.stabilize_video(_cuda(f), crop=True, **kw).cpu().numpy(), cut)
    whole = transforms.stabilize_video(f, max_shift=ms, levels=(lc, lf))
    x, y, w, h = stabilize.valid_rect(H, W, ms)
    assert (x, y, w, h) == (4, 4, W - 8, H - 8)
    assert sc.same(transforms.stabilize_video(f, max_shift=ms, levels=(lc, lf), crop=True), np.ascontiguousarray(whole[:, y:y + h, x:x + w]))
    b = np.array(sc.frames_of("45x67_bgr"))
    assert transforms.stabilize_video(b, max_shift=4.0, levels=(2, 0), model="similarity", crop=True).shape == (sc.N, 33, 55, 3)


def test_stabilized_capture_round_trip():
    """an 'average' monitor on the shaken capture behind StabilizedCapture(model='similarity') gives, value for value, the monitor on the
    pre-stabilised frames"""
    from respmon_amd import stabilize, transforms
    from respmon_amd.base import RespiratoryMonitor
    from respmon_amd.stabilize import StabilizedCapture
    still, shaken, true, _, _ = sc.purpose_scene()
    shaken = np.array(shaken[:24])
    kw = dict(model="similarity", max_linear=0.04)
    pre = transforms.stabilize_video(shaken, **kw)
    roi = (42, 49, 21, 18)

    def run(cap):
        mon = RespiratoryMonitor(capture_target=cap, visualize=None, save_all_data=True, motion_extraction_method='average', run_on_init=False)
        mon.sync_to_fps = lambda: None
        mon.skip_calibration(*roi)
        mon.run()
        return mon
    wrapped = StabilizedCapture(synth.FakeCapture(shaken, fps=10), **kw)
    assert wrapped.isOpened() and wrapped.get(synth.CAP_PROP_FPS) == 10.0 and wrapped.get(synth.CAP_PROP_FRAME_WIDTH) == 128.0
    a, b, raw = run(wrapped), run(synth.FakeCapture(pre, fps=10)), run(synth.FakeCapture(shaken, fps=10))
    assert len(a.all_data) == 24 and np.array_equal(np.array(a.all_data, float), np.array(b.all_data, float))
    assert np.array_equal(np.array(a.data, float), np.array(b.data, float))
    assert not np.array_equal(np.array(a.all_data, float), np.array(raw.all_data, float))
    assert not wrapped.isOpened() and wrapped.stabilizer is None and len(wrapped.last_transform) == 4
    last = np.array(wrapped.last_transform)
    from tests import stabilize_sim_reference as ssr
    assert np.abs(ssr.corners(last, 96, 128) - ssr.corners(true[23], 96, 128)).max() < 0.1 and wrapped.last_shift == wrapped.last_transform[2:]
    # the frames themselves, as the capture delivers them, whole and cropped; the shift model reports (0, 0, dx, dy)
    cap = StabilizedCapture(synth.FakeCapture(shaken, fps=10), crop=True, **kw)
    x, y, w, h = stabilize.valid_rect(96, 128, 8.0, 0.04)
    assert cap.get(synth.CAP_PROP_FRAME_WIDTH) == float(w) and cap.get(synth.CAP_PROP_FRAME_HEIGHT) == float(h) and (x, y, w, h) == (13, 13, 102, 70)
    for i in range(3):
        ret, frame = cap.read()
        assert ret and frame.shape == (h, w, 3) and frame.dtype == np.uint8
        assert sc.same(frame, np.ascontiguousarray(np.repeat(pre[i][y:y + h, x:x + w, None], 3, axis=2)))
    cap.release()
    cap = StabilizedCapture(synth.FakeCapture(shaken, fps=10))
    cap.read(); cap.read()
    assert cap.last_transform[:2] == (0.0, 0.0) and cap.last_transform[2:] == cap.last_shift and cap.get(synth.CAP_PROP_FRAME_WIDTH) == 128.0
    cap.release()
