"""The rate map (include/respmon_hip.h rm_spectral_operator / rm_spectral_peak / rm_rate_map / rm_window_rate_map, respmon_amd/rate.py)
on the MI355X: all seven cases of tests/rate_cases.py -- both forms of the MFMA kernel against the long-double reference at every
size, the form switch and T = 512 on a level wider than the switch, degenerate columns, rm_rate_map and the window's ring against
rm_spectral_peak bit for bit, the three-blob clip, argument errors, and the Python layer.  The host-emulated twin (cases 1-6) is
tests/test_emu_rate_map.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import rate_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device

    class B:
        lib = _capi.load()
        ctx = device.ctx()
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        stream = staticmethod(device.stream_ptr)
        dev = staticmethod(lambda a: torch.from_numpy(np.array(a)).cuda())      # (a copy: the shared inputs are read-only arrays)
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        out = staticmethod(lambda shape: torch.full(tuple(shape), float("nan"), dtype=torch.float64, device="cuda"))
        out_i32 = staticmethod(lambda shape: torch.full(tuple(shape), -7, dtype=torch.int32, device="cuda"))
        np = staticmethod(lambda t: t.cpu().numpy())
    return B


@pytest.mark.parametrize("case", rc.OPERATOR_CASES, ids=str)
def test_spectral_operator(be, case):
    rc.check_operator(be.lib, case)


@pytest.mark.parametrize("F", rc.FS)
@pytest.mark.parametrize("T", rc.TS)
def test_spectral_peak_against_reference(be, T, F):
    rc.check_peak(be, T, F)


def test_spectral_peak_either_side_of_the_form_switch(be):
    rc.check_form_switch(be)


def test_spectral_peak_T512_wider_than_the_switch(be):
    rc.check_long_wide(be)


def test_degenerate_columns(be):
    rc.check_degenerate(be)


@pytest.mark.parametrize("T", (16, 9))
@pytest.mark.parametrize("geom", rc.RATE_GEOMS, ids=str)
def test_rate_map_equals_peak_of_pyr_down(be, geom, T):
    rc.check_rate_map_equals_peak(be, geom, T)


@pytest.mark.parametrize("T", (16, 9))
def test_window_rate_map_equals_rate_map(be, T):
    rc.check_window(be, T)


def test_purpose_three_blobs(be):
    rc.check_purpose(be)


def test_rate_argument_errors(be):
    rc.check_argument_errors(be)


# ---- case 7: the Python layer --------------------------------------------------------------------------------------------------
def test_python_spectral_peak_and_operator(be):
    import torch
    from respmon_amd import transforms
    kw = rc.BAND
    x = rc.signals(64, 35, kw["fps"], 29).reshape(64, 5, 7)
    got = transforms.spectral_peak(np.array(x), kw["fps"], kw["fmin"], kw["fmax"], nfreq=16)
    assert type(got).__name__ == "SpectralPeak" and got._fields == ("freq", "power", "total", "index")
    assert all(isinstance(v, np.ndarray) and v.shape == (5, 7) for v in got) and got.index.dtype == np.int32
    want = rc.peak(be, x.reshape(64, 35), kw["fps"], kw["fmin"], kw["fmax"], 16)
    rc.same_outputs([v.reshape(-1) for v in got], want, "numpy")
    dev = transforms.spectral_peak(torch.from_numpy(np.array(x)).cuda(), kw["fps"], kw["fmin"], kw["fmax"], nfreq=16)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and tuple(v.shape) == (5, 7) for v in dev)
    rc.same_outputs([v.cpu().numpy().reshape(-1) for v in dev], want, "device")
    A, freqs = transforms.spectral_operator(64, kw["fps"], kw["fmin"], kw["fmax"], 16)
    A_ref, f_ref, _, _ = rc.ref_operator(64, kw["fps"], kw["fmin"], kw["fmax"], 16)
    assert A.shape == (32, 64) and np.array_equal(freqs, f_ref) and np.abs(A - A_ref.astype(np.float64)).max() < 1e-15


def test_python_rate_maps(be):
    import torch
    from respmon_amd import rate
    from respmon_amd.base import RespiratoryMonitor
    from respmon_amd.window import SlidingCalibration
    P = rc.PURPOSE
    clip = rc.purpose_clip()
    inner, bgm, rects = rc.purpose_masks()
    step_bpm = 60 * (P["fmax"] - P["fmin"]) / (P["F"] - 1)
    want = rc.rate_map(be, clip, 1, P["fps"], P["fmin"], P["fmax"], P["F"])
    # static form, like locate(): frames and fps, the band of locate()'s defaults (0.1 - 1.0 Hz)
    rm = RespiratoryMonitor.rate_map(np.array(clip), P["fps"], level=1)
    assert isinstance(rm, rate.RateMap) and rm.level == 1 and tuple(rm.freq.shape) == rc.level_shape(P["H"], P["W"], 1)
    assert all(v.is_cuda for v in (rm.freq, rm.power, rm.total, rm.index)) and rm.index.dtype == torch.int32
    rc.same_outputs([v.cpu().numpy().reshape(-1) for v in (rm.freq, rm.power, rm.total, rm.index)], want, "static")
    assert torch.equal(rm.bpm[rm.index >= 0], 60 * rm.freq[rm.index >= 0])
    per = rm.periodicity.cpu().numpy()
    tot, pw = rm.total.cpu().numpy(), rm.power.cpu().numpy()
    assert np.all(per[tot == 0] == 0) and (tot == 0).sum() >= bgm.sum() and np.array_equal(per[tot > 0], (pw / np.where(tot > 0, tot, 1))[tot > 0])
    assert np.all((per >= 0) & (per <= 1)) and per[inner[0]].min() > 1.0 / P["F"]
    for rect, (_, f) in zip(rects, P["blobs"]):
        r = rm.roi_bpm(rect)
        assert r == pytest.approx(rc.roi_bpm_host(want[0], want[1], want[3], rm.freq.shape, 1, rect), rel=1e-12) and abs(r - 60 * f) <= step_bpm
    assert rm.roi_bpm((0, 0, 4, 4)) is None                       # an all-static rectangle (the clip's corner is background)
    assert bgm[:2, :2].all()
    # instance form: the monitor's own buffer, fps and band
    mon = RespiratoryMonitor.__new__(RespiratoryMonitor)
    mon.calibration_buffer = torch.from_numpy(np.array(clip)).cuda()
    mon.fps, mon.freq_min, mon.freq_max = P["fps"], P["fmin"], P["fmax"]
    rm2 = mon.rate_map(level=1)
    rc.same_outputs([v.cpu().numpy().reshape(-1) for v in (rm2.freq, rm2.power, rm2.total, rm2.index)], want, "instance")
    assert mon.rate_map().level == 4
    with pytest.raises(TypeError):
        RespiratoryMonitor.rate_map()
    # the sliding window: level = its skip_levels_at_top
    win = SlidingCalibration(P["T"], P["H"], P["W"], pyramid_levels=4, skip_levels_at_top=1)
    try:
        win.push(np.array(clip[:40]))
        win.push(np.array(clip[40:]))
        win.push(np.array(clip[:9]))                               # wraps: the ring holds clip[9:] + clip[:9]
        rm3 = win.rate_map(P["fps"], P["fmin"], P["fmax"], P["F"])
        want3 = rc.rate_map(be, np.concatenate([clip[9:], clip[:9]]), 1, P["fps"], P["fmin"], P["fmax"], P["F"])
        assert rm3.level == 1
        rc.same_outputs([v.cpu().numpy().reshape(-1) for v in (rm3.freq, rm3.power, rm3.total, rm3.index)], want3, "window")
    finally:
        win.close()
