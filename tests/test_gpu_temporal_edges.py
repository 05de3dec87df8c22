"""The temporal band-pass at every band regime on the MI355X: rm_temporal_bandpass_filter_fft under its three kernel forms against a
long-double DFT operator with a componentwise bound, the lengths and class sizes where the form changes, the pixel-count edges, the
mirror and column-isolation properties, the T = 2048 / 2049 / 2050 limits, the consumers (rm_locate, rm_calibrate, rm_magnify) at the
same regimes, rm_lfilter and rm_threshold_mask.  Reference, tolerance, case tables and check bodies: tests/temporal_edges.py; the
emulated twin is test_emu_temporal_edges.py.

Worst err / (2^-53 amp A|x|) per form, measured on the MI355X on these cases: DESIGN.md section 4.2."""
import ctypes

import numpy as np
import pytest

from tests import temporal_edges as te

pytestmark = pytest.mark.gpu


class GpuRunner:
    def set(self, key, value):
        from respmon_amd import device
        device.debug_set(key, value)

    def temporal(self, x, fps, fmin, fmax, amp):
        from respmon_amd import transforms
        return transforms.temporal_bandpass_filter_fft(x, fps, freq_min=fmin, freq_max=fmax, amplification_factor=amp)

    def temporal_rc(self, x, fps, fmin, fmax, amp):
        """the raw return code (a refusal is an answer, not an exception) and the output"""
        import torch
        from respmon_amd import _capi, device
        lib = _capi.load()
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        out = torch.zeros_like(xd)
        rc = lib.rm_temporal_bandpass_filter_fft(device.ctx(), device.ptr(xd), xd.shape[0], xd[0].numel(), float(fps), float(fmin), float(fmax),
                                                 float(amp), device.ptr(out), device.stream_ptr())
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()

    def operator(self, T, fps, fmin, fmax):
        from respmon_amd import transforms
        return transforms.temporal_operator(T, fps, fmin, fmax)

    def _dev(self, v):
        import torch
        return torch.from_numpy(np.ascontiguousarray(v)).cuda()

    def locate(self, v, fps, fmin, fmax, amp, L, S):
        from respmon_amd.base import RespiratoryMonitor
        return RespiratoryMonitor.locate(self._dev(v), fps, freq_min=fmin, freq_max=fmax, amplification=amp, pyramid_levels=L, skip_levels_at_top=S)

    def calibrate(self, v, fps, fmin, fmax, amp, L, S):
        from respmon_amd import dist
        return dist.hip_calibrate(self._dev(v), fps, freq_min=fmin, freq_max=fmax, amplification=amp, pyramid_levels=L, skip_levels_at_top=S).cpu().numpy()

    def eulerian(self, v, fps, fmin, fmax, amp, L, S):
        from respmon_amd import transforms
        return transforms.eulerian_magnification_bandpass(v, fps, fmin, fmax, amp, pyramid_levels=L, skip_levels_at_top=S)

    def magnify(self, v, fps, fmin, fmax, amp, L, S):
        from respmon_amd import transforms
        return transforms.eulerian_magnification_video(v, fps, fmin, fmax, amp, pyramid_levels=L, skip_levels_at_top=S, out_dtype="float64")

    def lfilter(self, b, a, x):
        from respmon_amd import transforms
        return transforms.butter_bandpass_filter_fast(x, b, a, axis=0)

    def lfilter_rc(self, b, a, x):
        import torch
        from respmon_amd import _capi, device
        lib = _capi.load()
        xd = self._dev(x)
        out = torch.zeros_like(xd)
        b = np.ascontiguousarray(b, dtype=np.float64); a = np.ascontiguousarray(a, dtype=np.float64)
        rc = lib.rm_lfilter(device.ctx(), device.ptr(xd), xd.shape[0], xd[0].numel(), ctypes.c_void_p(b.ctypes.data), ctypes.c_void_p(a.ctypes.data),
                            len(b), 1.0, device.ptr(out), device.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def threshold_mask(self, raw, thr):
        import torch
        from respmon_amd import _capi, device
        lib = _capi.load()
        rd = self._dev(raw)
        masked = torch.empty_like(rd)
        mm = (ctypes.c_double * 2)()
        _capi.check(lib, lib.rm_threshold_mask(device.ctx(), device.ptr(rd), rd.numel(), float(thr), device.ptr(masked), mm, device.stream_ptr()),
                    "rm_threshold_mask")
        torch.cuda.synchronize()
        return masked.cpu().numpy(), (mm[0], mm[1])

    def cus(self):
        import torch
        return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


@pytest.fixture(scope="module")
def r():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from respmon_amd import _capi
    _capi.load()   # raises if the HIP extension is missing: no fallback
    return GpuRunner()


# ---------------------------------------------------------------------------------------------------------------------------
# rm_temporal_bandpass_filter_fft
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", te.REGIME_NAMES)
@pytest.mark.parametrize("T", te.LENGTHS + te.LENGTHS_GPU_ONLY, ids=lambda T: "T%d" % T)
def test_band_regime(r, T, name, record_property):
    """every band regime at every length, default / temporal_wide / temporal_valu (NP = 65; 17 at T >= 512, where the long-double
    reference costs the most)"""
    te.check_filter(r, te.regime_band(T, name), NP=65 if T <= 256 else 17, seed=1000 * T + te.REGIME_NAMES.index(name), record=record_property)


@pytest.mark.parametrize("rows", list(te.TILE_CASES), ids=lambda n: "rows%d" % n)
def test_tile_count_boundary(r, rows, record_property):
    """T = 256: the larger symmetry class holds exactly 16 | 17, 32 | 33, 48 | 49 merged rows; 49 is past TM_MAX_HALF and must be
    right through the silent VALU fallback, with no knob set"""
    band = te.tile_band(rows)
    assert max(band.class_rows()) == rows, (band, band.class_rows())
    assert band.matrix_core() == (rows <= 48)
    record_property("class_rows", band.class_rows())
    te.check_filter(r, band, NP=65, seed=rows, record=record_property)


@pytest.mark.parametrize("NP", te.PIXEL_COUNTS, ids=lambda n: "NP%d" % n)
def test_pixel_count(r, NP, record_property):
    te.check_filter(r, te.regime_band(64, "standard"), NP=NP, seed=NP, record=record_property)


def test_pixel_count_wide_by_default(r, record_property):
    """NP = 64 * 4 * CUs + 1 at T = 16: the DEFAULT choice takes k_temporal_sym_px (and its last workgroup holds one column)"""
    NP = 64 * 4 * r.cus() + 1
    record_property("NP", NP)
    te.check_filter(r, te.regime_band(16, "standard"), NP=NP, seed=16, cache=False, record=record_property)


def test_column_isolation(r):
    te.check_column_isolation(r)


# ---------------------------------------------------------------------------------------------------------------------------
# limits
# ---------------------------------------------------------------------------------------------------------------------------
def _still_usable(r):
    """a small call on the same context after a refusal"""
    te.check_filter(r, te.regime_band(64, "standard"), NP=17, seed=5, forms=te.FORMS[:1])


def test_limit_T2048_valu(r, record_property):
    """the longest T the VALU form stages in LDS (T * TF_KC doubles = 64 KiB), forced, NP = 65"""
    band = te.regime_band(2048, "standard")
    te.check_filter(r, band, NP=65, seed=2048, forms=[f for f in te.FORMS if f[0] == "valu"], record=record_property)


def test_limit_T2049_unsupported(r):
    """T = 2049 is odd (VALU form) and past its LDS limit: RM_E_UNSUPPORTED, nothing written, and the context stays usable"""
    band = te.regime_band(2049, "standard")
    x = np.random.default_rng(2049).standard_normal((2049, 65))
    rc, out = r.temporal_rc(x, band.fps, band.fmin, band.fmax, te.AMP)
    assert rc == te.RM_E_UNSUPPORTED, rc
    assert not out.any()
    _still_usable(r)


def test_limit_T2050_matrix_core(r, record_property):
    """T = 2050 is past the VALU limit, so it is served only where the matrix-core form applies: at most 48 merged rows per class.
    The band (0.1, 1.0) at 10 fps keeps bins 20 .. 205 there (93 rows per class): no form serves it and the library must refuse it
    cleanly.  At 40 fps the same band keeps bins 5 .. 51 (24 + 23 rows), takes the matrix-core form -- forcing the VALU form on it
    is refused, which shows which form ran -- and passes the bound under the default and the wide form."""
    at10 = te.regime_band(2050, "standard")
    assert max(at10.class_rows()) == 93 and not at10.matrix_core()
    x = np.random.default_rng(2050).standard_normal((2050, 65))
    rc, out = r.temporal_rc(x, at10.fps, at10.fmin, at10.fmax, te.AMP)
    assert rc == te.RM_E_UNSUPPORTED and not out.any(), rc
    band = te.limit_2050_band()
    assert band.class_rows() == (24, 23) and band.matrix_core()
    te.check_filter(r, band, NP=65, seed=2050, forms=te.FORMS[:2], record=record_property)
    r.set("temporal_valu", 1)
    try:
        rc, _ = r.temporal_rc(x, band.fps, band.fmin, band.fmax, te.AMP)
    finally:
        r.set("temporal_valu", 0)
    assert rc == te.RM_E_UNSUPPORTED, rc
    _still_usable(r)


def test_worst_ratio_per_form(r, record_property):
    """(runs after the cases above) the worst err / (2^-53 amp A|x|) of this session per form, and where"""
    worst = te.report_worst(record_property)
    assert set(worst) == {"default", "wide", "valu"}


# ---------------------------------------------------------------------------------------------------------------------------
# the consumers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", te.CONSUMER_REGIMES)
@pytest.mark.parametrize("shape", te.CONSUMER_SHAPES, ids=lambda s: "T%d_%dx%d_L%dS%d" % s)
def test_consumers(r, oracle, shape, name):
    """float64 and uint8 buffers: rm_locate == oracle.locate (None where nothing survives at T = 64 / 256), rm_calibrate within 1e-12
    of the oracle's avg_frame and bit-identical to the materialised average, raw within 1e-11 (exactly zero when nothing survives),
    rm_magnify == frame + raw bit for bit"""
    band, roi = te.check_consumers(r, oracle, shape, name)
    if shape[0] in (64, 256) and band.nkept == 0:
        assert roi is None


# ---------------------------------------------------------------------------------------------------------------------------
# rm_lfilter, rm_threshold_mask
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncoef", [1, 2, 15, 16], ids=lambda n: "ncoef%d" % n)
def test_lfilter(r, ncoef):
    te.check_lfilter(r, ncoef)


def test_lfilter_refusals(r):
    te.check_lfilter_refusals(r)


@pytest.mark.parametrize("n", te.THRESHOLD_N, ids=lambda n: "n%d" % n)
def test_threshold_mask(r, n):
    te.check_threshold_mask(r, n)
