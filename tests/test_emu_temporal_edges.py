"""The temporal band-pass at every band regime, on the host-emulated build (tests/emu): the twin of test_gpu_temporal_edges.py at
T <= 256.  Reference, tolerance, case tables and check bodies: tests/temporal_edges.py.  The emulation models the fp64 matrix-core
product, it is not the hardware: the `-m gpu` module is the test proper.

Worst err / (2^-53 amp A|x|) per form, measured under emulation on these cases: DESIGN.md section 4.2."""
import numpy as np
import pytest

from tests import temporal_edges as te


class EmuRunner:
    def __init__(self, emu):
        self.e = emu

    def set(self, key, value):
        self.e.debug_set(key, value)

    def temporal(self, x, fps, fmin, fmax, amp):
        return self.e.temporal(x, fps, fmin, fmax, amp)

    def temporal_rc(self, x, fps, fmin, fmax, amp):
        return self.e.temporal_rc(x, fps, fmin, fmax, amp)

    def operator(self, T, fps, fmin, fmax):
        return self.e.operator(T, fps, fmin, fmax)

    def locate(self, v, fps, fmin, fmax, amp, L, S):
        return self.e.locate(v, fps, fmin=fmin, fmax=fmax, amp=amp, levels=L, skip=S)

    def calibrate(self, v, fps, fmin, fmax, amp, L, S):
        return self.e.calibrate(v, fps, fmin=fmin, fmax=fmax, amp=amp, levels=L, skip=S)[0]

    def eulerian(self, v, fps, fmin, fmax, amp, L, S):
        masked, raw, _ = self.e.eulerian(v, fps, fmin, fmax, amp, L, S)
        return masked, raw

    def magnify(self, v, fps, fmin, fmax, amp, L, S):
        return self.e.magnify(v, fps, fmin, fmax, amp, L, S)

    def lfilter(self, b, a, x):
        return self.e.lfilter(b, a, x)

    def lfilter_rc(self, b, a, x):
        from tests.emu_harness import ptr
        x = np.ascontiguousarray(x); out = np.empty_like(x)
        b = np.ascontiguousarray(b, dtype=np.float64); a = np.ascontiguousarray(a, dtype=np.float64)
        return self.e.lib.rm_lfilter(self.e.ctx, ptr(x), x.shape[0], x[0].size, ptr(b), ptr(a), len(b), 1.0, ptr(out), None)

    def threshold_mask(self, raw, thr):
        return self.e.threshold_mask(raw, thr)


@pytest.fixture(scope="module")
def r():
    from tests.emu_harness import Emu
    return EmuRunner(Emu())


# ---------------------------------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_emu_reference_number_format():
    """np.longdouble has the x87 format here (eps 1.08e-19 < 2^-60); where it has not, the reference runs on mpmath -- never on float64"""
    if not te.WIDE:
        import mpmath  # noqa: F401
    assert te.WIDE or te._MP[0]


def test_emu_reference_mpmath_form_agrees():
    """the mpmath form of the reference (for hosts whose long double is a plain double) gives the longdouble form's numbers"""
    band = te.regime_band(16, "half_bin_ties")
    _, want, bound = te.reference(band, 3, seed=1, cache=False)
    try:
        te.use_mpmath(True)
        _, want_mp, bound_mp = te.reference(band, 3, seed=1, cache=False)
    finally:
        te.use_mpmath(False)
    assert want_mp.dtype == object
    assert np.abs(te.f64(want_mp - want.astype(object))).max() <= 1e-17 * te.f64(bound).max()
    assert np.abs(te.f64(bound_mp - bound.astype(object))).max() <= 1e-17 * te.f64(bound).max()


def test_emu_band_bounds_pinned_for_every_table_case(oracle):
    """(lo, hi) of the reference == oracle.band_bounds for every (T, band) of the tables, the GPU-only lengths included"""
    for band in te.every_table_band():
        te.check_bounds_pinned(oracle, band)


@pytest.mark.parametrize("T", te.LENGTHS, ids=lambda T: "T%d" % T)
def test_emu_host_operator_pinned(r, T, record_property):
    """rm_temporal_operator's (blo, bhi) and M against the reference's, every regime (and the tile-count bands at T = 256):
    |M_lib - M| <= 4 * 2^-53"""
    bands = [te.regime_band(T, n) for n in te.REGIME_NAMES]
    if T == te.TILE_T:
        bands += [te.tile_band(rows) for rows in te.TILE_CASES]
    for shape in te.CONSUMER_SHAPES:
        if shape[0] == T:
            bands += [te.regime_band(T, n) for n in te.CONSUMER_REGIMES]
    worst = max(te.check_operator_pinned(r, b) for b in bands)
    record_property("max_abs_operator_error", worst)


def test_emu_regimes_reach_every_kind_of_kept_set():
    """from the reference's own kept sets at T = 64: an empty one, a nearly full one, kept sets with and without DC"""
    bands = [te.regime_band(64, n) for n in te.REGIME_NAMES]
    assert {b.nkept for b in bands} == {0, 8, 10, 12, 60, 62}
    assert sum(b.nkept == 0 for b in bands) == 3                                  # inverted, equal, negative fmin
    assert any(b.nkept >= 60 for b in bands)
    assert any(b.nkept > 0 and b.keep[0] for b in bands) and any(b.nkept > 0 and not b.keep[0] for b in bands)
    assert any(b.hi == 0 for b in bands) and any(b.lo == 0 for b in bands) and any(b.lo >= 32 for b in bands) and any(b.hi >= 32 for b in bands)
    for T in (64, 256):
        assert [n for n in te.CONSUMER_REGIMES if te.regime_band(T, n).nkept == 0] == ["inverted", "equal", "negative_fmin"]
    # the forms the lengths take: 7 and 9 (odd) and 2 (short) cannot take the matrix cores, 8 can; wide bands at T = 256 cannot
    assert not te.regime_band(7, "standard").matrix_core() and te.regime_band(8, "standard").matrix_core()
    assert not te.regime_band(9, "standard").matrix_core() and not te.regime_band(2, "everything").matrix_core()
    assert te.regime_band(256, "standard").matrix_core() and not te.regime_band(256, "everything").matrix_core()


# ---------------------------------------------------------------------------------------------------------------------------
# rm_temporal_bandpass_filter_fft
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", te.REGIME_NAMES)
@pytest.mark.parametrize("T", te.LENGTHS, ids=lambda T: "T%d" % T)
def test_emu_band_regime(r, T, name, record_property):
    te.check_filter(r, te.regime_band(T, name), NP=65, seed=1000 * T + te.REGIME_NAMES.index(name), record=record_property)


@pytest.mark.parametrize("rows", list(te.TILE_CASES), ids=lambda n: "rows%d" % n)
def test_emu_tile_count_boundary(r, rows, record_property):
    """T = 256: the larger symmetry class holds exactly 16 | 17, 32 | 33, 48 | 49 merged rows; 49 is past TM_MAX_HALF and must be
    right through the silent VALU fallback"""
    band = te.tile_band(rows)
    assert max(band.class_rows()) == rows, (band, band.class_rows())
    assert band.matrix_core() == (rows <= 48)
    record_property("class_rows", band.class_rows())
    te.check_filter(r, band, NP=65, seed=rows, record=record_property)


@pytest.mark.parametrize("NP", te.PIXEL_COUNTS, ids=lambda n: "NP%d" % n)
def test_emu_pixel_count(r, NP, record_property):
    te.check_filter(r, te.regime_band(64, "standard"), NP=NP, seed=NP, record=record_property)


def test_emu_column_isolation(r):
    te.check_column_isolation(r)


def test_emu_worst_ratio_per_form(r, record_property):
    """(runs after the cases above) the worst err / (2^-53 amp A|x|) of this session per form, and where"""
    worst = te.report_worst(record_property)
    assert set(worst) == {"default", "wide", "valu"}


# ---------------------------------------------------------------------------------------------------------------------------
# the consumers
# ---------------------------------------------------------------------------------------------------------------------------
# One emulated call of these entry points takes 0.3 s (T = 31) to 4 s (T = 256), so this twin runs every regime at the T = 31 shape, the
# regimes that differ in kind at T = 64 and one nothing-survives regime at T = 256, one buffer dtype per case; the `-m gpu` module runs
# the full table (three shapes x ten regimes x float64 and uint8).
EMU_CONSUMER_CASES = [(te.CONSUMER_SHAPES[1], n) for n in te.CONSUMER_REGIMES]
EMU_CONSUMER_CASES += [(te.CONSUMER_SHAPES[0], n) for n in ("inverted", "everything", "hi_is_0", "lo_is_0")]
EMU_CONSUMER_CASES += [(te.CONSUMER_SHAPES[2], "equal")]


@pytest.mark.parametrize("case", EMU_CONSUMER_CASES, ids=lambda c: "T%d_%dx%d_L%dS%d-" % c[0] + c[1])
def test_emu_consumers(r, oracle, case):
    """rm_locate == oracle.locate, rm_calibrate within 1e-12 of the oracle's avg_frame and bit-identical to the materialised
    average, raw within 1e-11 (exactly zero when nothing survives), rm_magnify == frame + raw"""
    shape, name = case
    kind = ("float64", "uint8")[te.CONSUMER_REGIMES.index(name) % 2]
    band, roi = te.check_consumers(r, oracle, shape, name, kinds=(kind,))
    if shape[0] in (64, 256) and band.nkept == 0:
        assert roi is None


# ---------------------------------------------------------------------------------------------------------------------------
# rm_lfilter, rm_threshold_mask
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncoef", [1, 2, 15, 16], ids=lambda n: "ncoef%d" % n)
def test_emu_lfilter(r, ncoef):
    te.check_lfilter(r, ncoef)


def test_emu_lfilter_refusals(r):
    te.check_lfilter_refusals(r)


@pytest.mark.parametrize("n", te.THRESHOLD_N, ids=lambda n: "n%d" % n)
def test_emu_threshold_mask(r, n):
    te.check_threshold_mask(r, n)
