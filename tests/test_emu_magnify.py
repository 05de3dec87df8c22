"""rm_magnify (the magnified video: frames + band-passed motion in one fused pass, respmon_amd/csrc/rm_magnify.h) on the host
emulation of the shipped kernels: small shapes through every branch.  The `-m gpu` counterpart is tests/test_gpu_magnify.py.

Definition under test (include/respmon_hip.h):  m[t] = f[t] + raw[t], one float64 addition per pixel, f the frame as the calibration
reads it and raw the raw_bandpassed_data of rm_eulerian_magnification_bandpass, bit for bit."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from respmon_amd import _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_CODE = {np.dtype(np.uint8): _capi.RM_U8, np.dtype(np.float32): _capi.RM_F32, np.dtype(np.float64): _capi.RM_F64}


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


def magnify_rc(emu, frames, fps, fmin, fmax, amp, levels, skip, out, ctx=None, out_code=None):
    """The raw rm_magnify call: (return code, out)."""
    from tests.emu_harness import buf_args, ptr
    T, H, W, code = buf_args(frames)
    rc = emu.lib.rm_magnify(ctx or emu.ctx, ptr(frames), code, T, H, W, float(fps), float(fmin), float(fmax), float(amp), int(levels), int(skip),
                            ptr(out), OUT_CODE[out.dtype] if out_code is None else out_code, None)
    return rc


def magnify(emu, frames, fps=10.0, fmin=0.1, fmax=1.0, amp=500.0, levels=4, skip=2, out_dtype=np.float64, ctx=None):
    frames = np.ascontiguousarray(frames)
    out = np.empty(frames.shape[:3], out_dtype)
    emu.ck(magnify_rc(emu, frames, fps, fmin, fmax, amp, levels, skip, out, ctx=ctx), "rm_magnify")
    return out


def as_read(frames, oracle):
    """f: the frame buffer as the calibration reads it, float64."""
    if frames.ndim == 4:
        frames = np.stack([oracle.cvtColor_bgr2gray(f) for f in frames])
    if frames.dtype == np.uint8:
        return oracle.uint8_to_float(frames)
    return frames.astype(np.float64)


def to_u8(emu, m):
    """clamp to [0, 1], then rm_float_to_uint8 (transforms.py:26-29)."""
    from tests.emu_harness import ptr
    c = np.ascontiguousarray(np.clip(m, 0.0, 1.0))
    u8 = np.empty(c.shape, np.uint8)
    emu.ck(emu.lib.rm_float_to_uint8(emu.ctx, ptr(c), ptr(u8), c.size, None), "float_to_uint8")
    return u8


def video(T, H, W, dtype, seed):
    u8 = synth.synth_breathing(T, H, W, seed=seed)
    if dtype == "bgr":
        rng = np.random.default_rng(seed)
        return np.ascontiguousarray(np.clip(u8[..., None].astype(np.int32) + rng.integers(-20, 21, (T, H, W, 3)), 0, 255).astype(np.uint8))
    if dtype == np.uint8:
        return u8
    return (u8 * (1.0 / 255)).astype(dtype)


# (T, H, W, levels, skip, input dtype, path)
CASES = [
    (6, 40, 70, 3, 1, np.uint8, "fused"),        # S = 1, W neither a multiple of 16 nor of 64, H not of 16: element-wise accesses
    (9, 48, 128, 4, 2, np.float64, "fused"),     # S = 2, odd T, whole tiles: the 16-byte accesses
    (33, 40, 72, 5, 3, np.float32, "fused"),     # S = 3, T = 33
    (2, 70, 152, 6, 4, np.float16, "fused"),     # S = 4, T = 2
    (5, 9, 20, 3, 1, np.uint8, "fused"),         # a frame smaller than one tile
    (4, 16, 64, 3, 1, np.uint8, "fused"),        # exactly one tile, uint8: 16 pixels per lane
    (8, 33, 64, 4, 2, np.uint8, "fused"),        # T even: the middle frame T / 2 is served once
    (6, 40, 70, 4, 2, "bgr", "fused"),           # BGR against its gray buffer
    (4, 16, 64, 3, 1, "bgr", "fused"),           # ... with the 48-byte pieces (uint8 output)
    (6, 20, 30, 3, 0, np.float64, "plain"),      # skip 0
    (4, 70, 70, 7, 5, np.uint8, "plain"),        # skip 5
    (3, 260, 260, 10, 8, np.float32, "plain"),   # a depth make_geom refuses
    (4, 2, 2, 3, 1, np.float64, "plain"),        # level 1 is a single row: TileEval does not apply
    (5, 20, 30, 3, 0, "bgr", "plain"),
    (5, 20, 30, 3, 2, np.uint8, "zero"),         # skip >= levels - 1: nothing is filtered
    (5, 20, 30, 2, 4, np.float32, "zero"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d_%dx%d_L%dS%d_%s_%s" % (c[0], c[1], c[2], c[3], c[4], getattr(c[5], "__name__", c[5]), c[6]))
def test_emu_magnify_equals_its_definition_bit_for_bit(emu, oracle, case):
    T, H, W, L, S, dt, path = case
    v = video(T, H, W, dt, seed=T + H)
    f = as_read(v, oracle)
    raw = emu.eulerian(v, 10.0, 0.1, 1.0, 500.0, L, S)[1]
    want = f + raw
    ctx = emu.new_ctx()   # a fresh context: its workspace names show which path ran
    m = magnify(emu, v, levels=L, skip=S, ctx=ctx)
    assert np.array_equal(m, want), np.abs(m - want).max()
    if path == "zero":
        assert np.array_equal(m, f) and not raw.any()
    # the fused path allocates no [T,H,W] float64 array: the workspace of the context stays below one
    from tests.emu_harness import ptr
    probe = np.empty(1)
    has_raw = emu.lib.rm_debug_workspace(ctx, b"magnify_raw", ptr(probe), 8, None) == _capi.RM_OK
    assert has_raw == (path == "plain" and S >= 1)
    if path == "fused":
        assert emu.lib.rm_debug_workspace(ctx, b"raw_full", ptr(probe), 8, None) == _capi.RM_E_BADARG
    # the other output dtypes are conversions of the same sum
    assert np.array_equal(magnify(emu, v, levels=L, skip=S, out_dtype=np.float32, ctx=ctx), want.astype(np.float32))
    assert np.array_equal(magnify(emu, v, levels=L, skip=S, out_dtype=np.uint8, ctx=ctx), to_u8(emu, want))
    if dt == "bgr":
        gray = np.stack([oracle.cvtColor_bgr2gray(fr) for fr in v])
        assert np.array_equal(magnify(emu, gray, levels=L, skip=S, ctx=ctx), m)
    emu.lib.rm_ctx_destroy(ctx)


def test_emu_magnify_unaligned_buffers_take_the_elementwise_accesses(emu, oracle):
    """Whole tiles but a frame buffer / output that does not start on a 16-byte boundary."""
    T, H, W, L, S = 5, 32, 64, 4, 2
    v = video(T, H, W, np.uint8, seed=3)
    raw = emu.eulerian(v, 10.0, 0.1, 1.0, 500.0, L, S)[1]
    want = as_read(v, oracle) + raw
    from tests.emu_harness import buf_args, ptr
    store_in = np.zeros(v.size + 64, np.uint8)
    store_out = np.zeros(v.size + 64, np.uint8)
    for off_in, off_out in [(1, 0), (0, 3), (5, 7)]:
        a_in = (-store_in.ctypes.data) % 16 + off_in
        a_out = (-store_out.ctypes.data) % 16 + off_out
        fin = store_in[a_in:a_in + v.size].reshape(v.shape)
        fin[:] = v
        fout = store_out[a_out:a_out + v.size].reshape(v.shape)
        fout[:] = 0
        emu.ck(magnify_rc(emu, fin, 10.0, 0.1, 1.0, 500.0, L, S, fout), "rm_magnify")
        assert np.array_equal(fout, to_u8(emu, want)), (off_in, off_out)
        assert not store_out[:a_out].any() and not store_out[a_out + v.size:].any()   # nothing outside the output


def test_emu_magnify_non_finite_frames(emu, oracle):
    """NaN and +-inf frames: the sum is what the definition gives (the temporal filter spreads them over every frame)."""
    for S, L, shape in [(2, 4, (8, 40, 70)), (0, 3, (6, 20, 30))]:
        v = video(*shape, np.float64, seed=9)
        v[2, 5:9, 7:30] = np.nan
        v[3, 20:, :10] = np.inf
        v[5, :3, -4:] = -np.inf
        raw = emu.eulerian(v, 10.0, 0.1, 1.0, 500.0, L, S)[1]
        with np.errstate(invalid="ignore"):
            want = v + raw
        m = magnify(emu, v, levels=L, skip=S)
        assert np.array_equal(m, want, equal_nan=True)
        assert np.isnan(m).any()
        assert np.array_equal(magnify(emu, v, levels=L, skip=S, out_dtype=np.float32), want.astype(np.float32), equal_nan=True)
        assert np.array_equal(magnify(emu, v, levels=L, skip=S, out_dtype=np.uint8), to_u8(emu, want))
        assert not magnify(emu, v, levels=L, skip=S, out_dtype=np.uint8)[np.isnan(want)].any()   # NaN -> 0, as rm_float_to_uint8


def test_emu_magnify_output_conversions_at_the_edges(emu):
    """Values below 0, above 1, exactly 0 (either sign), exactly 1, the neighbours of the truncation steps and NaN reach the converters of
    both kernels unchanged: amplification 0 makes raw an exact zero on the fused path, skip >= levels - 1 on the plain one."""
    special = np.array([-0.5, -1e-300, -0.0, 0.0, 1e-300, 0.5, 1.0 / 255, np.nextafter(1.0 / 255, 0), np.nextafter(1.0, 0), 1.0, np.nextafter(1.0, 2), 1.5,
                        254.0 / 255, 255.0 / 255, 2.0 ** -1074, 3e9, -3e9, 128.5 / 255])
    T, H, W = 4, 16, 64
    v = np.resize(special, (T, H, W)).astype(np.float64)
    for levels, skip, amp in [(3, 1, 0.0), (3, 2, 500.0), (5, 3, 0.0)]:
        m = magnify(emu, v, levels=levels, skip=skip, amp=amp)
        assert np.array_equal(m, v)
        u8 = magnify(emu, v, levels=levels, skip=skip, amp=amp, out_dtype=np.uint8)
        assert np.array_equal(u8, to_u8(emu, v))
        assert np.array_equal(u8, (np.clip(v, 0, 1) * 255).astype(np.uint8))   # transforms.py:26-29 on the clamped value
        assert set(np.unique(u8)) >= {0, 127, 254, 255}
        f32 = magnify(emu, v, levels=levels, skip=skip, amp=amp, out_dtype=np.float32)
        assert np.array_equal(f32, v.astype(np.float32))
    vn = v.copy()
    vn[1, 3, 5] = np.nan
    u8 = magnify(emu, vn, levels=3, skip=2, out_dtype=np.uint8)   # (plain path: NaN stays where it is)
    assert u8[1, 3, 5] == 0 and np.array_equal(u8, to_u8(emu, vn))


def reference_magnified(oracle, f, fps, fmin, fmax, amp, L, S):
    """transforms.py:148-170 followed by the commented line 181, with the oracle alone: the band-passed levels added into the video's
    own Laplacian pyramid, and that pyramid collapsed."""
    pyr = oracle.create_laplacian_video_pyramid(f, L)
    for i in range(len(pyr)):
        if i < S or i >= len(pyr) - 1:
            continue
        pyr[i] = pyr[i] + oracle.temporal_bandpass_filter_fft(pyr[i], fps, freq_min=fmin, freq_max=fmax, amplification_factor=amp)
    return oracle.collapse_laplacian_video_pyramid(pyr)


def test_emu_magnify_means_what_the_reference_means(emu, oracle):
    """m against collapse(vid_pyramid) of the reference (transforms.py:170, 181).  The two differ by rounding only: the reference adds the
    band-passed signal level by level and collapses once, the definition collapses the band-passed levels alone and adds the frame.
    d0 = max|ref - (f + raw_oracle)| / max|ref| is the cost of that reordering, measured with the oracle alone; measured on these
    inputs: 3.8e-16, 6.5e-16 and 3.4e-16 (the error of the emulated kernels against ref: 1.6e-15, 4.9e-15, 3.0e-15).  Bound: 4 d0 (inputs other than the measured ones) + the 1e-12 * max|raw| the emulated suite
    allows between the device's raw and the oracle's (tests/test_emu_calibration.py), rescaled to max|ref|."""
    for T, H, W, L, S in [(12, 48, 80, 4, 2), (10, 70, 100, 6, 4), (9, 40, 70, 3, 1)]:
        f = oracle.uint8_to_float(synth.synth_breathing(T, H, W, seed=L))
        ref = reference_magnified(oracle, f, 10.0, 0.1, 1.0, 500.0, L, S)
        raw_o = oracle.eulerian_magnification_bandpass(f.copy(), 10.0, 0.1, 1.0, 500.0, pyramid_levels=L, skip_levels_at_top=S)[1]
        scale = np.abs(ref).max()
        d0 = np.abs(ref - (f + raw_o)).max() / scale
        e_raw = 1e-12 * np.abs(raw_o).max() / scale
        m = magnify(emu, f, levels=L, skip=S)
        err = np.abs(m - ref).max() / scale
        print("magnify vs reference: T%d %dx%d L%d S%d d0=%.3g e_raw=%.3g err=%.3g" % (T, H, W, L, S, d0, e_raw, err))
        assert 0 < d0 < 1e-14
        assert err <= 4 * d0 + e_raw, (T, H, W, L, S, err, d0, e_raw)


def test_emu_magnify_arguments(emu):
    v = video(4, 16, 64, np.uint8, seed=1)
    out = np.empty(v.shape, np.uint8)
    E = _capi.RM_E_BADARG
    from tests.emu_harness import ptr
    lib, c = emu.lib, emu.ctx

    def call(frames=ptr(v), dtype=_capi.RM_U8, T=4, H=16, W=64, o=ptr(out), od=_capi.RM_U8, ctx=c, fps=10.0, levels=3, skip=1):
        return lib.rm_magnify(ctx, frames, dtype, T, H, W, fps, 0.1, 1.0, 500.0, levels, skip, o, od, None)

    assert call() == _capi.RM_OK
    good = out.copy()
    for od in (_capi.RM_F16, _capi.RM_BGR8, 7, -1):
        assert call(od=od) == E
    assert b"out_dtype" in lib.rm_last_error_string()
    assert call(o=ptr(v)) == E                                   # in place
    assert b"overlap" in lib.rm_last_error_string()
    both = np.zeros(2 * v.size, np.uint8)
    both[:v.size] = v.ravel()
    assert call(frames=ptr(both), o=ctypes.c_void_p(both.ctypes.data + v.size - 1)) == E       # the last byte of the frames
    assert call(frames=ptr(both), o=ctypes.c_void_p(both.ctypes.data + v.size)) == _capi.RM_OK   # back to back is fine
    assert np.array_equal(both[v.size:].reshape(v.shape), good)
    assert call(o=ctypes.c_void_p(v.ctypes.data - 8 * v.size + 1), od=_capi.RM_F64) == E   # a float64 output whose last byte is the frames' first
    assert call(T=0) == E and call(T=-3) == E and call(H=0) == E and call(W=0) == E
    assert call(frames=None) == E and call(o=None) == E and call(ctx=None) == E
    assert call(dtype=9) == E and call(fps=0.0) == E and call(levels=0) == E and call(skip=-1) == E
    assert call(T=4097) == _capi.RM_E_UNSUPPORTED
    out[:] = 0
    assert call() == _capi.RM_OK and np.array_equal(out, good)   # the context still works


def test_emu_magnify_is_declared_everywhere():
    """One more C-ABI entry: header, ctypes table; the ABI version stays 1 (the change is additive)."""
    assert "rm_magnify" in _capi.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "respmon_hip.h")).read()
    assert "int rm_magnify(" in hdr and "transforms.py:181" in hdr
    from tests.emu_harness import Emu   # noqa: F401  (the emulated library binds every declared symbol)


def test_frame_buffer_kernel_sources_are_untouched():
    """rm_magnify lives in units of its own: the sources hashed into rm_debug_kernel_source_stamp (csrc/Makefile STAMP_SRCS) still carry
    the stamp the committed PMC figures were measured on."""
    csrc = os.path.join(ROOT, "respmon_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("STAMP_SRCS")][0].split("=", 1)[1].split()
    assert not any("magnify" in s for s in srcs)
    sha = hashlib.sha256(b"".join(open(os.path.join(csrc, s), "rb").read() for s in srcs)).hexdigest()[:16]
    committed = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
    stamps = {v["kernel_source_sha"] for v in (committed.values() if isinstance(committed, dict) else committed) if isinstance(v, dict) and "kernel_source_sha" in v}
    assert stamps == {sha}, (stamps, sha)
