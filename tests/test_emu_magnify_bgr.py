"""rm_magnify_bgr (the magnified video in colour: BGR frames in, BGR video out, respmon_amd/csrc/rm_magnify.h) on the host emulation of
the shipped kernels: small shapes through every branch.  The `-m gpu` counterpart is tests/test_gpu_magnify_bgr.py.

Definition under test (include/respmon_hip.h), for every frame t, pixel p and channel c:

    out[t,p,c] = u8(clamp01((double)frames[t,p,c] * (1./255) + raw[t,p]))

raw the raw_dev of rm_eulerian_magnification_bandpass on the same RM_BGR8 buffer, bit for bit; clamp01 / u8 the clamp to [0, 1] and
rm_float_to_uint8's truncation, as rm_magnify's RM_U8 output."""
import ctypes
import os

import numpy as np
import pytest

from respmon_amd import _capi, synth
from tests.test_emu_magnify import magnify, to_u8, video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


def magnify_bgr_rc(emu, frames, out, levels, skip, fps=10.0, fmin=0.1, fmax=1.0, amp=500.0, ctx=None):
    """The raw rm_magnify_bgr call on [T,H,W,3] uint8 arrays (any alignment): the return code."""
    from tests.emu_harness import ptr
    T, H, W, C = frames.shape
    assert C == 3 and frames.dtype == np.uint8 and out.dtype == np.uint8 and out.shape == frames.shape
    return emu.lib.rm_magnify_bgr(ctx or emu.ctx, ptr(frames), T, H, W, float(fps), float(fmin), float(fmax), float(amp), int(levels), int(skip),
                                  ptr(out), None)


def magnify_bgr(emu, frames, levels, skip, amp=500.0, ctx=None):
    frames = np.ascontiguousarray(frames)
    out = np.empty_like(frames)
    emu.ck(magnify_bgr_rc(emu, frames, out, levels, skip, amp=amp, ctx=ctx), "rm_magnify_bgr")
    return out


def definition(emu, v, levels, skip, amp=500.0):
    """(want, the sum before the clamp): numpy float64 in the operation order of the definition, the truncation by rm_float_to_uint8."""
    raw = emu.eulerian(v, 10.0, 0.1, 1.0, amp, levels, skip)[1]
    pre = v.astype(np.float64) * (1.0 / 255) + raw[..., None]
    return to_u8(emu, pre), pre


def has_workspace(emu, ctx, name):
    from tests.emu_harness import ptr
    probe = np.empty(1)
    rc = emu.lib.rm_debug_workspace(ctx, name, ptr(probe), 8, None)
    assert rc in (_capi.RM_OK, _capi.RM_E_BADARG)
    return rc == _capi.RM_OK


# (T, H, W, levels, skip, path)
CASES = [
    (6, 40, 70, 3, 1, "fused"),      # S = 1, W neither a multiple of 16 nor of 64, H not of 16: element-wise accesses
    (9, 48, 128, 4, 2, "fused"),     # S = 2, odd T, whole tiles: the three 16-byte pieces
    (33, 40, 72, 5, 3, "fused"),     # S = 3, T = 33, element-wise
    (5, 40, 80, 5, 3, "fused"),      # S = 3, W a multiple of 16 but not of 64, H not of 16: 16-byte pieces next to lanes outside the frame
    (2, 70, 152, 6, 4, "fused"),     # S = 4, T = 2, element-wise
    (8, 80, 160, 6, 4, "fused"),     # S = 4, T even, 16-byte pieces
    (5, 9, 20, 3, 1, "fused"),       # a frame smaller than one tile
    (4, 16, 64, 3, 1, "fused"),      # exactly one tile
    (1, 16, 64, 3, 1, "fused"),      # T = 1
    (2, 32, 64, 4, 2, "fused"),      # T = 2: frame 1 is the middle frame, served once
    (8, 33, 64, 4, 2, "fused"),      # T even: the middle frame T / 2 is served once
    (7, 33, 48, 4, 2, "fused"),      # T odd
    (5, 20, 30, 3, 0, "plain"),      # skip 0
    (4, 70, 70, 7, 5, "plain"),      # skip 5
    (4, 2, 2, 3, 1, "plain"),        # level 1 is a single row: TileEval does not apply
    (5, 20, 30, 3, 2, "zero"),       # skip >= levels - 1: nothing is filtered
    (5, 32, 64, 2, 4, "zero"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d_%dx%d_L%dS%d_%s" % c)
def test_emu_magnify_bgr_equals_its_definition_bit_for_bit(emu, case):
    T, H, W, L, S, path = case
    v = video(T, H, W, "bgr", seed=T + H)
    assert (v[..., 0] != v[..., 1]).any() and (v[..., 1] != v[..., 2]).any()   # channels that differ
    want, pre = definition(emu, v, L, S)
    ctx = emu.new_ctx()   # a fresh context: its workspace names show which path ran
    got = magnify_bgr(emu, v, L, S, ctx=ctx)
    assert got.shape == (T, H, W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), int(np.abs(got.astype(int) - want).max())
    # no large intermediate: the fused path allocates neither materialised raw buffer; the plain path behind S >= 1 collapses into one
    assert has_workspace(emu, ctx, b"magnify_raw") == (path == "plain" and S >= 1)
    if path == "fused":
        assert not has_workspace(emu, ctx, b"raw_full")
    if path == "zero":   # raw == 0: float_to_uint8(uint8_to_float(k)) per byte
        assert not (pre - v.astype(np.float64) * (1.0 / 255)).any()
        assert np.array_equal(got, (v.astype(np.float64) * (1.0 / 255) * 255).astype(np.uint8))
    emu.lib.rm_ctx_destroy(ctx)


def test_emu_magnify_bgr_nothing_filtered_is_not_an_identity_copy(emu):
    """skip >= levels - 1: every byte k becomes u8(k * (1./255)) = float_to_uint8(uint8_to_float(k)), which is k - 1 on 24 of the 256
    levels (the table tests/test_oracle_golden.py::test_dtype_helpers_lut pins) and k on the others -- the gray path's rule."""
    T, H, W = 3, 16, 64
    v = (np.arange(T * H * W * 3, dtype=np.int64) * 7 % 256).astype(np.uint8).reshape(T, H, W, 3)
    assert len(np.unique(v)) == 256
    k = np.arange(256)
    lut = (k * (1.0 / 255) * 255).astype(np.uint8)
    assert int((lut != k).sum()) == 24 and set((k - lut)[lut != k]) == {1}
    for W_ in (64, 50):   # whole tiles and not: the conversion-only kernel is the same
        vv = np.ascontiguousarray(v[:, :, :W_])
        got = magnify_bgr(emu, vv, 3, 2)
        assert np.array_equal(got, lut[vv])
        assert np.array_equal(got, to_u8(emu, vv.astype(np.float64) * (1.0 / 255)))
        assert int((got != vv).sum()) > 0 and set(np.unique(vv[got != vv].astype(int) - got[got != vv])) == {1}
        assert len(np.unique(vv[got != vv])) == 24


def test_emu_magnify_bgr_unaligned_buffers_take_the_elementwise_accesses(emu):
    """Whole tiles, but a frame buffer and / or an output that starts 1 or 8 bytes off a 16-byte boundary: the same video."""
    T, H, W, L, S = 5, 32, 64, 4, 2
    v = video(T, H, W, "bgr", seed=3)
    want, _ = definition(emu, v, L, S)
    assert np.array_equal(magnify_bgr(emu, v, L, S), want)
    store_in = np.zeros(v.size + 64, np.uint8)
    store_out = np.zeros(v.size + 64, np.uint8)
    for off_in, off_out in [(0, 0), (1, 0), (0, 1), (8, 0), (0, 8), (1, 8), (8, 8)]:
        a_in = (-store_in.ctypes.data) % 16 + off_in
        a_out = (-store_out.ctypes.data) % 16 + off_out
        fin = store_in[a_in:a_in + v.size].reshape(v.shape)
        fin[:] = v
        store_out[:] = 0
        fout = store_out[a_out:a_out + v.size].reshape(v.shape)
        assert fin.ctypes.data % 16 == off_in and fout.ctypes.data % 16 == off_out
        emu.ck(magnify_bgr_rc(emu, fin, fout, L, S), "rm_magnify_bgr")
        assert np.array_equal(fout, want), (off_in, off_out)
        assert not store_out[:a_out].any() and not store_out[a_out + v.size:].any()   # nothing outside the output


@pytest.mark.parametrize("shape", [(9, 48, 128, 4, 2), (6, 40, 70, 3, 1), (5, 20, 30, 3, 0), (5, 20, 30, 3, 2)], ids=["vector", "elementwise", "plain", "zero"])
def test_emu_magnify_bgr_equal_channels_are_the_gray_video(emu, shape):
    """(k, k, k) is gray k under the integer cvtColor: every output channel is rm_magnify's RM_U8 output on that buffer."""
    T, H, W, L, S = shape
    gray = synth.synth_breathing(T, H, W, seed=5)
    v = np.ascontiguousarray(gray[..., None].repeat(3, -1))
    got = magnify_bgr(emu, v, L, S)
    g8 = magnify(emu, v, levels=L, skip=S, out_dtype=np.uint8)
    assert g8.shape == (T, H, W)
    for c in range(3):
        assert np.array_equal(got[..., c], g8), c
    assert np.array_equal(g8, magnify(emu, gray, levels=L, skip=S, out_dtype=np.uint8))


@pytest.mark.parametrize("shape", [(9, 48, 128, 4, 2), (6, 40, 70, 4, 2), (5, 20, 30, 3, 0)], ids=["vector", "elementwise", "plain"])
def test_emu_magnify_bgr_clamps_on_both_sides(emu, shape):
    T, H, W, L, S = shape
    v = video(T, H, W, "bgr", seed=8)
    amp = 50000.0
    want, pre = definition(emu, v, L, S, amp=amp)
    assert pre.min() < 0.0 and pre.max() > 1.0   # the case is not vacuous: the sum leaves [0, 1] on both sides
    got = magnify_bgr(emu, v, L, S, amp=amp)
    assert np.array_equal(got, want)
    assert np.array_equal(got, (np.clip(pre, 0.0, 1.0) * 255).astype(np.uint8))
    assert (got == 0).any() and (got == 255).any()
    assert (got[pre < 0] == 0).all() and (got[pre > 1] == 255).all()


def test_emu_magnify_bgr_arguments(emu):
    from tests.emu_harness import ptr
    v = video(4, 16, 64, "bgr", seed=1)
    out = np.zeros_like(v)
    E = _capi.RM_E_BADARG
    lib, c = emu.lib, emu.ctx

    def call(frames=ptr(v), T=4, H=16, W=64, o=ptr(out), ctx=c, fps=10.0, levels=3, skip=1):
        return lib.rm_magnify_bgr(ctx, frames, T, H, W, fps, 0.1, 1.0, 500.0, levels, skip, o, None)

    assert call() == _capi.RM_OK
    good = out.copy()
    assert np.array_equal(good, definition(emu, v, 3, 1)[0])
    assert call(frames=None) == E and call(o=None) == E and call(ctx=None) == E
    assert call(T=0) == E and call(T=-3) == E and call(H=0) == E and call(H=-1) == E and call(W=0) == E and call(W=-1) == E
    assert call(levels=0) == E and call(skip=-1) == E
    assert call(fps=0.0) == E and call(fps=-1.0) == E and call(fps=float("nan")) == E
    assert b"rm_magnify_bgr" in lib.rm_last_error_string()
    assert call(T=4097) == _capi.RM_E_UNSUPPORTED
    # overlap: 3 T H W bytes on both sides
    n = v.size
    assert n == 3 * 4 * 16 * 64
    assert call(o=ptr(v)) == E                                   # in place
    assert b"overlap" in lib.rm_last_error_string()
    three = np.zeros(3 * n, np.uint8)
    mid = three[n:2 * n]
    mid[:] = v.ravel()
    base = three.ctypes.data
    assert call(frames=ptr(mid), o=ctypes.c_void_p(base + 2 * n - 1)) == E    # the output begins on the last byte of the frames
    assert call(frames=ptr(mid), o=ctypes.c_void_p(base + 1)) == E            # the output's last byte is the frames' first
    assert call(frames=ptr(mid), o=ctypes.c_void_p(base + n + n // 3)) == E   # (a [T,H,W] reading of the sizes would let this pass)
    assert not three[:n].any() and not three[2 * n:].any() and np.array_equal(mid, v.ravel())   # a refused call writes nothing
    assert call(frames=ptr(mid), o=ctypes.c_void_p(base + 2 * n)) == _capi.RM_OK   # immediately after the frame buffer
    assert np.array_equal(three[2 * n:].reshape(v.shape), good)
    assert call(frames=ptr(mid), o=ctypes.c_void_p(base)) == _capi.RM_OK           # immediately before it
    assert np.array_equal(three[:n].reshape(v.shape), good) and np.array_equal(mid, v.ravel())
    # rm_magnify keeps refusing a BGR output
    g = np.empty(v.shape[:3], np.uint8)
    assert lib.rm_magnify(c, ptr(v), _capi.RM_BGR8, 4, 16, 64, 10.0, 0.1, 1.0, 500.0, 3, 1, ptr(g), _capi.RM_BGR8, None) == E
    assert b"out_dtype" in lib.rm_last_error_string()
    out[:] = 0
    assert call() == _capi.RM_OK and np.array_equal(out, good)   # the context still works
    assert lib.rm_abi_version() == 1


def test_emu_magnify_bgr_is_declared_everywhere():
    """One more C-ABI entry: header (with the reason the same raw goes onto the three channels), ctypes table; the ABI version stays 1."""
    assert "rm_magnify_bgr" in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["rm_magnify_bgr"][1]) == 13
    hdr = open(os.path.join(ROOT, "include", "respmon_hip.h")).read()
    assert "int rm_magnify_bgr(" in hdr and "(1, 1, 1)" in hdr and "NOT an identity copy" in hdr
    src = open(os.path.join(ROOT, "respmon_amd", "csrc", "rm_magnify.h")).read()
    assert "(1, 1, 1)" in src and "Y row of YIQ" in src
