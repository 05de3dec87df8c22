"""The pulse path (include/respmon_hip.h rm_bgr_block_sums / rm_bgr_roi_sums / rm_pulse_pos / rm_pulse_map) on the host-emulated
build (tests/emu): both forms of the block-sum kernel with their lane folds, the rectangle sums, the two POS kernels bit for bit
against the scalar restatement, rm_pulse_map against its parts, the purpose scene and every refusal (tests/pulse_cases.py), and what
needs no library at all: the restatement against the textbook POS, and the purpose criteria by the references alone.  The GPU twin
is tests/test_gpu_pulse.py."""
import ctypes

import numpy as np
import pytest

from tests import pulse_cases as pc
from tests import pulse_reference as pr


@pytest.fixture(scope="module")
def be():
    from tests.emu_harness import Emu
    emu = Emu()

    def dev(a, offset=0):
        a = np.ascontiguousarray(a)
        raw = np.empty(a.nbytes + offset + 64, np.uint8)
        start = (-raw.ctypes.data) % 64 + offset          # `offset` bytes past a 64-byte boundary
        view = raw[start:start + a.nbytes]
        view[:] = a.reshape(-1).view(np.uint8)
        return view

    class B:
        lib, ctx = emu.lib, emu.ctx
        stream = staticmethod(lambda: None)
        other_stream = staticmethod(lambda: ctypes.c_void_p(1))
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        out = staticmethod(lambda shape: np.full(shape, np.nan))
        out_i32 = staticmethod(lambda shape: np.full(shape, -7, np.int32))
        np = staticmethod(lambda a: a)
        fill = staticmethod(lambda nbytes: np.full(nbytes, pc.SENTINEL, np.uint8))
        get = staticmethod(lambda buf, dtype, shape: buf.view(np.uint8).reshape(-1).view(dtype).reshape(shape).copy())
    B.dev = staticmethod(dev)
    return B


# ---- no library ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,l", pc.pos_cases())
def test_pos_restatement_agrees_with_the_textbook_form(N, l):
    """the mean subtractions the rule leaves out are zero in exact arithmetic: within 1e-12 of max|H| on the inputs of the bit-for-bit
    case.  (Of the whole input's max|H|, not a column's: where S1 and a S2 cancel -- two-frame windows, where a = |S1| / |S2| -- a
    column's H is rounding noise around an exact 0 in both forms.)"""
    s = pc.pos_inputs(N, l)
    H, T = pc.pos_reference(N, l), pr.pos_textbook(s, l)
    scale = np.abs(H).max()
    err = np.abs(H - T).max()
    print("POS restatement vs textbook, N=%d l=%d: %.3g of max|H| = %.3g" % (N, l, err / scale, scale))
    assert scale > 0 and err <= 1e-12 * scale
    pc.check_pos_reference_properties(N, l)


@pytest.mark.parametrize("seed", pc.PURPOSE_SEEDS)
def test_purpose_criteria_are_met_by_the_references_alone(seed):
    figs = pc.purpose_reference(seed)
    print("purpose, references alone, seed %d: %s" % (seed, figs))


def test_synth_pulse_bgr_is_the_scene_of_the_issue():
    clip = pc.purpose_clip(0)
    assert clip.shape == (256, 64, 64, 3) and clip.dtype == np.uint8
    m = clip.astype(np.float64).mean(axis=(0, 1))
    assert np.allclose(m[:32].mean(axis=0), (110, 140, 200), atol=0.2) and np.allclose(m[32:].mean(axis=0), (120, 120, 120), atol=0.2)
    # the lamp dominates every channel: the frame mean of green follows 0.9 Hz with 2 % depth
    g = clip[:, :, :32, 1].astype(np.float64).mean(axis=(1, 2))
    t = np.arange(256) / 20.0
    assert abs(np.dot(g - g.mean(), np.sin(2 * np.pi * 0.9 * t)) * 2 / 256 - 0.02 * 140) < 0.15


# ---- the emulated library ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 3))
@pytest.mark.parametrize("block", pc.BLOCKS)
@pytest.mark.parametrize("shape", pc.SHAPES, ids=str)
def test_emu_block_sums_exact(be, shape, block, N):
    pc.check_block_sums(be, shape[0], shape[1], block, N)


@pytest.mark.parametrize("block", (8, 32))
def test_emu_block_sums_exact_at_the_other_block_sizes(be, block):
    for H, W in ((17, 37), (33, 64), (5, 1040)):
        pc.check_block_sums(be, H, W, block, 3)


def test_emu_block_sums_of_a_view_one_byte_into_its_allocation(be):
    pc.check_block_sums_misaligned(be)


def test_emu_roi_sums_exact(be):
    pc.check_roi_sums(be)


@pytest.mark.parametrize("N,l", pc.pos_cases())
def test_emu_pos_bit_for_bit(be, N, l):
    pc.check_pos(be, N, l)


@pytest.mark.parametrize("N", (9, 16))
@pytest.mark.parametrize("geom", pc.MAP_GEOMS, ids=str)
def test_emu_pulse_map_equals_its_three_parts(be, geom, N):
    pc.check_map_equals_parts(be, geom, N)


def test_emu_purpose_pulse_under_a_flickering_lamp(be):
    print("purpose, emulated library: %s" % pc.check_purpose(be, pc.PURPOSE_SEEDS[0]))


def test_emu_pulse_argument_errors(be):
    pc.check_argument_errors(be)


def test_emu_pulse_is_refused_while_a_submission_is_in_flight_on_another_stream(be):
    pc.check_busy(be)
