"""The newer entry points at the sizes where their launch geometry turns (tests/geometry_cases.py), on the host-emulated build
(tests/emu): folds over more than 64 tiles in both stabilisers, the row cap of the four warps, rm_bgr_to_gray's scalar tail at
misaligned bases, frame buffers that start off a 16-byte boundary through the frame-buffer chain, and the smallest and thinnest
frames through the stateful entry points.  The emulation runs a workgroup at a time, so the 2^26-pixel rm_bgr_to_gray case is left to
the GPU twin, tests/test_gpu_geometry.py, which runs everything."""
import ctypes

import numpy as np
import pytest

from tests import geometry_cases as gc


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
        full = staticmethod(lambda shape, dtype, value: np.full(shape, value, dtype=dtype))
        out = staticmethod(lambda shape: np.full(shape, np.nan))
        out_i32 = staticmethod(lambda shape: np.full(shape, -7, np.int32))
        empty = staticmethod(lambda shape, dtype: np.empty(shape, dtype))
        np = staticmethod(lambda a: a)
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        fill = staticmethod(lambda nbytes: np.full(nbytes, gc.pc.SENTINEL, np.uint8))
        get = staticmethod(lambda buf, dtype, shape: buf.view(np.uint8).reshape(-1).view(dtype).reshape(shape).copy())
        debug_set = staticmethod(emu.debug_set)
    B.dev = staticmethod(dev)
    return B


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ("shift", "sim"))
def test_restatement_spread_on_the_fold_cases(model):
    D = gc.fold_spread(model)
    print("%s: D = %.3g px (recorded %.3g); bound max(64 D, 2^-40) = %.3g px" % (model, D, gc.RECORDED_D[model], gc.fold_tolerance(model)))
    assert D < 1e-9                                                                        # a wrong tap or sign shows at 1e-3 px


@pytest.mark.parametrize("model", ("shift", "sim"))
@pytest.mark.parametrize("name", list(gc.FOLD_CASES))
def test_emu_estimate_folds_more_than_64_tiles(be, name, model):
    gc.check_fold_case(be, name, model)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("u8", "f64"))
@pytest.mark.parametrize("shape", gc.THIN_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", ("shift", "sim"))
def test_emu_warp_beyond_the_row_cap(be, model, shape, kind):
    gc.check_thin_warp(be, model, shape[0], shape[1], kind)


@pytest.mark.parametrize("shape", gc.THIN_BGR_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", ("shift", "sim"))
def test_emu_warp_bgr_beyond_the_row_cap(be, model, shape):
    gc.check_thin_warp(be, model, shape[0], shape[1], "bgr")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", gc.GRAY_OFFSETS, ids=lambda o: "in%d_out%d" % o)
def test_emu_bgr_to_gray_tail_at_every_base_alignment(be, offsets):
    gc.check_bgr_to_gray(be, gc.NPIX_SMALL, *offsets)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_emu_calibrate_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_calibrate(be, case)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_emu_rate_map_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_rate_map(be, case)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_emu_window_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_window(be, case)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_emu_stream_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_stream(be, case)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_emu_time_average_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_time_average(be, case)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
SHAPE_IDS = dict(ids=lambda s: "%dx%d" % s)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_emu_magnify_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_magnify(be, *shape)


@pytest.mark.parametrize("pair", gc.MAG_PAIRS, ids=lambda p: "L%dS%d" % p)
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_emu_magnify_means_what_the_reference_means_on_degenerate_and_thin_frames(be, shape, pair):
    """rm_magnify within 4 d0 + e_raw of the oracle's collapse of the magnified pyramid.  Where level S is a single pixel the oracle's
    raw is 0 or rounding alone and the bound is below 1e-15 of the frame: the library must take the Laplacians before the filter there."""
    gc.check_edge_magnify_reference(be, *shape, *pair)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_emu_stream_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_stream(be, *shape)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_emu_window_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_window(be, *shape)


def test_emu_window_whose_level_s_is_one_pixel_at_depth(be):
    gc.check_edge_window(be, 5, 4, L=5, S=3)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_emu_rate_map_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_rate_map(be, *shape)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_emu_stabilisers_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_stab(be, *shape)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_emu_phase_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_phase(be, *shape)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_emu_pulse_sums_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_pulse(be, *shape)
