"""The newer entry points at the sizes where their launch geometry turns (tests/geometry_cases.py), on the MI355X: folds over more than
64 tiles in both stabilisers, the row cap of the four warps, rm_bgr_to_gray with its block cap, grid stride and scalar tail at every
base alignment (2^26 + 5 pixels), frame buffers that start off a 16-byte boundary through the frame-buffer chain, and the smallest and
thinnest frames through the stateful entry points.  The host-emulated twin is tests/test_emu_geometry.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import geometry_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device

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
        full = staticmethod(lambda shape, dtype, value: torch.from_numpy(np.full(shape, value, dtype=dtype)).cuda())
        out = staticmethod(lambda shape: torch.full(tuple(shape), float("nan"), dtype=torch.float64, device="cuda"))
        out_i32 = staticmethod(lambda shape: torch.full(tuple(shape), -7, dtype=torch.int32, device="cuda"))
        empty = staticmethod(lambda shape, dtype: torch.from_numpy(np.zeros(shape, dtype)).cuda())
        np = staticmethod(lambda t: t.cpu().numpy())
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        fill = staticmethod(lambda nbytes: torch.full((nbytes,), gc.pc.SENTINEL, dtype=torch.uint8, device="cuda"))
        get = staticmethod(lambda buf, dtype, shape: buf.cpu().numpy().view(dtype).reshape(shape))
        debug_set = staticmethod(device.debug_set)
    B.dev = staticmethod(dev)
    return B


SHAPE_IDS = dict(ids=lambda s: "%dx%d" % s)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ("shift", "sim"))
@pytest.mark.parametrize("name", list(gc.FOLD_CASES))
def test_estimate_folds_more_than_64_tiles(be, name, model):
    gc.check_fold_case(be, name, model)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("u8", "f64"))
@pytest.mark.parametrize("shape", gc.THIN_SHAPES, **SHAPE_IDS)
@pytest.mark.parametrize("model", ("shift", "sim"))
def test_warp_beyond_the_row_cap(be, model, shape, kind):
    gc.check_thin_warp(be, model, shape[0], shape[1], kind)


@pytest.mark.parametrize("shape", gc.THIN_BGR_SHAPES, **SHAPE_IDS)
@pytest.mark.parametrize("model", ("shift", "sim"))
def test_warp_bgr_beyond_the_row_cap(be, model, shape):
    gc.check_thin_warp(be, model, shape[0], shape[1], "bgr")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", (gc.NPIX_SMALL, gc.NPIX_CAP), ids=("three_trips", "block_cap"))
@pytest.mark.parametrize("offsets", gc.GRAY_OFFSETS, ids=lambda o: "in%d_out%d" % o)
def test_bgr_to_gray_stride_and_tail_at_every_base_alignment(be, offsets, npix):
    gc.check_bgr_to_gray(be, npix, *offsets)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_calibrate_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_calibrate(be, case)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_rate_map_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_rate_map(be, case)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_window_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_window(be, case)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_stream_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_stream(be, case)


@pytest.mark.parametrize("case", gc.CHAIN_CASES, ids=gc.chain_id)
def test_time_average_on_a_buffer_off_the_boundary(be, case):
    gc.check_chain_time_average(be, case)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_magnify_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_magnify(be, *shape)


@pytest.mark.parametrize("pair", gc.MAG_PAIRS, ids=lambda p: "L%dS%d" % p)
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_magnify_means_what_the_reference_means_on_degenerate_and_thin_frames(be, shape, pair):
    gc.check_edge_magnify_reference(be, *shape, *pair)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_stream_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_stream(be, *shape)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_window_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_window(be, *shape)


def test_window_whose_level_s_is_one_pixel_at_depth(be):
    gc.check_edge_window(be, 5, 4, L=5, S=3)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_rate_map_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_rate_map(be, *shape)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_stabilisers_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_stab(be, *shape)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_phase_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_phase(be, *shape)


@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, **SHAPE_IDS)
def test_pulse_sums_on_degenerate_and_thin_frames(be, shape):
    gc.check_edge_pulse(be, *shape)
