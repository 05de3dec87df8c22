"""rm_sosfilt and rm_stream_* (the causal band-pass in second-order sections with carried state, a live stream magnified chunk by chunk:
respmon_amd/csrc/rm_stream.hip, rm_stream_kernels.h) on the host emulation of the shipped kernels.  Cases and check bodies:
tests/stream_cases.py; the `-m gpu` twin is tests/test_gpu_stream.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import stream_cases as sc


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


@pytest.fixture(scope="module")
def be(emu):
    class B:
        lib, ctx = emu.lib, emu.ctx
        stream = staticmethod(lambda: None)
        other_stream = staticmethod(lambda: ctypes.c_void_p(0x40))
        dev = staticmethod(lambda a: np.array(a, order="C"))
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        empty = staticmethod(lambda shape, dtype: np.zeros(shape, dtype))
        np = staticmethod(lambda a: a)

        @staticmethod
        def new_ctx(device=0):
            h = ctypes.c_void_p()
            return h if emu.lib.rm_ctx_create(device, ctypes.byref(h)) == _capi.RM_OK else None

        free_ctx = staticmethod(emu.lib.rm_ctx_destroy)
    return B


@pytest.mark.parametrize("rate", sc.SOS_RATES, ids=lambda r: "fps%g_%g-%g" % r)
@pytest.mark.parametrize("order", sc.SOS_ORDERS)
def test_emu_sosfilt_equals_its_definition_bit_for_bit(be, order, rate):
    sc.check_sosfilt(be, order, rate)


def test_emu_sosfilt_refusals(be):
    sc.check_sosfilt_refusals(be)


def test_emu_sections_are_stable_where_the_ba_form_is_not(be, emu):
    sc.check_why_sos(be, emu.lfilter)


@pytest.mark.parametrize("with_zi", [False, True], ids=["rest", "zi"])
@pytest.mark.parametrize("case", sc.STREAM_CASES, ids=sc.case_id)
def test_emu_stream_is_its_definition_however_it_is_cut(be, case, with_zi):
    sc.check_stream_case(be, case, with_zi)


def test_emu_stream_steady_start_is_quiet(be):
    sc.check_steady_start_is_quiet(be)


def test_emu_stream_state_hygiene(be, emu):
    sc.check_state_hygiene(be, lambda v: emu.locate(v, sc.FPS, levels=4, skip=2), lambda v: emu.magnify(v, 10.0, 0.1, 1.0, 500.0, 4, 2))


def test_emu_stream_refusals(be, emu):
    sc.check_stream_refusals(be, lambda v: emu.locate_submit(v, sc.FPS, levels=4, skip=2), emu.locate_result)


@pytest.mark.parametrize("case", sc.REFERENCE_CASES, ids=sc.case_id)
def test_emu_stream_means_what_the_reference_means(be, oracle, case):
    sc.check_means_what_the_reference_means(be, oracle, case)


def test_emu_stream_is_declared_everywhere(be):
    sc.check_bookkeeping(be.lib)
