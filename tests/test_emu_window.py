"""The sliding-window calibration (include/respmon_hip.h rm_window_*) on the host-emulated build (tests/emu): the ring read in place by
the RING variants of the temporal kernels against rm_calibrate / rm_locate on the contiguous buffer of the same frames, bit for bit
(tests/window_cases.py, cases 1-4 and 7 at the small geometry).  The GPU twin is tests/test_gpu_window.py."""
import ctypes

import numpy as np
import pytest

from tests import window_cases as wc


@pytest.fixture(scope="module")
def be():
    from tests.emu_harness import Emu
    emu = Emu()

    class B:
        lib, ctx = emu.lib, emu.ctx
        stream = staticmethod(lambda: None)
        dev = staticmethod(np.ascontiguousarray)
        p = staticmethod(lambda a: ctypes.c_void_p(a.ctypes.data))
        out = staticmethod(lambda shape: np.full(shape, np.nan))
        np = staticmethod(lambda a: a)
    return B


@pytest.mark.parametrize("T,knobs", [(T, k) for T in wc.TS for k in wc.knob_cases(T)], ids=str)
def test_emu_window_every_head_position(be, T, knobs):
    wc.check_every_head(be, wc.SMALL, T, knobs)


@pytest.mark.parametrize("T", wc.TS)
def test_emu_window_push_granularity(be, T):
    wc.check_granularity(be, wc.SMALL, T)


def test_emu_window_dtypes(be):
    wc.check_dtypes(be, wc.SMALL, 10)


@pytest.mark.parametrize("flag", wc.FLAGS)
def test_emu_window_flags(be, flag):
    wc.check_flag(be, wc.SMALL, 10, flag)


def test_emu_window_argument_errors(be):
    wc.check_argument_errors(be)
