"""The frame-buffer kernel's hand-off of its segment boundary (rm_down_chain.h k_down_chain_stitch) on the host-emulated build: G_S
equals S successive rm_pyr_down calls, bit for bit, at every split of the two segments -- with the hand-off taken (the lower block made
to run first), not taken (the emulation's index order: the upper wave looks before the lower one wrote), withheld for one strip of a
lockstep workgroup, refused by the host geometry, and switched off.  Shared checks: tests/chain_stitch_cases.py."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import chain_stitch_cases as cc
from tests.emu_harness import Emu, ptr


@pytest.fixture(scope="module")
def be():
    emu = Emu()

    class B:
        lib, ctx = emu.lib, emu.ctx
        stream = staticmethod(lambda: None)
        dev = staticmethod(lambda a: np.ascontiguousarray(a))
        p = staticmethod(ptr)
        out = staticmethod(lambda shape: np.full(tuple(shape), np.nan))
        np = staticmethod(lambda a: a)
    B.emu = emu
    return B


SHAPES = [(S, H, W, T) for S in cc.DEPTHS for H in cc.heights(S) for W in cc.WIDTHS for T in (1, 5)]


@pytest.mark.parametrize("S,H,W,T", SHAPES, ids=str)
def test_every_split_taken_and_not_taken(be, S, H, W, T):
    sh = cc.Shape(be, S, H, W, T)
    handed = 0
    for s, p in cc.permilles(sh.rows):
        d = cc.check_split(sh, p, swap=1, want_taken=True)        # the lower block first: every pair injects
        assert d["split"] in (0, s)
        handed += d["stitch"]
        cc.check_split(sh, p, swap=0, want_taken=False)           # index order: every pair falls back
        if d["split"]:
            cc.check_ranges(d, S, H)
    assert handed >= 1, "no split of this shape hands over: the case would check nothing"


@pytest.mark.parametrize("S,H,W,T", SHAPES, ids=str)
def test_refused_splits_and_the_switch(be, S, H, W, T):
    """splits whose hand-off rows meet an image border: stitch == 0, nothing counted; dc_stitch 0: the same at every split"""
    sh = cc.Shape(be, S, H, W, T)
    refused = 0
    for s, p in cc.permilles(sh.rows):
        cc.check_off(sh, p)
        with cc.Knobs(be, dc_segs=2, dc_split=p):
            d = cc.info(be, S, H, W, T)
        if d["split"] and not d["stitch"]:
            refused += 1
            d = cc.check_split(sh, p, swap=1, want_taken=True)
            assert d["stitch"] == 0
    assert refused >= 1, "every two-segment split of this shape hands over: the case would check nothing"


@pytest.mark.parametrize("S,H,T", [(S, H, 5) for S in cc.DEPTHS for H in cc.heights(S)], ids=str)
def test_mixed_workgroup(be, S, H, T):
    """W = 336: one strip's flag withheld -- the call returns (no wave waits at a barrier its partner never reaches), equals the
    reference, and both strips of that workgroup fell back"""
    sh = cc.Shape(be, S, H, 336, T)
    seen = 0
    for s, p in cc.permilles(sh.rows):
        for swap in (1, 0):
            d = cc.check_stalled(sh, p, swap, frame=T // 2)
            seen += d is not None
            if d is not None and S == 4:
                assert d["strips"] == 2                              # two waves in one lockstep workgroup
    assert seen >= 2


def test_calibrate_with_and_without(be):
    """one rm_calibrate at 64 x 128 x 8, L = 5, S = 2, two segments: heatmap and min / max equal with the hand-off on and off"""
    from respmon_amd import synth
    v = synth.synth_breathing(8, 64, 128, seed=5).astype(np.float64) * (1.0 / 255)
    res = []
    for on in (1, 0):
        with cc.Knobs(be, dc_segs=2, dc_split=750, dc_stitch=on, dc_stitch_swap=1, dc_stitch_count=1):
            d = cc.info(be, 2, 64, 128, 8)
            heat, mm = be.emu.calibrate(v, 10.0, levels=5, skip=2)
            d["injected"], d["fallback"] = cc.counters(be)
        res.append((heat, mm))
        assert d["stitch"] == on and d["injected"] == (8 * d["strips"] if on else 0), d
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
