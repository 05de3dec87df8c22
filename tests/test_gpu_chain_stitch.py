"""The frame-buffer kernel's hand-off of its segment boundary (rm_down_chain.h k_down_chain_stitch) on the MI355X, where the two
segments of a frame really run on two XCDs at the same time: G_S equals S successive rm_pyr_down calls bit for bit whichever (frame,
strip) pairs found their flags set, injected + fallback accounts for every pair, a withheld flag hangs nothing, and rm_locate finds
the same ROI with the hand-off on and off.  The host-emulated twin is tests/test_emu_chain_stitch.py; shared checks:
tests/chain_stitch_cases.py.  The share of pairs that took the hand-off is printed, not asserted: it depends on scheduling."""
import ctypes

import numpy as np
import pytest

from respmon_amd import _capi
from tests import chain_stitch_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    from respmon_amd import device
    lib = _capi.load()
    h = ctypes.c_void_p()      # a context of its own: the switches of this module never reach the one the other modules share
    _capi.check(lib, lib.rm_ctx_create(torch.cuda.current_device(), ctypes.byref(h)), "rm_ctx_create")

    class B:
        stream = staticmethod(device.stream_ptr)
        dev = staticmethod(lambda a: torch.from_numpy(np.array(a)).cuda())
        p = staticmethod(lambda t: ctypes.c_void_p(t.data_ptr()))
        out = staticmethod(lambda shape: torch.full(tuple(shape), float("nan"), dtype=torch.float64, device="cuda"))
        np = staticmethod(lambda t: t.cpu().numpy())
    B.lib, B.ctx = lib, h
    yield B
    torch.cuda.synchronize()
    lib.rm_ctx_destroy(h)


@pytest.mark.parametrize("S", cc.DEPTHS)
def test_emulated_shapes_every_split(be, S):
    taken = pairs = handed = 0
    for H in cc.heights(S):
        for W in cc.WIDTHS:
            sh = cc.Shape(be, S, H, W, 5)
            for s, p in cc.permilles(sh.rows):
                d = cc.check_split(sh, p, swap=0, want_taken=None)
                cc.check_off(sh, p)
                if d["stitch"]:
                    handed += 1
                    taken += d["injected"]; pairs += d["injected"] + d["fallback"]
    assert handed >= 6
    print("depth %d: %d of %d (frame, strip) pairs took the hand-off (%.1f %%)" % (S, taken, pairs, 100.0 * taken / pairs))


def test_full_hd(be):
    """1080 x 1920 x T = 4 at depth 4, two segments by force: six strips in three lockstep workgroups per segment"""
    sh = cc.Shape(be, 4, 1080, 1920, 4)
    for p in (0, 530):
        d = cc.check_split(sh, p, swap=0, want_taken=None)
        assert d["stitch"] == 1 and d["strips"] == 6, d
        print("1080p, dc_split %d: %d of %d pairs took the hand-off" % (p, d["injected"], d["injected"] + d["fallback"]))
    cc.check_off(sh, 0)


@pytest.mark.parametrize("S", cc.DEPTHS)
def test_withheld_flag(be, S):
    H = cc.heights(S)[1]
    sh = cc.Shape(be, S, H, 336, 5)
    seen = 0
    for s, p in cc.permilles(sh.rows):
        seen += cc.check_stalled(sh, p, swap=0, frame=2) is not None
    assert seen >= 1


def test_locate_same_roi(be):
    from respmon_amd import synth
    T, H, W = 16, 128, 336
    v = be.dev(synth.synth_breathing(T, H, W, seed=11).astype(np.float64) * (1.0 / 255))
    rois = []
    for on in (1, 0):
        with cc.Knobs(be, dc_segs=2, dc_split=750, dc_stitch=on, dc_stitch_count=1):
            d = cc.info(be, 2, H, W, T)
            xywh = np.full(4, -7, np.int32)
            rc = _capi.check(be.lib, be.lib.rm_locate(be.ctx, be.p(v), _capi.RM_F64, T, H, W, 10.0, 0.1, 1.0, 500.0, 5, 2, 0.7, 20, 0,
                                                      ctypes.c_void_p(xywh.ctypes.data), be.stream()), "rm_locate")
            inj, fb = cc.counters(be)
        assert d["stitch"] == on and inj + fb == (T * d["strips"] if on else 0), (d, inj, fb)
        rois.append((rc, tuple(int(x) for x in xywh)))
    assert rois[0] == rois[1] and rois[0][0] == _capi.RM_OK, rois
