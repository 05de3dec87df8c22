"""The host arithmetic of the frame-buffer kernel's segment hand-off (rm_down_chain.h make_down_geom / down_chain_ranges, read through
rm_debug_chain_stitch of the shipped library; no GPU work is queued): for chain depths 2..4, heights 64..1100 and every split of
the two segments, the row ranges the two waves walk.  Shared checks: tests/chain_stitch_cases.py check_ranges."""
import pytest

from respmon_amd import _capi
from tests import chain_stitch_cases as cc

HEIGHTS = sorted(set(list(range(64, 200)) + list(range(200, 1101, 7)) + [719, 720, 1079, 1080, 1081, 1100]))


@pytest.fixture(scope="module")
def be():
    class B:      # no context: the host-only form of the query (no device is touched)
        lib, ctx, knobs = _capi.load(), None, {}
        stream = staticmethod(lambda: None)
    return B


@pytest.mark.parametrize("S", cc.DEPTHS)
def test_ranges_at_every_height_and_split(be, S):
    handed = refused = 0
    for H in HEIGHTS:
        rows = cc.level_sizes(H, S)[-1]
        for s, p in cc.permilles(rows):
            for on in (1, 0):
                with cc.Knobs(be, dc_segs=2, dc_split=p, dc_stitch=on):
                    d = cc.info(be, S, H, 1920, 4)
                assert d["segs"] == 2 and d["split"] in (0, s) and (d["injected"], d["fallback"]) == (0, 0), (H, s, d)
                assert on or not d["stitch"]
                if not d["split"]:                  # the upper share is not the larger one: two equal segments, no hand-off
                    assert not d["stitch"]
                    continue
                cc.check_ranges(d, S, H)
                if on:
                    handed += d["stitch"]
                    refused += not d["stitch"]
                    # refused exactly when a hand-off row or a row derived with it would meet a border rule: the cone of level-S
                    # row s must lie inside the image at every level
                    top, bot, inside = s, s, s >= 2
                    for k in range(S - 1, -1, -1):
                        top, bot = 2 * top - 2, 2 * bot + 2
                        inside = inside and top >= 0 and bot <= cc.level_sizes(H, S)[k] - 1
                    assert bool(d["stitch"]) == inside, (H, s, d)
    assert handed > 100 and refused > 100


def test_headline_geometry_hands_over(be):
    """256 x 1080p, depth 4 under the default switches: two segments, the boundary handed over, three of 1080 input rows read twice"""
    with cc.Knobs(be):
        d = cc.info(be, 4, 1080, 1920, 256)
    assert d["stitch"] == 1 and d["segs"] == 2 and d["strips"] == 6, d
    uf, ul, _, _, lf, _ = d["levels"][0]
    assert ul - lf + 1 == 3 and lf == 16 * d["split"] - 30
    with cc.Knobs(be, dc_stitch=0):
        d0 = cc.info(be, 4, 1080, 1920, 256)
    assert d0["stitch"] == 0 and d0["levels"][0][1] - d0["levels"][0][4] + 1 == 45
