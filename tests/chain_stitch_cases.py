"""Shared by tests/test_emu_chain_stitch.py, tests/test_host_chain_stitch.py and tests/test_gpu_chain_stitch.py (not a test module): the
frame-buffer kernel's hand-off of its segment boundary (respmon_amd/csrc/rm_down_chain.h, "the stitch").  A backend `be` hides where
the memory lives (as in tests/window_cases.py): be.lib, be.ctx, be.stream(), be.dev(ndarray), be.p(buffer), be.out(shape), be.np(buffer).

The reference for G_S is S successive rm_pyr_down calls on the same frames -- never the stitched kernel itself -- and every comparison
is exact: the handed-over rows are the values the upper wave would have computed, from the same inputs by the same operations."""
import ctypes

import numpy as np

from respmon_amd import _capi

WORDS = 64                                   # RM_CHAIN_STITCH_WORDS
DEPTHS = (2, 3, 4)
WIDTHS = (64, 336)                           # one strip; at depth 4 two strips in one lockstep workgroup (21 level-4 columns > 20)
DEFAULTS = {"dc_segs": 0, "dc_split": 0, "dc_stitch": 1, "dc_stitch_count": 0, "dc_stitch_swap": 0, "dc_stitch_stall_frame": -1}


def heights(S):
    """even and odd heights at every level"""
    return (8 << S, (8 << S) + (1 << S) - 2, (12 << S) + 1)


def level_sizes(n, S):
    out = [n]
    for _ in range(S):
        out.append((out[-1] + 1) // 2)
    return out


class Knobs:
    """sets the switches, puts every switch of this feature back to its default on exit"""
    def __init__(self, be, **knobs):
        self.be, self.knobs = be, knobs

    def _set(self, k, v):
        if self.be.ctx is None:      # the host-only query of rm_debug_chain_stitch: the switches travel with the call
            self.be.knobs[k] = int(v)
            return
        _capi.check(self.be.lib, self.be.lib.rm_debug_set(self.be.ctx, k.encode(), int(v)), "rm_debug_set")

    def __enter__(self):
        for k, v in DEFAULTS.items():
            self._set(k, self.knobs.get(k, v))
        return self

    def __exit__(self, *exc):
        for k, v in DEFAULTS.items():
            self._set(k, v)


def info(be, S, H, W, T):
    """rm_debug_chain_stitch under the switches in force -> dict (ranges: level -> six inclusive bounds)"""
    out = np.zeros(WORDS, np.int64)
    if be.ctx is None:
        out[:4] = [be.knobs["dc_segs"], 0, be.knobs["dc_split"], be.knobs["dc_stitch"]]
    _capi.check(be.lib, be.lib.rm_debug_chain_stitch(be.ctx, S, H, W, T, ctypes.c_void_p(out.ctypes.data), be.stream()), "rm_debug_chain_stitch")
    d = dict(stitch=int(out[0]), segs=int(out[1]), split=int(out[2]), strips=int(out[3]), injected=int(out[4]), fallback=int(out[5]),
             stall=int(out[6]))
    d["levels"] = {k: tuple(int(v) for v in out[8 + 6 * k: 14 + 6 * k]) for k in range(S + 1)} if S else {}
    return d


def counters(be):
    d = info(be, 0, 0, 0, 0)
    return d["injected"], d["fallback"]


def permilles(rows):
    """one dc_split value per possible boundary: upper = int(rows * p / 1000 + 0.5) = s for s = 1 .. rows - 1"""
    out = []
    for s in range(1, rows):
        p = int(round(s * 1000.0 / rows))
        assert p > 0 and int(rows * (p * 0.001) + 0.5) == s, (rows, s, p)
        out.append((s, p))
    return out


_FRAMES = {}


def frames(T, H, W):
    """float64 [T,H,W] noise (made once, read-only): every pixel matters to an exact comparison"""
    key = (T, H, W)
    if key not in _FRAMES:
        a = np.random.default_rng(1000 * T + 7 * H + W).random((T, H, W))
        a.setflags(write=False)
        _FRAMES[key] = a
    return _FRAMES[key]


def levels_for(S):
    return S + 2


def chain(be, buf, T, H, W, S):
    """G_S as the fused chain computes it: what rm_shard_pyramid returns on the filter-first path"""
    NP = ctypes.c_size_t()
    _capi.check(be.lib, be.lib.rm_shard_layout(H, W, levels_for(S), S, ctypes.byref(NP)), "rm_shard_layout")
    hs, ws = level_sizes(H, S)[-1], level_sizes(W, S)[-1]
    assert int(NP.value) == hs * ws, "not the filter-first layout: rm_shard_pyramid would not return G_S"
    out = be.out((T, hs * ws))
    _capi.check(be.lib, be.lib.rm_shard_pyramid(be.ctx, be.p(buf), _capi.RM_F64, T, H, W, levels_for(S), S, 0, be.p(out), be.stream()),
                "rm_shard_pyramid")
    return be.np(out).reshape(T, hs, ws)


def reference(be, buf, T, H, W, S):
    """S successive rm_pyr_down calls"""
    cur, code = buf, _capi.RM_F64
    hh, ww = level_sizes(H, S), level_sizes(W, S)
    for k in range(S):
        dst = be.out((T, hh[k + 1], ww[k + 1]))
        _capi.check(be.lib, be.lib.rm_pyr_down(be.ctx, be.p(cur), code, T, hh[k], ww[k], be.p(dst), be.stream()), "rm_pyr_down")
        cur = dst
    return be.np(cur)


class Shape:
    """one (S, H, W, T): the frames where the library reads them, and the reference (computed once, never modified)"""
    _cache = {}

    def __new__(cls, be, S, H, W, T):
        key = (id(be), S, H, W, T)
        if key not in cls._cache:
            o = object.__new__(cls)
            o.be, o.S, o.H, o.W, o.T = be, S, H, W, T
            o.buf = be.dev(frames(T, H, W))
            with Knobs(be, dc_stitch=0):
                o.ref = reference(be, o.buf, T, H, W, S)
            o.ref.setflags(write=False)
            o.rows = level_sizes(H, S)[-1]
            cls._cache[key] = o
        return cls._cache[key]

    def run(self, **knobs):
        """G_S under the switches, the geometry the host function reports for them, the counters of that launch"""
        be = self.be
        with Knobs(be, dc_segs=2, **knobs):
            d = info(be, self.S, self.H, self.W, self.T)
            got = chain(be, self.buf, self.T, self.H, self.W, self.S)
            d["injected"], d["fallback"] = counters(be)
        return got, d


def check_split(sh, p, swap, want_taken):
    """one dc_split value with the hand-off on and counted.  want_taken: True = every pair must inject (the emulation with the lower
    block first), False = every pair must fall back (the emulation in index order), None = any mix (a GPU)"""
    got, d = sh.run(dc_split=p, dc_stitch=1, dc_stitch_count=1, dc_stitch_swap=swap)
    assert np.array_equal(got, sh.ref), (sh.S, sh.H, sh.W, sh.T, p, d)
    pairs = sh.T * d["strips"]
    if not d["stitch"]:
        assert (d["injected"], d["fallback"]) == (0, 0), d
    elif want_taken is None:
        assert d["injected"] + d["fallback"] == pairs, d
    else:
        assert (d["injected"], d["fallback"]) == ((pairs, 0) if want_taken else (0, pairs)), d
    return d


def check_off(sh, p):
    got, d = sh.run(dc_split=p, dc_stitch=0, dc_stitch_count=1)
    assert d["stitch"] == 0 and (d["injected"], d["fallback"]) == (0, 0), d
    assert np.array_equal(got, sh.ref), (sh.S, sh.H, sh.W, sh.T, p)


def check_stalled(sh, p, swap, frame):
    """the lower wave of (frame, strip 0) keeps its flag back: the call returns, equals the reference, and every strip of the workgroup
    that holds strip 0 of that frame fell back.  Returns the geometry (None: this split does not hand over)."""
    got, d = sh.run(dc_split=p, dc_stitch=1, dc_stitch_count=1, dc_stitch_swap=swap, dc_stitch_stall_frame=frame)
    assert np.array_equal(got, sh.ref), (sh.S, sh.H, sh.W, sh.T, p, d)
    if not d["stitch"]:
        return None
    assert d["stall"] == frame
    pairs, in_wg = sh.T * d["strips"], min(2, d["strips"])
    if swap:     # the emulation with the lower block first: every flag but the withheld one is there
        assert (d["injected"], d["fallback"]) == (pairs - in_wg, in_wg), d
    else:
        assert d["injected"] + d["fallback"] == pairs and d["fallback"] >= in_wg, d
    return d


def check_ranges(d, S, H):
    """the ranges of one two-segment geometry (info()): every level-S row exactly once, every injected row one the lower segment emits,
    three shared input rows wherever the launch hands over, the halo otherwise"""
    hh = level_sizes(H, S)
    lv = d["levels"]
    s = d["split"]
    uf, ul, jf, jl, lf, ll = lv[S]
    assert (uf, ul, lf, ll) == (0, s - 1, s, hh[S] - 1) and jf > jl, d       # level S itself is never handed over
    for k in range(S):
        uf, ul, jf, jl, lf, ll = lv[k]
        assert 0 <= uf <= ul < hh[k] and 0 <= lf <= ll == hh[k] - 1, (k, d)
        if d["stitch"]:
            if k == 0:
                assert jf > jl and ul - lf + 1 == 3, (k, d)                  # exactly three input rows are read twice
            else:
                assert (jf, jl) == (ul + 1, ul + 3) and jf == lf and jl <= ll, (k, d)     # injected rows continue the upper wave's own and are the lower wave's first three
            # what the upper wave has at level k (its own rows and the injected ones) is what the level-(k+1) rows it computes need:
            # row 2y + 2 for the last of them
            have = jl if k else ul
            need = 2 * lv[k + 1][1] + 2
            assert have == need, (k, have, need, d)
            assert lf == 2 * lv[k + 1][4] - 2, (k, d)                        # the lower wave's first row: no border rule on the way
        else:
            assert jf > jl and ul == min(hh[k] - 1, 2 * lv[k + 1][1] + 2), (k, d)
