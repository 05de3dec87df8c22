"""TEST INFRASTRUCTURE (not a test module): the contour ranking of locate() without a contour, the case table that goes with it and the
checks that tests/test_emu_roi_reference.py and tests/test_gpu_roi_reference.py share.

The product's ROI is cv2's: the largest contourArea among the RETR_EXTERNAL contours, then its boundingRect.  Everything else in the
suite that knows which contour that is (oracle/cvref.c) follows borders the way the product does.  This module does not.  For an
external contour traced through pixel centres with 8-connectivity,

    contourArea = #(full 2 x 2 blocks) + 1/2 #(2 x 2 blocks with three pixels set)      of the hole-filled component,

because the polygon through the border pixels' centres covers exactly the unit squares between four set pixels and half of the
squares between three; and RETR_EXTERNAL lists exactly the 8-connected components of the hole-filled image (the background of an
8-connected foreground is 4-connected, so scipy's default fill removes every component nested in a hole of another).  boundingRect is
the component's box.  findContours lists contours by DESCENDING raster index of their first pixel, and Python's max keeps the first
maximum, so an exact tie goes to the component whose first pixel comes last in raster order.  clip_frame (OpenCV <= 3.1) zeroes the
one-pixel frame first.
"""
import itertools

import numpy as np
import scipy.ndimage as ndi

THRESHOLD = 20
EIGHT = np.ones((3, 3), bool)
KS = (1, 2, 5, 64)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def framed(m, clip_frame):
    m = np.array(m, dtype=bool)
    if clip_frame:
        m[0, :] = False; m[-1, :] = False; m[:, 0] = False; m[:, -1] = False
    return m


def ranked(m, clip_frame=False):
    """[(x, y, w, h, area)] of the external contours of boolean image `m`, in the order of the list findContours returns."""
    m = framed(m, clip_frame)
    if not m.any():
        return []
    f = ndi.binary_fill_holes(m)
    lab, n = ndi.label(f, structure=EIGHT)
    fi = f.astype(np.int8)
    b = fi[:-1, :-1] + fi[1:, :-1] + fi[:-1, 1:] + fi[1:, 1:]
    owner = np.maximum(np.maximum(lab[:-1, :-1], lab[1:, :-1]), np.maximum(lab[:-1, 1:], lab[1:, 1:]))   # set pixels of a block share a label
    area2 = 2 * np.bincount(owner[b == 4], minlength=n + 1) + np.bincount(owner[b == 3], minlength=n + 1)
    flat = lab.ravel()
    at = np.flatnonzero(flat)
    of, xs = flat[at], at % lab.shape[1]
    first, last = np.empty(n + 1, np.int64), np.empty(n + 1, np.int64)
    first[of[::-1]] = at[::-1]                     # the last write wins: the first pixel in raster order (set in `m` itself) ...
    last[of] = at                                  # ... and the last one, in the bottom row
    x0, x1 = np.full(n + 1, lab.shape[1]), np.full(n + 1, -1)
    np.minimum.at(x0, of, xs); np.maximum.at(x1, of, xs)
    first, x0, x1, y0, y1 = first[1:], x0[1:], x1[1:], first[1:] // lab.shape[1], last[1:] // lab.shape[1]
    order = np.argsort(-first, kind="stable")
    cols = (x0[order], y0[order], (x1 - x0 + 1)[order], (y1 - y0 + 1)[order], area2[1:][order] / 2.0)
    return list(zip(*(c.tolist() for c in cols)))


def winner(m, clip_frame=False, _ranked=None):
    """The ROI (x, y, w, h) of base.py:568-575 on boolean image `m`, or None."""
    r = ranked(m, clip_frame) if _ranked is None else _ranked
    return max(r, key=lambda c: c[4])[:4] if r else None


def ranking(r, K, min_area):
    """rm_heatmap_to_rois on the list `r` of ranked(): keep area >= min_area, stable sort on -area, the first K."""
    kept = [c for c in r if c[4] >= min_area]
    kept.sort(key=lambda c: -c[4])
    return kept[:K]


def n_components(m, clip_frame=False):
    return ndi.label(framed(m, clip_frame), structure=EIGHT)[1]


def oracle_list(oracle, m, clip_frame=False):
    """The same list from the oracle's border following: [(x, y, w, h, area)] in findContours order."""
    u8 = np.where(m, 255, 0).astype(np.uint8)
    return [oracle.boundingRect(c) + (oracle.contourArea(c),) for c in oracle.findContours(u8, clip_frame=clip_frame)]


# ---- the case table ----------------------------------------------------------------------------------------------------------------
TILE_GEOMETRIES = [(64, 64), (64, 128), (96, 192), (352, 640)]           # rows of whole 64-pixel words: k_ccl_tile / k_ccl_seam / k_ccl_fold
RAGGED_GEOMETRIES = [(1, 1), (1, 200), (200, 1), (3, 3), (33, 70), (65, 129)]
GEOMETRIES = TILE_GEOMETRIES + RAGGED_GEOMETRIES
GPU_GEOMETRIES = [(720, 1280), (1080, 1920)]


def _z(H, W):
    return np.zeros((H, W), bool)


def _seed(name, H, W):
    return [20261019, H, W] + [ord(c) for c in name]


def _noise(dens):
    def make(H, W):
        if H * W < 2:
            return None
        return np.random.default_rng(_seed("noise%g" % dens, H, W)).random((H, W)) < dens
    return make


def _blobs(specks):
    def make(H, W):
        if H < 24 or W < 24:
            return None
        rng = np.random.default_rng(_seed("blobs%g" % specks, H, W))
        m = ndi.gaussian_filter(rng.standard_normal((H, W)), min(H, W) / 16.0) > 0.0
        return m | (rng.random((H, W)) < specks)
    return make


def _diag_square(H, W):
    """a one-pixel line from corner to corner (the largest box, area 0) beside a small solid square (area 9)"""
    if H < 16 or W < 16:
        return None
    m = _z(H, W)
    if W >= H:
        x = np.arange(W); m[x * (H - 1) // (W - 1), x] = True
    else:
        y = np.arange(H); m[y, y * (W - 1) // (H - 1)] = True
    m[2:6, W - 7:W - 3] = True
    return m


def _staircase(H, W):
    """(i, i) and (i, i + 1): two pixels thick, every 2 x 2 block it owns holds three pixels; beside a 3 x 3 square of area 4"""
    if H < 16 or W < 16:
        return None
    m = _z(H, W)
    i = np.arange(1, min(H, W - 1) - 1)
    m[i, i] = True; m[i, i + 1] = True
    m[H - 5:H - 2, 2:5] = True
    return m


def _comb(H, W):
    if H < 16 or W < 16:
        return None
    m = _z(H, W)
    m[2, 2:W - 2] = True; m[2:H - 6, 2:W - 2:2] = True
    m[H - 5:H - 1, 3:W // 3] = True
    return m


def _spiral(H, W):
    if H < 24 or W < 24:
        return None
    m = _z(H, W)
    for k in range(1, min(H, W) // 2 - 6, 4):
        m[k, k:W - k] = True; m[k:H - k, W - 1 - k] = True
        m[H - 1 - k, k + 2:W - k] = True; m[k + 4:H - k, k + 2] = True
    cy, cx = H // 2, W // 2
    if W > H + 16:
        m[cy - 1:cy + 2, cx - (W - H) // 4:cx + (W - H) // 4] = True          # a solid rival in the spiral's eye where there is room for one
    return m


def _plus(H, W):
    if H < 16 or W < 16:
        return None
    m = _z(H, W)
    m[2:H - 2, W // 2 - 1:W // 2 + 2] = True; m[H // 2 - 1:H // 2 + 2, 2:W - 2] = True
    m[3:7, 3:8] = True
    return m


def _checker(H, W):
    """a checkerboard patch (ONE 8-connected component, every background cell a hole) across tile seams, and a solid block"""
    if H < 24 or W < 40:
        return None
    m = _z(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    h, w = min(H - 12, 70), min(W - 2, 140)
    m[(yy >= 1) & (yy <= h) & (xx >= 1) & (xx <= w) & ((yy + xx) % 2 == 0)] = True
    m[H - 8:H - 2, 3:12] = True
    return m


def _frame_block(H, W):
    """a hollow frame one pixel thick (its count bound is tiny, its area is its whole box) beside a solid block with a smaller box"""
    if H < 24 or W < 40:
        return None
    m = _z(H, W)
    h = H // 2
    m[1:h, 1:W // 2] = True; m[2:h - 1, 2:W // 2 - 1] = False
    m[2:h - 2, W // 2 + 2:W - 3] = True
    return m


# shapes of equal area: a 3 x 5 block, a 2 x 9 bar and a diamond of radius 2 all enclose 8; a 3 x 3 square and a 2 x 5 bar enclose 4
def _put(m, y, x, shape):
    if shape == "block":
        m[y:y + 3, x:x + 5] = True
    elif shape == "bar":
        m[y:y + 2, x:x + 9] = True
    elif shape == "diamond":
        for dy in range(-2, 3):
            r = 2 - abs(dy)
            m[y + 2 + dy, x + 2 - r:x + 3 + r] = True
    elif shape == "sq3":
        m[y:y + 3, x:x + 3] = True
    elif shape == "bar5":
        m[y:y + 2, x:x + 5] = True
    elif shape == "col5":
        m[y:y + 5, x:x + 2] = True


TIE_SLOTS = [(2, 30), (4, 3), (13, 16)]           # raster order: the first slot is met first, the last one last


def _tie_perm(perm):
    def make(H, W):
        if H < 24 or W < 44:
            return None
        m = _z(H, W)
        for (y, x), s in zip(TIE_SLOTS, perm):
            _put(m, y, x, s)
        return m
    return make


def _tie_bound(swap):
    """a solid 10 x 12 block, whose count bound settles it, and a hollow 10 x 12 frame, whose border must be followed: both enclose 99"""
    def make(H, W):
        if H < 30 or W < 44:
            return None
        m = _z(H, W)
        a, b = ((3, 4), (16, 25)) if swap else ((16, 25), (3, 4))
        m[a[0]:a[0] + 10, a[1]:a[1] + 12] = True
        m[b[0]:b[0] + 10, b[1]:b[1] + 12] = True; m[b[0] + 1:b[0] + 9, b[1] + 1:b[1] + 11] = False
        return m
    return make


def _tie_three(H, W):
    """three contours of area 4 below a winner of area 25"""
    if H < 24 or W < 44:
        return None
    m = _z(H, W)
    _put(m, 2, 30, "sq3"); _put(m, 4, 3, "bar5"); _put(m, 13, 16, "col5")
    m[12:18, 30:36] = True
    return m


def _ring(m, y, x, h, w):
    m[y:y + h, x:x + w] = True; m[y + 1:y + h - 1, x + 1:x + w - 1] = False


def _ring_island(H, W):
    """a ring of 48 pixels holding an island of 63; a blob outside"""
    if H < 24 or W < 40:
        return None
    m = _z(H, W)
    _ring(m, 1, 2, 12, 14)
    m[4:11, 4:13] = True
    m[16:20, 20:26] = True
    return m


def _ring_diagonal(H, W):
    """... whose island touches a spur of the ring by one corner only: 8-connected to it, so the same component"""
    if H < 24 or W < 40:
        return None
    m = _z(H, W)
    _ring(m, 1, 2, 12, 16)
    m[2, 8] = True                         # the spur, hanging from the top side
    m[3:9, 9:14] = True                    # the island: (3, 9) is diagonal to (2, 8), and no pixel of it is 4-adjacent to the ring
    m[16:20, 20:26] = True
    return m


def _diagonal_pocket(H, W):
    """a diamond outline of diagonal steps only seals a pocket; the pixel inside is nested, not external"""
    if H < 24 or W < 40:
        return None
    m = _z(H, W)
    for dy in range(-4, 5):
        r = 4 - abs(dy)
        m[7 + dy, 10 - r] = True; m[7 + dy, 10 + r] = True
    m[6:9, 10] = True; m[7, 9:12] = True   # a plus inside: |dy| + |dx| <= 1, its 8-neighbours reach 3, the outline is at 4
    m[14:17, 24:27] = True
    return m


def _island_in_island(H, W):
    if H < 24 or W < 40:
        return None
    m = _z(H, W)
    _ring(m, 1, 1, 20, 30); _ring(m, 4, 4, 14, 24); m[7:15, 8:24] = True; m[9:13, 11:21] = False; m[10:12, 13:19] = True
    return m


def _edge_blobs(H, W):
    if H < 24 or W < 40:
        return None
    m = _z(H, W)
    m[0:3, 12:17] = True; m[H - 4:H, 20:27] = True; m[8:12, 0:3] = True; m[7:10, W - 6:W] = True
    m[0:3, 0:4] = True; m[0:2, W - 3:W] = True; m[H - 3:H, 0:2] = True; m[H - 3:H, W - 4:W] = True
    m[H // 2:H // 2 + 3, W // 2:W // 2 + 4] = True
    return m


def _through_frame(H, W):
    """two bars joined through pixels of row 0 only: one component, two once the frame is clipped; and a smaller blob"""
    if H < 24 or W < 40:
        return None
    m = _z(H, W)
    m[0:8, 4:7] = True; m[0:8, 12:16] = True; m[0, 4:16] = True
    m[14:17, 24:28] = True
    return m


def _frame_only(H, W):
    """pixels of the one-pixel frame only: a contour of area (H - 1)(W - 1) that vanishes with the frame clipped"""
    if H < 3 or W < 3:
        return None
    m = _z(H, W)
    m[0, :] = True; m[-1, :] = True; m[:, 0] = True; m[:, -1] = True
    if H >= 24 and W >= 40:
        m[5:9, 6:12] = True                # an island in the frame's hole: external only once the frame is clipped away
    return m


def _empty(H, W):
    return _z(H, W)


FAMILIES = ([("a_noise%g" % d, _noise(d)) for d in (0.05, 0.3, 0.45, 0.62, 0.9)] +
            [("b_blobs", _blobs(0.0)), ("b_blobs_specks", _blobs(0.05))] +
            [("c_diag_square", _diag_square), ("c_staircase", _staircase), ("c_comb", _comb), ("c_spiral", _spiral), ("c_plus", _plus),
             ("c_checker", _checker), ("c_frame_block", _frame_block)] +
            [("d_tie_" + "_".join(p), _tie_perm(p)) for p in itertools.permutations(("block", "bar", "diamond"))] +
            [("d_tie_sq3_bar5", _tie_perm(("sq3", "bar5"))), ("d_tie_bar5_sq3", _tie_perm(("bar5", "sq3"))),
             ("d_tie_bound_a", _tie_bound(False)), ("d_tie_bound_b", _tie_bound(True)), ("d_tie_three", _tie_three)] +
            [("e_ring_island", _ring_island), ("e_ring_diagonal", _ring_diagonal), ("e_diagonal_pocket", _diagonal_pocket),
             ("e_island_in_island", _island_in_island)] +
            [("f_edge_blobs", _edge_blobs), ("f_through_frame", _through_frame), ("f_frame_only", _frame_only)] +
            [("empty", _empty)])
GPU_FAMILIES = [("a_noise0.3", _noise(0.3)), ("b_blobs_specks", _blobs(0.05)), ("c_frame_block", _frame_block)]


class Case:
    """One image: `m` the boolean image, `heat` the 0 / 1 float64 heat map that thresholds to it.  A map without foreground is flat
    (NaN after normalisation, nothing above the threshold, as in the reference); one without background is no case."""

    def __init__(self, name, m):
        assert m.dtype == bool and not m.all()
        self.name, self.m = name, m
        self.heat = np.ascontiguousarray(m, dtype=np.float64)
        self._r = {}

    def __repr__(self):
        return self.name

    def ranked(self, clip):
        if clip not in self._r:
            self._r[clip] = ranked(self.m, clip)
        return self._r[clip]

    def winner(self, clip):
        return winner(None, _ranked=self.ranked(clip))


_CASES = {}


def cases(H, W, families=None):
    key = (H, W, families is None)
    if key not in _CASES:
        out = []
        for name, make in (FAMILIES if families is None else families):
            m = make(H, W)
            if m is not None and not m.all():
                out.append(Case("%s_%dx%d" % (name, H, W), m))
        _CASES[key] = out
    return _CASES[key]


def random_image(rng, hmax=40, wmax=60):
    """one image of the sweep against the oracle: noise of any density, smooth blobs, blobs with specks"""
    H, W = int(rng.integers(1, hmax + 1)), int(rng.integers(1, wmax + 1))
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return rng.random((H, W)) < rng.uniform(0.05, 0.95)
    m = ndi.gaussian_filter(rng.standard_normal((H, W)), float(rng.uniform(0.8, 4.0))) > rng.uniform(-0.3, 0.3) * 0.2
    if kind == 2:
        m = m | (rng.random((H, W)) < 0.05)
    return m


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def check_against_oracle(oracle, m, clip):
    """check 1: the reference's list, in order, and its winner equal the oracle's border following.  Returns the number of contours."""
    got = ranked(m, clip)
    want = oracle_list(oracle, framed(m, False), clip) if m.size else []
    assert got == want, (m.shape, clip, got[:4], want[:4])
    u8 = np.where(m, 255, 0).astype(np.uint8)
    assert winner(None, _ranked=got) == oracle.roi_from_heatmap_u8(u8, THRESHOLD, clip_frame=clip), (m.shape, clip)
    return len(got)


def check_product(be, case, paths=True, lists=True, clip_labelled=True):
    """checks 2 (`paths`) and 3 (`lists`) on one case.  clip_labelled=False: under the <= 3.1 frame rule the labelled path is asked
    for once, not with every switch (rm_roi.hip serves that rule by the host path alone, so the switches change nothing there).  `be` offers dev(heat), roi(handle, clip, labelling), rois(handle, H, W, K, min_area, clip) ->
    (rc, rects, areas, n), set(key, value), stats() -> (count, labelled), path()."""
    from respmon_amd import _capi
    H, W = case.m.shape
    d = be.dev(case.heat)
    for clip in (False, True):
        r = case.ranked(clip)
        want = case.winner(clip)
        tag = (case.name, clip)
        assert be.roi(d, clip, False) == want, tag + ("borders",)
        ncomp = n_components(case.m, clip)
        for bound in ((0, 1) if clip_labelled or not clip else (1,)) if paths else ():
            be.set("host_area_bound", bound)
            try:
                assert be.roi(d, clip, True) == want, tag + ("labelled, host_area_bound", bound)
            finally:
                be.set("host_area_bound", 1)
            n, labelled = be.stats()
            assert bool(labelled) == (not clip), tag         # (the <= 3.1 frame rule is served by the host path alone: rm_roi.hip)
            assert clip or n == ncomp, tag + (n, ncomp)      # one record per 8-connected component
        for tiles in (0, 1) if paths and (clip_labelled or not clip) else ():
            for table in (0, 1):
                be.set("ccl_tiles", tiles); be.set("ccl_table", table)
                try:
                    assert be.roi(d, clip, True) == want, tag + ("ccl_tiles", tiles, "ccl_table", table)
                finally:
                    be.set("ccl_tiles", 1); be.set("ccl_table", -1)
                assert clip or be.stats()[0] == ncomp, tag + ("ccl_tiles", tiles, "ccl_table", table)
        areas = sorted(c[4] for c in r)
        top = areas[-1] if areas else 0.0
        for min_area in (0.0, 0.5, areas[len(areas) // 2] if areas else 3.0, top, top + 0.5) if lists else ():
            for K in KS:
                exp = ranking(r, K, min_area)
                rc, rects, got_areas, n = be.rois(d, H, W, K, min_area, clip)
                assert n == len(exp) and rc == (_capi.RM_OK if exp else _capi.RM_NO_CONTOUR), tag + (K, min_area, n, len(exp), rc)
                assert rects == [c[:4] for c in exp], tag + (K, min_area, rects[:3], exp[:3])
                assert got_areas == [c[4] for c in exp], tag + (K, min_area, got_areas[:3], exp[:3])
                if min_area == 0.0:
                    assert (rects[0] if rects else None) == want, tag + (K,)


def check_table(H=65, W=129):
    """check 4, the part that needs no product: the table holds what its families are for."""
    by = {c.name.rsplit("_", 1)[0]: c for c in cases(H, W)}
    for name, c in by.items():
        if name.startswith("d_tie_") and name not in ("d_tie_three",):
            for clip in (False, True):
                a = sorted((x[4] for x in c.ranked(clip)), reverse=True)
                assert a[0] == a[1], (name, a)                          # the maximum is tied
    for p in itertools.permutations(("block", "bar", "diamond")):
        r = by["d_tie_" + "_".join(p)].ranked(False)
        assert [x[4] for x in r] == [8.0, 8.0, 8.0]
        # the winner is whatever shape stands in the last slot: not the largest box, not the most pixels, not the first met
        y, x = TIE_SLOTS[2]
        w = by["d_tie_" + "_".join(p)].winner(False)
        assert y <= w[1] < y + 5 and x <= w[0] < x + 9, (p, w)
    a = sorted(x[4] for x in by["d_tie_three"].ranked(False))
    assert a == [4.0, 4.0, 4.0, 25.0]
    assert [x[4] for x in by["d_tie_bound_a"].ranked(False)] == [99.0, 99.0]
    # family (c): the component with the largest box bound (w - 1)(h - 1) is not the winner
    r = by["c_diag_square"].ranked(False)
    lead = max(r, key=lambda x: (x[2] - 1) * (x[3] - 1))
    assert lead[4] == 0.0 and by["c_diag_square"].winner(False) != lead[:4] and by["c_diag_square"].winner(False)[2:] == (4, 4)
    r = by["c_staircase"].ranked(False)
    assert max(x[4] for x in r) == min(H, W - 1) - 3 and len(r) == 2                  # two half blocks per step, no full one
    assert len(by["c_checker"].ranked(False)) == 2 and n_components(by["c_checker"].m) == 2
    # family (e): the island holds more pixels than its ring and is not listed
    c = by["e_ring_island"]
    lab, n = ndi.label(c.m, structure=EIGHT)
    sizes = np.bincount(lab.ravel())[1:]
    assert n == 3 and sizes[lab[1, 2] - 1] == 48 and sizes[lab[4, 4] - 1] == 63 and len(c.ranked(False)) == 2
    assert c.winner(False) == (2, 1, 14, 12)
    assert n_components(by["e_ring_diagonal"].m) == 2 and len(by["e_ring_diagonal"].ranked(False)) == 2
    assert n_components(by["e_diagonal_pocket"].m) == 3 and len(by["e_diagonal_pocket"].ranked(False)) == 2
    assert n_components(by["e_island_in_island"].m) == 4 and len(by["e_island_in_island"].ranked(False)) == 1
    # family (f): the two frame conventions differ
    for name in ("f_edge_blobs", "f_through_frame", "f_frame_only"):
        assert by[name].ranked(False) != by[name].ranked(True), name
    assert len(by["f_through_frame"].ranked(False)) == 2 and len(by["f_through_frame"].ranked(True)) == 3
    assert by["f_frame_only"].winner(False) == (0, 0, W, H) and by["f_frame_only"].winner(True) == (6, 5, 6, 4)
    small = cases(3, 3)
    assert [c.name for c in small if c.name.startswith("f_")] == ["f_frame_only_3x3"]
    fo = next(c for c in small if c.name.startswith("f_"))
    assert fo.winner(False) == (0, 0, 3, 3) and fo.winner(True) is None


# ---- check_product's backend interface on the two builds (tests/test_emu_roi_reference.py, tests/test_gpu_roi_reference.py,
# tests/instantiation_cases.py) -------------------------------------------------------------------------------------------------
class EmuRoi:
    """on the emulated C-ABI (tests/emu_harness.py Emu)"""

    def __init__(self, emu):
        self.emu = emu
        self.paths = set()

    def dev(self, heat):
        return heat

    def roi(self, heat, clip, labelling):
        roi = self.emu.heatmap_to_roi(heat, THRESHOLD, clip_frame=clip, labelling=1 if labelling else 0)[0]
        self.paths.add(self.emu.roi_path())
        return roi

    def rois(self, heat, H, W, K, min_area, clip):
        from tests import subjects_cases as sc
        from tests.emu_harness import ptr
        return sc.heatmap_to_rois(self.emu.lib, self.emu.ctx, ptr(heat), H, W, K, min_area, threshold=THRESHOLD, clip=clip)

    def set(self, key, value):
        self.emu.debug_set(key, value)

    def stats(self):
        return self.emu.contour_stats()

    def path(self):
        return self.emu.roi_path()


class GpuRoi:
    """on the product's C-ABI (device heat maps)"""

    def __init__(self):
        import torch
        assert torch.cuda.is_available()
        from respmon_amd import _capi, device, dist
        self.torch, self.device, self.dist = torch, device, dist
        self.lib, self.ctx = _capi.load(), device.ctx()
        self.paths = set()

    def dev(self, heat):
        return self.torch.from_numpy(np.ascontiguousarray(heat)).cuda()

    def roi(self, heat, clip, labelling):
        roi = self.dist.hip_heatmap_to_roi(heat, THRESHOLD, clip_frame=clip, labelling=bool(labelling))
        self.paths.add(self.dist.roi_path())
        return roi

    def rois(self, heat, H, W, K, min_area, clip):
        import ctypes
        from tests import subjects_cases as sc
        return sc.heatmap_to_rois(self.lib, self.ctx, ctypes.c_void_p(heat.data_ptr()), H, W, K, min_area, threshold=THRESHOLD, clip=clip,
                                  stream=self.device.stream_ptr())

    def set(self, key, value):
        self.device.debug_set(key, value)

    def stats(self):
        n, labelled = self.dist.contour_stats()
        return n, int(labelled)

    def path(self):
        return self.dist.roi_path()
