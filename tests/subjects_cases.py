"""Shared by tests/test_emu_subjects.py and tests/test_gpu_subjects.py (not a test module): small heat maps whose thresholded image
is known, the ranked contour list the oracle derives from it, and thin callers of the multi-subject C-ABI that work on raw pointers
(numpy memory for the host-emulated build, device memory on the GPU).

The expected list is the definition in include/respmon_hip.h restated with the oracle's cv2 stand-ins:
    contours = findContours(thresh, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)      (with clip_frame as set)
    keep contourArea(c) >= min_area; stable sort on -area over the list order; boundingRect + area of the first K.
"""
import ctypes

import numpy as np

from respmon_amd import _capi

THRESHOLD = 20
GEOMETRIES = [(33, 70), (48, 100),      # rows that are not whole 64-pixel words
              (40, 64), (64, 128),      # rows of whole words: the k_heat_rows_u8 / tile-labelling geometry of the single-ROI stage
              (1, 1), (3, 200)]
KS = (1, 2, 5, 64)


# ---- images (uint8 0 / 1, [H, W]) ----------------------------------------------------------------------------------------------
def _rect(img, y, x, h, w):
    img[y:y + h, x:x + w] = 1


def _empty(H, W):
    return np.zeros((H, W), np.uint8)


def _one_blob(H, W):
    if H < 8 or W < 12:
        return None
    img = _empty(H, W)
    _rect(img, H // 4, W // 4, H // 3, W // 3)
    _rect(img, H // 4 + 2, W // 4 - 2, 3, 2)           # a bump: not a plain rectangle
    return img


def _five_blobs(H, W):
    img = _empty(H, W)
    if H >= 14 and W >= 60:
        for i, (h, w) in enumerate([(3, 4), (9, 7), (5, 5), (7, 10), (4, 8)]):     # areas (h-1)(w-1) = 6, 48, 16, 54, 21
            _rect(img, 1 + (i % 2) * 2, 2 + i * 12, h, w)
        return img
    if H == 3 and W >= 40:
        x = 1
        for w in (3, 6, 2, 5, 4):                                                  # 3 rows high: areas 4, 10, 2, 8, 6
            _rect(img, 0, x, 3, w)
            x += w + 2
        return img
    return None


def _ties(order):
    """Two or three blobs of exactly equal area at different raster positions; `order` moves which one the raster scan meets first."""
    def make(H, W):
        if H < 12 or W < 40:
            return None
        img = _empty(H, W)
        if order == "two_a":            # same shape, the left one starts higher
            _rect(img, 2, 3, 4, 6); _rect(img, 5, 20, 4, 6)
        elif order == "two_b":          # ... the right one starts higher
            _rect(img, 5, 3, 4, 6); _rect(img, 2, 20, 4, 6)
        elif order == "two_shapes":     # 3 x 5 and 2 x 9: both area 8, different boxes, same top row (the left one is met first)
            _rect(img, 4, 3, 3, 5); _rect(img, 4, 20, 2, 9)
        elif order == "three":          # three equal ones and a larger and a smaller one around them
            _rect(img, 1, 30, 3, 4); _rect(img, 6, 2, 3, 4); _rect(img, 6, 12, 3, 4)
            _rect(img, 1, 2, 4, 8); _rect(img, 8, 30, 2, 2)
        return img
    return make


def _ring_island(H, W):
    if H < 14 or W < 30:
        return None
    img = _empty(H, W)
    _rect(img, 1, 2, 11, 13)
    img[2:11, 3:14] = 0                    # a ring one pixel thick ...
    _rect(img, 5, 7, 3, 3)                 # ... with an island inside: not an external contour
    _rect(img, 3, 20, 4, 5)                # and a blob outside
    return img


def _edges(H, W):
    if H < 12 or W < 40:
        return None
    img = _empty(H, W)
    _rect(img, 0, 10, 3, 5)                # top edge
    _rect(img, H - 4, 20, 4, 7)            # bottom edge
    _rect(img, 5, 0, 4, 3)                 # left edge
    _rect(img, 4, W - 6, 3, 6)             # right edge
    _rect(img, H - 3, W - 4, 3, 4)         # bottom-right corner
    img[0, 0] = 1                          # the top-left corner pixel: gone altogether with the frame clipped
    _rect(img, 5, 12, 3, 4)                # interior
    return img


def _edges_flat(H, W):
    if not (H == 3 and W >= 40):
        return None
    img = _empty(H, W)
    _rect(img, 0, 0, 3, 4); _rect(img, 0, 10, 2, 5); _rect(img, 1, 20, 2, 6); _rect(img, 0, W - 5, 3, 5); _rect(img, 1, 30, 1, 4)
    return img


def _diagonals(H, W):
    if H < 12 or W < 40:
        return None
    img = _empty(H, W)
    for i in range(7):
        img[1 + i, 2 + i] = 1              # a diagonal chain: 8-connected, one contour of area 0
        img[1 + i, 20 - i] = 1             # an anti-diagonal one
    for i in range(10):
        img[2 + (i % 2) * 2 + (i % 3 == 0), 24 + i] = 1        # a zigzag that encloses nothing
    img[9, 30] = img[10, 31] = img[9, 32] = img[8, 31] = 1     # a diamond around one hole pixel: area 2
    return img


def _pixels_lines(H, W):
    if W < 40:
        return None
    img = _empty(H, W)
    mid = H // 2
    img[mid, 2] = 1                        # single pixels: area 0
    img[mid, 5] = 1
    _rect(img, mid, 8, 1, 9)               # 1 x n line: area 0
    if H >= 8:
        _rect(img, 1, 22, 6, 1)            # n x 1 line
        _rect(img, 2, 26, 2, 2)            # area 1
    else:
        _rect(img, 0, 26, 2, 2)
    img[mid, W - 1] = 1                    # a single pixel on the frame
    return img


def _checker(H, W):
    if H < 14 or W < 40:
        return None
    img = _empty(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    patch = (yy >= 1) & (yy < 9) & (xx >= 2) & (xx < 14)
    img[patch & ((yy + xx) % 2 == 0)] = 1                      # a checkerboard: ONE 8-connected component full of holes
    dots = (yy >= 2) & (yy < 12) & (xx >= 18) & (xx < 38)
    img[dots & (yy % 2 == 0) & (xx % 2 == 0)] = 1              # every other pixel both ways: fifty tiny contours
    return img


def _random(H, W):
    if H * W < 2000:
        return None
    rng = np.random.default_rng(20261017 + H * 1000 + W)
    return (rng.random((H, W)) < 0.30).astype(np.uint8)


CONTENTS = [("empty", _empty), ("one_blob", _one_blob), ("five_blobs", _five_blobs), ("tie_two_a", _ties("two_a")),
            ("tie_two_b", _ties("two_b")), ("tie_two_shapes", _ties("two_shapes")), ("tie_three", _ties("three")),
            ("ring_island", _ring_island), ("edges", _edges), ("edges_flat", _edges_flat), ("diagonals", _diagonals),
            ("pixels_lines", _pixels_lines), ("checker", _checker), ("random30", _random)]


def heat_of(img):
    """A float64 heat map whose image under base.py:563-566 (normalise, float_to_uint8, threshold 20) is `img`: foreground 1.0 or
    0.09 (uint8 255 / 22), background 0.0 or 0.07 (uint8 0 / 17), with the extrema 0 and 1 both present.  An image without
    foreground becomes a flat map (0 / 0 -> NaN -> uint8 0 -> no contour, as in the reference); so does one without background,
    which therefore is not a case."""
    H, W = img.shape
    if not img.any():
        return np.zeros((H, W))
    assert not img.all()
    yy, xx = np.mgrid[0:H, 0:W]
    heat = np.where(img > 0, np.where((yy + xx) % 3 == 0, 0.09, 1.0), np.where((yy + xx) % 2 == 0, 0.07, 0.0))
    fy, fx = np.argwhere(img > 0)[0]
    by, bx = np.argwhere(img == 0)[0]
    heat[fy, fx] = 1.0
    heat[by, bx] = 0.0
    return np.ascontiguousarray(heat, dtype=np.float64)


class Case:
    def __init__(self, name, img, clip):
        self.name, self.img, self.clip = name, img, clip
        self.heat = heat_of(img)
        self._ranked = None

    def __repr__(self):
        return self.name

    def all_contours(self, oracle):
        """[(area, (x, y, w, h))] in the order of the list findContours returns, computed once."""
        if self._ranked is None:
            _, u8 = oracle.heatmap_u8(self.heat[None])
            _, binary = oracle.threshold(u8, THRESHOLD, 255)
            assert np.array_equal(binary != 0, self.img != 0), "the heat map does not threshold to the intended image"
            cs = oracle.findContours(binary, clip_frame=self.clip)
            self._ranked = [(oracle.contourArea(c), oracle.boundingRect(c)) for c in cs]
        return self._ranked

    def expected(self, oracle, K, min_area):
        kept = [r for r in self.all_contours(oracle) if r[0] >= min_area]
        kept.sort(key=lambda r: -r[0])       # stable: equal areas keep the list order
        return kept[:K]

    def min_areas(self, oracle):
        """0, 0.5, one equal to an existing area (>= keeps it), one above the maximum."""
        areas = sorted({a for a, _ in self.all_contours(oracle)})
        existing = areas[len(areas) // 2] if areas else 3.0
        return [0.0, 0.5, existing, (areas[-1] if areas else 0.0) + 1.0]

    def ks(self, oracle):
        n = len(self.all_contours(oracle))
        return list(KS) + ([n + 3] if n + 3 <= _capi.RM_MAX_ROIS and n + 3 not in KS else [])


def cases():
    out = []
    for H, W in GEOMETRIES:
        for name, make in CONTENTS:
            img = make(H, W)
            if img is None or img.all():
                continue
            for clip in (False, True):
                out.append(Case("%s_%dx%d%s" % (name, H, W, "_clip" if clip else ""), img, clip))
    return out


CASES = cases()


# ---- the C-ABI on raw pointers --------------------------------------------------------------------------------------------------
def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def heatmap_to_rois(lib, ctx, heat_ptr, H, W, K, min_area, threshold=THRESHOLD, clip=False, stream=None, want_area=True):
    """-> (rc, [(x, y, w, h)], [area], n): the raw return code (a refusal is an answer), the entries the call wrote"""
    xywh = np.full((max(K, 1), 4), -7, np.int32)
    area = np.full(max(K, 1), -7.0)
    n = ctypes.c_int(-7)
    lib.rm_set_contour_clip_frame(ctx, 1 if clip else 0)
    try:
        rc = lib.rm_heatmap_to_rois(ctx, heat_ptr, H, W, threshold, K, float(min_area), _vp(xywh), _vp(area) if want_area else None,
                                    ctypes.byref(n), stream)
    finally:
        lib.rm_set_contour_clip_frame(ctx, 0)
    m = max(n.value, 0)
    return rc, [tuple(int(v) for v in r) for r in xywh[:m]], [float(a) for a in area[:m]], n.value


def roi_mean_multi_clip(lib, ctx, frames_ptr, code, N, H, W, rois, out=None, stream=None):
    """-> (rc, out [N, K])"""
    r = np.ascontiguousarray(rois, dtype=np.int32).reshape(-1, 4)
    if out is None:
        out = np.full((N, len(r)), -7.0)
    rc = lib.rm_roi_mean_multi_clip(ctx, frames_ptr, code, N, H, W, _vp(r), len(r), _vp(out), stream)
    return rc, out


def check_case(oracle, case, call, single):
    """Every K and min_area of `case`: call(K, min_area) -> (rc, rois, areas, n) against the oracle's ranking; single() -> the ROI of
    the single-ROI function on the same image (or None), which entry 0 must equal whenever min_area == 0."""
    one = single()
    for K in case.ks(oracle):
        for min_area in case.min_areas(oracle):
            want = case.expected(oracle, K, min_area)
            rc, rois, areas, n = call(K, min_area)
            tag = (case.name, K, min_area)
            assert n == len(want), tag + (n, len(want))
            assert rc == (_capi.RM_OK if want else _capi.RM_NO_CONTOUR), tag + (rc,)
            assert rois == [r for _, r in want], tag + (rois, want)
            assert areas == [a for a, _ in want], tag + (areas, want)
            if min_area == 0.0:
                assert (rois[0] if rois else None) == one, tag + (rois[:1], one)


# ---- clips for the multi-ROI means ---------------------------------------------------------------------------------------------
CLIP_DTYPES = (np.uint8, np.float16, np.float32, np.float64)


def small_clip(dtype, N=5, H=20, W=37, seed=5):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, (N, H, W), dtype=np.uint8)
    return rng.random((N, H, W)).astype(dtype)


def small_rois(K, H=20, W=37, seed=11):
    """overlapping, repeated, 1 x 1 and full-frame rectangles first, seeded random ones behind them"""
    fixed = [(3, 2, 17, 9), (10, 5, 20, 12), (10, 5, 20, 12), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, H), (5, 0, 3, H), (0, 7, W, 1)]
    rng = np.random.default_rng(seed)
    while len(fixed) < K:
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        fixed.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    if K == 1:
        return [fixed[0]]
    if K == 3:
        return [fixed[0], fixed[1], fixed[2]]
    return fixed[:K]


# ---- a calibration buffer with three subjects -----------------------------------------------------------------------------------
def three_subject_clip(seed, amplitudes, T=64, H=96, W=128, fps=10.0, breath_hz=0.4, noise=0.01):
    """uint8 [T,H,W] in the manner of respmon_amd.synth.synth_breathing: a static low-pass texture, white noise, and three Gaussian
    blobs whose brightness oscillates in phase at `breath_hz` with the given amplitudes."""
    from respmon_amd import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    tex = synth._lowpass_noise(rng, H, W)
    g = 255.0 * (0.5 + 0.25 * tex)[None] + 255.0 * noise * rng.standard_normal((T, H, W))
    s = np.sin(2 * np.pi * breath_hz * np.arange(T) / fps)[:, None, None]
    for (cy, cx), amp in zip(((0.27, 0.22), (0.30, 0.75), (0.74, 0.50)), amplitudes):
        yy = (np.arange(H)[:, None] - cy * H) / (0.09 * H)
        xx = (np.arange(W)[None, :] - cx * W) / (0.07 * W)
        g = g + (amp * 255.0 * np.exp(-0.5 * (yy * yy + xx * xx)))[None] * s
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


# Pinned for the locate tests: seed 3, amplitudes 0.20 / 0.15 / 0.11.  The oracle alone gives three contours at threshold 20, with
# areas 299.0 (18, 17, 21, 19), 207.0 (88, 21, 17, 17) and 96.0 (58, 66, 13, 11): pairwise far apart, no tie decides the ranking.
THREE_SEED, THREE_AMPS = 3, (0.20, 0.15, 0.11)
THREE_AREAS = [299.0, 207.0, 96.0]
# ... and a second buffer for the alternating sequences, whose strongest blob is another one: the oracle gives 298.0 (86, 19, 21, 20),
# 174.5 (56, 64, 17, 15) and 73.0 (23, 21, 11, 10), so rm_locate answers differently on the two buffers
OTHER_SEED, OTHER_AMPS = 7, (0.10, 0.20, 0.14)
OTHER_ROI = (86, 19, 21, 20)

LOCATE_KW = dict(fps=10.0, freq_min=0.1, freq_max=1.0, amplification=500, pyramid_levels=5, skip_levels_at_top=2,
                 temporal_threshold=0.7, threshold=THRESHOLD)


def locate_multi(lib, ctx, frames_ptr, code, T, H, W, K, min_area=0.0, flags=0, stream=None, kw=LOCATE_KW):
    """rm_locate_multi -> (rc, [(x, y, w, h)], [area])"""
    xywh = np.full((max(K, 1), 4), -7, np.int32)
    area = np.full(max(K, 1), -7.0)
    n = ctypes.c_int(-7)
    rc = lib.rm_locate_multi(ctx, frames_ptr, code, T, H, W, float(kw["fps"]), float(kw["freq_min"]), float(kw["freq_max"]),
                             float(kw["amplification"]), kw["pyramid_levels"], kw["skip_levels_at_top"], float(kw["temporal_threshold"]),
                             kw["threshold"], flags, K, float(min_area), _vp(xywh), _vp(area), ctypes.byref(n), stream)
    m = max(n.value, 0)
    return rc, [tuple(int(v) for v in r) for r in xywh[:m]], [float(a) for a in area[:m]]


def locate(lib, ctx, frames_ptr, code, T, H, W, flags=0, stream=None, kw=LOCATE_KW):
    """rm_locate -> (x, y, w, h) or None"""
    xywh = np.zeros(4, np.int32)
    rc = _capi.check(lib, lib.rm_locate(ctx, frames_ptr, code, T, H, W, float(kw["fps"]), float(kw["freq_min"]), float(kw["freq_max"]),
                                        float(kw["amplification"]), kw["pyramid_levels"], kw["skip_levels_at_top"],
                                        float(kw["temporal_threshold"]), kw["threshold"], flags, _vp(xywh), stream), "rm_locate")
    return None if rc == _capi.RM_NO_CONTOUR else tuple(int(v) for v in xywh)


def oracle_ranking(oracle, frames_u8, clip=False, kw=LOCATE_KW):
    """[(area, (x, y, w, h))] of the oracle's calibration of the buffer, ranked: eulerian_magnification_bandpass -> heatmap_u8 ->
    threshold -> findContours / contourArea / boundingRect, stable sort on -area."""
    masked, _ = oracle.eulerian_magnification_bandpass(oracle.uint8_to_float(frames_u8), kw["fps"], kw["freq_min"], kw["freq_max"],
                                                       kw["amplification"], pyramid_levels=kw["pyramid_levels"],
                                                       skip_levels_at_top=kw["skip_levels_at_top"], threshold=kw["temporal_threshold"])
    _, u8 = oracle.heatmap_u8(masked)
    _, binary = oracle.threshold(u8, kw["threshold"], 255)
    ranked = [(oracle.contourArea(c), oracle.boundingRect(c)) for c in oracle.findContours(binary, clip_frame=clip)]
    ranked.sort(key=lambda r: -r[0])
    return ranked
