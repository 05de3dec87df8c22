"""The motion path's edge inputs on the host-emulated build (tests/emu) before they reach the GPU: corners and pyramidal LK on every
crop from 1x1 to 23x23 (the bounding boxes locate() can return for thin blobs), and the PCA reduction against exact arithmetic
on degenerate, collinear, isotropic and extreme-magnitude motion data.  The GPU twin is tests/test_gpu_motion_edges.py."""
import numpy as np
import pytest

from respmon_amd import synth
from tests import motion_reference as mr


@pytest.fixture(scope="module")
def emu():
    from tests.emu_harness import Emu
    return Emu()


class _EmuAdapter:
    """The sweep drivers' backend interface on the emulated C-ABI."""

    def __init__(self, emu):
        self.emu = emu
        self.state = emu.flow_state()
        self.h = self.w = 0

    def gftt(self, img, bs):
        return self.emu.good_features(img, mr.FEATURE["maxCorners"], mr.FEATURE["qualityLevel"], mr.FEATURE["minDistance"], bs)

    def begin(self, img, bs):
        return self.begin_pts(img, mr.FEATURE["maxCorners"], mr.FEATURE["qualityLevel"], mr.FEATURE["minDistance"], bs)

    def begin_pts(self, img, n, q, md, bs):
        self.h, self.w = img.shape
        self.cap = n
        return self.emu.flow_begin(img, 0, 0, self.w, self.h, n, q, md, bs, state=self.state)

    def lk(self, a, b, pts, win, lvl, crit):
        return self.emu.pyr_lk(a, b, pts, win, lvl, crit)

    def step(self, b, win, lvl, crit):
        mean, ng = self.emu.flow_step(b, 0, 0, self.w, self.h, win, lvl, crit, state=self.state)
        return mean, ng, self.emu.flow_points(self.cap, state=self.state)


def test_emu_corners_on_every_small_crop(emu, oracle):
    n = mr.sweep_corners(_EmuAdapter(emu), oracle, synth.synth_texture(64, 64, seed=23))
    assert n == len(mr.SMALL) ** 2 * 2 * 3 * 2


def test_emu_narrow_crops_have_no_corners(emu):
    """h < 3 or w < 3: RM_OK and no corners (OpenCV's "None"), from both entry points; the resident state then steps as with zero
    corners (mean 0, n_good 0)."""
    img = synth.synth_texture(64, 64, seed=23)(0, 0)
    for h, w in ((1, 40), (2, 40), (40, 1), (40, 2), (1, 1), (2, 2)):
        assert emu.good_features(img[:h, :w], 100, 0.3, 7, 7) is None
        st = emu.flow_state()
        assert emu.flow_begin(img, 5, 6, w, h, 100, 0.3, 7, 7, state=st) is None
        mean, ng = emu.flow_step(img, 5, 6, w, h, state=st)
        assert ng == 0 and mean[0] == 0 and mean[1] == 0


def test_emu_lk_on_every_small_crop(emu, oracle):
    n = mr.sweep_lk(_EmuAdapter(emu), oracle, synth.synth_texture(64, 64, seed=23))
    assert n >= len(mr.SMALL) ** 2 * 4


def test_emu_pca_against_exact_arithmetic(emu, oracle):
    worst = 0.0
    for name, m in mr.pca_families(np.random.default_rng(2024)):
        worst = max(worst, mr.check_pca(emu.pca_reduce(m), m, oracle))
    assert worst <= 1.0


def test_emu_lk_limits_are_refused(emu):
    """A window over LK_MAX_WIN taps, and a pyramid of more than LK_MAX_LEVELS levels after lk_max_level's clamping (winSize 3,
    maxLevel 9 on a 1080p crop): RM_E_UNSUPPORTED before anything is launched."""
    from respmon_amd import _capi
    pts = np.array([[[5.0, 5.0]]], np.float32)
    for shape, win, lvl in (((23, 23), (33, 33), 0), ((1080, 1920), (3, 3), 9)):
        img = np.zeros(shape, np.uint8)
        assert mr.lk_expect_unsupported(shape[0], shape[1], win, lvl)
        with pytest.raises(_capi.RespmonError, match=r"\(%d\)" % _capi.RM_E_UNSUPPORTED):
            emu.pyr_lk(img, img, pts, win, lvl)
