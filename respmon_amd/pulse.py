"""
The pulse beside the breath (include/respmon_hip.h rm_bgr_block_sums / rm_bgr_roi_sums / rm_pulse_pos / rm_pulse_map): POS, "plane
orthogonal to skin" (Wang, den Brinker, Stuijk, de Haan, Algorithmic Principles of Remote PPG, IEEE TBME 2017), on the three channels
of a BGR frame buffer.  Everything else here measures luma; the pulse is a sub-level colour change of skin that a gray mean cannot tell
from a flicker of the lamp.  Per block of the frame POS gives a pulse map -- skin is where the map is periodic, no face detector
needed --, per rectangle a pulse signal for the subjects locate_all() returns.  Gray and 16-bit buffers carry no chroma and are refused.
"""
import ctypes
import math

import numpy as np

from . import _capi, device
from .rate import RateMap, _outputs

BLOCKS = (4, 8, 16, 32, 64)


def _bgr(frames):
    buf = device.to_device(frames)
    if not device.is_bgr_buffer(buf):
        raise ValueError("POS needs the three colour channels: a [N,H,W,3] uint8 BGR buffer, got %s %s (a gray buffer holds no pulse "
                         "signal for POS)" % (tuple(buf.shape), str(buf.dtype).replace("torch.", "")))
    return buf


def default_window(fps):
    """the paper's 1.6 s in frames"""
    return int(math.ceil(1.6 * float(fps)))


def block_sums(frames, block=16):
    """[N,H,W,3] uint8 BGR -> device uint32 [N, ceil(H / block), ceil(W / block), 3]: the sum of each channel over each block
    (rm_bgr_block_sums); edge blocks are partial."""
    t = device.require_gpu()
    lib = _capi.load()
    buf = _bgr(frames)
    N, H, W = device.buffer_shape(buf)
    block = int(block)
    if block not in BLOCKS:
        raise ValueError("block must be one of %s, got %r" % (BLOCKS, block))
    out = t.empty((N, -(-H // block), -(-W // block), 3), dtype=t.uint32, device=buf.device)
    _capi.check(lib, lib.rm_bgr_block_sums(device.ctx(), device.ptr(buf), N, H, W, block, device.ptr(out), device.stream_ptr()), "rm_bgr_block_sums")
    return out


def _roi_array(rois):
    r = np.ascontiguousarray(np.asarray(rois, dtype=np.int32).reshape(-1, 4))
    if len(r) < 1:
        raise ValueError("at least one rectangle (x, y, w, h) is needed")
    return r


def roi_sums(frames, rois):
    """[N,H,W,3] uint8 BGR and K rectangles (x, y, w, h) -> device uint32 [N, K, 3]: the sum of each channel over each rectangle
    (rm_bgr_roi_sums)."""
    t = device.require_gpu()
    lib = _capi.load()
    buf = _bgr(frames)
    N, H, W = device.buffer_shape(buf)
    r = _roi_array(rois)
    out = t.empty((N, len(r), 3), dtype=t.uint32, device=buf.device)
    _capi.check(lib, lib.rm_bgr_roi_sums(device.ctx(), device.ptr(buf), N, H, W, ctypes.c_void_p(r.ctypes.data), len(r), device.ptr(out),
                                         device.stream_ptr()), "rm_bgr_roi_sums")
    return out


def pos(sums, window):
    """uint32 channel sums [N, ..., 3] -> device float64 [N, ...]: the POS pulse signal of every column with sliding windows of `window`
    frames, overlap-added (rm_pulse_pos)."""
    t = device.require_gpu()
    lib = _capi.load()
    s = device.to_device(sums)
    if s.dtype != t.uint32 or s.dim() < 2 or s.shape[-1] != 3:
        raise ValueError("sums must be uint32 [N, ..., 3], got %s %s" % (tuple(s.shape), s.dtype))
    N, shape = int(s.shape[0]), tuple(s.shape[1:-1])
    out = t.empty((N,) + shape, dtype=t.float64, device=s.device)
    _capi.check(lib, lib.rm_pulse_pos(device.ctx(), device.ptr(s), N, int(np.prod(shape, dtype=np.int64)), int(window), device.ptr(out),
                                      device.stream_ptr()), "rm_pulse_pos")
    return out


def pulse_map(frames, fps, block=16, window=None, freq_min=0.7, freq_max=3.0, nfreq=64):
    """The pulse map of a [N,H,W,3] uint8 BGR buffer: a rate.RateMap over the blocks of the frame with level = log2(block), so bpm,
    periodicity and roi_bpm(roi) work as on a rate map -- the dominant frequency of the POS signal of every block in the pulse band
    (42 - 180 bpm by default) and the share of the band's power in it (rm_pulse_map).  `window`: frames per POS window (default
    ceil(1.6 fps), the paper's 1.6 s)."""
    device.require_gpu()
    lib = _capi.load()
    buf = _bgr(frames)
    N, H, W = device.buffer_shape(buf)
    block = int(block)
    if block not in BLOCKS:
        raise ValueError("block must be one of %s, got %r" % (BLOCKS, block))
    window = default_window(fps) if window is None else int(window)
    freq, power, total, index = _outputs((-(-H // block), -(-W // block)), buf.device)
    _capi.check(lib, lib.rm_pulse_map(device.ctx(), device.ptr(buf), N, H, W, block, window, float(fps), float(freq_min), float(freq_max), int(nfreq),
                                      device.ptr(freq), device.ptr(power), device.ptr(total), device.ptr(index), device.stream_ptr()), "rm_pulse_map")
    return RateMap(freq, power, total, index, BLOCKS.index(block) + 2)


def pulse_signal(frames, rois, fps, window=None):
    """One POS pulse signal per rectangle: device float64 [N, K] (rm_bgr_roi_sums, then rm_pulse_pos)"""
    return pos(roi_sums(frames, rois), default_window(fps) if window is None else int(window))


def pulse_rate(frames, rois, fps, window=None, freq_min=0.7, freq_max=3.0, nfreq=64):
    """Per rectangle (bpm, periodicity): the spectral peak (rm_spectral_peak) of its POS signal in the pulse band and the share of the
    band's power in the peak's grid point; (None, 0.0) for a rectangle whose signal never changes."""
    from .transforms import spectral_peak
    sp = spectral_peak(pulse_signal(frames, rois, fps, window), fps, freq_min, freq_max, nfreq)
    freq, power, total, index = (v.cpu().numpy() for v in sp)
    return [(None, 0.0) if index[k] < 0 else (60.0 * float(freq[k]), float(power[k] / total[k]) if total[k] > 0 else 0.0) for k in range(len(index))]
