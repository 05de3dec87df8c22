"""
The rate map (include/respmon_hip.h rm_rate_map / rm_window_rate_map): for every pixel of a pyramid level the dominant frequency in
the breathing band and the share of the band's power that sits in that peak -- the estimator of the reference's
prototypes/temporal_analysis.py, for every pixel instead of one ROI signal.  Where the heat map of locate() lights up for any in-band
energy, this tells a chest from a swaying curtain (periodicity) and two subjects under one blanket apart (bpm).
"""
import ctypes

import numpy as np

from . import _capi, device


class RateMap:
    """Device tensors `freq` (Hz, NaN where nothing moves), `power`, `total` (float64) and `index` (int32, -1 where nothing moves) of
    shape [h_level, w_level]; `level` is the pyramid level they belong to (a pixel covers 2^level x 2^level full-resolution pixels)."""

    def __init__(self, freq, power, total, index, level):
        self.freq, self.power, self.total, self.index, self.level = freq, power, total, index, int(level)

    @property
    def bpm(self):
        return self.freq * 60.0

    @property
    def periodicity(self):
        """power / total: the share of the band's power in the peak's grid point; 0 where total == 0"""
        t = device.torch()
        return t.where(self.total == 0, t.zeros_like(self.total), self.power / self.total)

    def roi_bpm(self, roi):
        """Breaths per minute of a full-resolution rectangle (x, y, w, h), e.g. one of locate_all()'s: the power-weighted mean of bpm
        over the level pixels with index >= 0 among columns x >> level .. (x + w - 1) >> level and rows y >> level .. (y + h - 1) >>
        level; None when no pixel qualifies.  Computed on the host."""
        x, y, w, h = (int(v) for v in roi)
        L = self.level
        hl, wl = (int(v) for v in self.freq.shape)
        x0, x1 = max(x >> L, 0), min((x + w - 1) >> L, wl - 1)
        y0, y1 = max(y >> L, 0), min((y + h - 1) >> L, hl - 1)
        if w < 1 or h < 1 or x1 < x0 or y1 < y0:
            return None
        idx = self.index[y0:y1 + 1, x0:x1 + 1].cpu().numpy()
        keep = idx >= 0
        if not keep.any():
            return None
        f = self.freq[y0:y1 + 1, x0:x1 + 1].cpu().numpy()[keep]
        p = self.power[y0:y1 + 1, x0:x1 + 1].cpu().numpy()[keep]
        return float(np.sum(p * (60.0 * f)) / np.sum(p))


def _outputs(shape, dev):
    t = device.torch()
    return (t.empty(shape, dtype=t.float64, device=dev), t.empty(shape, dtype=t.float64, device=dev),
            t.empty(shape, dtype=t.float64, device=dev), t.empty(shape, dtype=t.int32, device=dev))


def level_shape(H, W, level):
    for _ in range(int(level)):
        H, W = (H + 1) // 2, (W + 1) // 2
    return H, W


def buffer_rate_map(frames, fps, freq_min=0.1, freq_max=1.0, level=4, nfreq=64):
    """RateMap of a frame buffer ([T,H,W] of uint8 / uint16 / float16 / float32 / float64, or [T,H,W,3] uint8 BGR; numpy or device tensor) at
    Gaussian pyramid level `level` (1..5): one pass over the frames (rm_rate_map)."""
    device.require_gpu()
    lib = _capi.load()
    buf = device.to_device(frames)
    T, H, W = device.buffer_shape(buf)
    freq, power, total, index = _outputs(level_shape(H, W, level), buf.device)
    _capi.check(lib, lib.rm_rate_map(device.ctx(), device.ptr(buf), device.buffer_dtype_code(buf), T, H, W, int(level), float(fps), float(freq_min),
                                     float(freq_max), int(nfreq), device.ptr(freq), device.ptr(power), device.ptr(total), device.ptr(index),
                                     device.stream_ptr()), "rm_rate_map")
    return RateMap(freq, power, total, index, level)


def window_rate_map(win, fps, freq_min=0.1, freq_max=1.0, nfreq=64):
    """RateMap of the frames a SlidingCalibration holds, read from its ring in place (rm_window_rate_map); level = its skip_levels_at_top"""
    freq, power, total, index = _outputs(level_shape(win.H, win.W, win.skip_levels_at_top), "cuda:%d" % win.device_index)
    _capi.check(win.lib, win.lib.rm_window_rate_map(win._ctx(), win._h, float(fps), float(freq_min), float(freq_max), int(nfreq), device.ptr(freq),
                                                    device.ptr(power), device.ptr(total), device.ptr(index), win._stream()), "rm_window_rate_map")
    return RateMap(freq, power, total, index, win.skip_levels_at_top)


class static_or_instance:
    """RespiratoryMonitor.rate_map(frames, fps) like the static locate(), monitor.rate_map() on the monitor's own buffer: the wrapped
    function receives the instance or None as its first argument."""

    def __init__(self, fn):
        self.fn = fn
        self.__doc__ = fn.__doc__

    def __get__(self, obj, cls=None):
        fn = self.fn

        def bound(*args, **kwargs):
            return fn(obj, *args, **kwargs)
        bound.__doc__ = fn.__doc__
        bound.__name__ = fn.__name__
        return bound


def spectral_operator_host(T, fps, freq_min, freq_max, nfreq):
    lib = _capi.load()
    A = np.empty((2 * int(nfreq), int(T)), dtype=np.float64)
    freqs = np.empty(int(nfreq), dtype=np.float64)
    _capi.check(lib, lib.rm_spectral_operator(int(T), float(fps), float(freq_min), float(freq_max), int(nfreq), ctypes.c_void_p(A.ctypes.data),
                                              ctypes.c_void_p(freqs.ctypes.data)), "rm_spectral_operator")
    return A, freqs
