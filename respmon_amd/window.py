"""
The calibration on a sliding window (include/respmon_hip.h rm_window_*): a ring of per-frame pyramid rows on the device takes the place
of the resident [T,H,W] calibration buffer.  Frames are pushed as the camera delivers them -- each goes through the frame-buffer
kernel once -- and the ROI is taken from the ring at any moment, bit for bit what RespiratoryMonitor.locate gives on the stacked
frames the ring holds.  Memory is T x NP x 8 bytes (17 MB instead of 4.2 GB at 1080p x 256, skip 4).
"""
import ctypes

import numpy as np

from . import _capi, device


class SlidingCalibration:
    """T frames of H x W; pyramid_levels / skip_levels_at_top and the hyper-parameter defaults of the calls are those of
    RespiratoryMonitor.locate, whose class switches (opencv_contours_clip_frame, reference_operation_order) are read at construction
    as locate() reads them per call.  skip_levels_at_top >= 1."""

    def __init__(self, T, H, W, pyramid_levels=9, skip_levels_at_top=4, flags=0, device_index=None):
        from .base import RespiratoryMonitor
        t = device.require_gpu()
        self.lib = _capi.load()
        self.T, self.H, self.W = int(T), int(H), int(W)
        self.skip_levels_at_top = int(skip_levels_at_top)
        self.device_index = t.cuda.current_device() if device_index is None else int(device_index)
        self.flags = int(flags) | (_capi.RM_FLAG_CONTOUR_CLIP_FRAME if RespiratoryMonitor.opencv_contours_clip_frame else 0) | \
            (_capi.RM_FLAG_FILTER_LAPLACIANS if RespiratoryMonitor.reference_operation_order else 0)
        self._h = ctypes.c_void_p()
        _capi.check(self.lib, self.lib.rm_window_create(self._ctx(), self.T, self.H, self.W, int(pyramid_levels), int(skip_levels_at_top),
                                                        self.flags, ctypes.byref(self._h)), "rm_window_create")

    def _ctx(self):
        return device._CTX.get(self.device_index) or device.ctx(self.device_index)

    def _stream(self):
        return ctypes.c_void_p(device.raw_stream(self.device_index))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.rm_window_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ state
    def _info(self):
        c, h, n, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        _capi.check(self.lib, self.lib.rm_window_info(self._h, ctypes.byref(c), ctypes.byref(h), ctypes.byref(n), ctypes.byref(b)), "rm_window_info")
        return c.value, h.value, int(n.value), int(b.value)

    @property
    def count(self):
        """frames held: min(frames pushed since the last reset, T)"""
        return self._info()[0]

    @property
    def head(self):
        return self._info()[1]

    @property
    def ring_bytes(self):
        return self._info()[3]

    def reset(self):
        """forget the frames held; the ring memory is kept"""
        _capi.check(self.lib, self.lib.rm_window_reset(self._ctx(), self._h), "rm_window_reset")

    # ------------------------------------------------------------------ frames in
    def push(self, frames, bgr=False):
        """One frame [H,W] or many [n,H,W] of uint8 / uint16 / float16 / float32 / float64 (the values uint8_to_float gives, as in a calibration
        buffer of that dtype); with bgr=True, BGR frames as captured: uint8 [H,W,3] or [n,H,W,3].  numpy or device tensor;
        asynchronous.  Successive pushes may differ in dtype.  Returns the number of frames pushed."""
        x = device.to_device(frames)
        if x.dim() == (3 if bgr else 2):
            x = x.unsqueeze(0)
        want = (self.H, self.W, 3) if bgr else (self.H, self.W)
        if x.dim() != len(want) + 1 or tuple(x.shape[1:]) != want or (bgr and x.dtype != device.torch().uint8):
            raise ValueError("frames must be [H,W] or [n,H,W] (bgr=True: uint8 [H,W,3] or [n,H,W,3]) with H x W = %d x %d, got %s %s"
                             % (self.H, self.W, tuple(x.shape), x.dtype))
        n = int(x.shape[0])
        if n == 0:
            return 0
        _capi.check(self.lib, self.lib.rm_window_push(self._ctx(), self._h, device.ptr(x), device.buffer_dtype_code(x), n, self._stream()),
                    "rm_window_push")
        return n

    # ------------------------------------------------------------------ ROI out
    def heatmap(self, fps, freq_min=0.1, freq_max=1.0, amplification=500, temporal_threshold=0.7):
        """float64 [H,W] device tensor: the heat map locate() thresholds (rm_window_calibrate)"""
        t = device.torch()
        heat = t.empty((self.H, self.W), dtype=t.float64, device="cuda:%d" % self.device_index)
        _capi.check(self.lib, self.lib.rm_window_calibrate(self._ctx(), self._h, float(fps), float(freq_min), float(freq_max), float(amplification),
                                                           float(temporal_threshold), device.ptr(heat), self._stream()), "rm_window_calibrate")
        return heat

    def locate(self, fps, freq_min=0.1, freq_max=1.0, amplification=500, temporal_threshold=0.7, threshold=20):
        """(x, y, w, h) or None: RespiratoryMonitor.locate on the frames held, oldest first (rm_window_locate)"""
        xywh = (ctypes.c_int32 * 4)()
        rc = _capi.check(self.lib, self.lib.rm_window_locate(self._ctx(), self._h, float(fps), float(freq_min), float(freq_max), float(amplification),
                                                             float(temporal_threshold), int(threshold), xywh, self._stream()), "rm_window_locate")
        return None if rc == _capi.RM_NO_CONTOUR else (xywh[0], xywh[1], xywh[2], xywh[3])

    def locate_all(self, fps, max_rois=4, min_area=0.0, freq_min=0.1, freq_max=1.0, amplification=500, temporal_threshold=0.7, threshold=20):
        """list of (x, y, w, h), largest contour first: RespiratoryMonitor.locate_all on the frames held (rm_window_locate_multi)"""
        cap = max(int(max_rois), 1)
        xywh = np.zeros((cap, 4), dtype=np.int32)
        n = ctypes.c_int(0)
        _capi.check(self.lib, self.lib.rm_window_locate_multi(self._ctx(), self._h, float(fps), float(freq_min), float(freq_max), float(amplification),
                                                              float(temporal_threshold), int(threshold), int(max_rois), float(min_area),
                                                              ctypes.c_void_p(xywh.ctypes.data), None, ctypes.byref(n), self._stream()),
                    "rm_window_locate_multi")
        return [tuple(int(v) for v in xywh[i]) for i in range(n.value)]

    # ------------------------------------------------------------------ rate out
    def rate_map(self, fps, freq_min=0.1, freq_max=1.0, nfreq=64):
        """rate.RateMap of the frames held (at least two), at pyramid level skip_levels_at_top: per pixel the dominant frequency in the
        band and its share of the band's power, read from the ring in place (rm_window_rate_map).  Needs the default operation order
        (the ring rows are the Gaussian level then)."""
        from . import rate
        return rate.window_rate_map(self, fps, freq_min, freq_max, nfreq)
