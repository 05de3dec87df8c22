"""The magnified video of a LIVE camera: frames in, magnified frames out, chunk by chunk (rm_stream_* and rm_phase_* of
include/respmon_hip.h): LiveMagnifier, the linear Eulerian method, and PhaseMagnifier, the phase-based method on the Riesz pyramid.

eulerian_magnification_video needs the whole [T,H,W] buffer and its band-pass is the reference's FFT operator, which is even in time:
the newest magnified frame mixes in motion of the oldest frame of the buffer.  LiveMagnifier runs the causal Butterworth band-pass of
transforms.temporal_bandpass_filter_sos with its state carried on the device, so every pushed frame comes back magnified at O(1) cost
and the result does not depend on how the stream was cut into pushes."""
import ctypes

import numpy as np

from . import _capi, device


class LiveMagnifier:
    """out[t] = convert(f[t] + raw[t]) for the frames pushed since construction or reset(), f the frame as the calibration reads it
    and raw the second result of transforms.eulerian_magnification_bandpass(frames so far, fps, freq_min, freq_max, amplification,
    pyramid_levels, skip_levels_at_top, temporal_filter_function=transforms.temporal_bandpass_filter_sos), bit for bit
    (start='rest'; the band-pass is Butterworth of `order` as second-order sections, 6 in that function).

    start='steady' (default): the first frame sets the filter state to the steady state of a video that has always shown that frame
    (scipy.signal.sosfilt_zi times the frame's pyramid) -- a band-pass has no DC gain, so the output starts at the frame itself
    instead of seconds of ringing from the step black -> first frame.  start='rest': scipy.signal.sosfilt's default.

    push(frames): [n,H,W] or [H,W] of uint8 / uint16 / float16 / float32 / float64, or [n,H,W,3] / [H,W,3] uint8 BGR; numpy in -> numpy
    out, device tensor in -> device tensor out, of the same number of frames.  out_dtype 'uint8' | 'uint16' | 'float32' | 'float64' (None:
    uint8 for uint8 and BGR input, uint16 for uint16 input, float64 otherwise, as eulerian_magnification_video); color=True: BGR frames in, BGR frames out, the same
    motion on the three channels (rm_magnify_bgr's rule).  A change of fps or band needs a new object."""

    def __init__(self, H, W, fps, freq_min=0.1, freq_max=1.0, amplification=50, pyramid_levels=4, skip_levels_at_top=2, order=6,
                 out_dtype=None, color=False, start='steady', device_index=None):
        from scipy.signal import sosfilt_zi
        from .transforms import butter_bandpass_sos
        t = device.require_gpu()
        if start not in ('steady', 'rest'):
            raise ValueError("start must be 'steady' or 'rest', got %r" % (start,))
        self.lib = _capi.load()
        self.H, self.W = int(H), int(W)
        self.color = bool(color)
        name = None if out_dtype is None else getattr(out_dtype, "__name__", str(out_dtype).replace("torch.", "").replace("numpy.", ""))
        if name not in (None, "uint8", "uint16", "float32", "float64"):
            raise TypeError("out_dtype must be uint8, uint16, float32 or float64, got %r" % (out_dtype,))
        if self.color and name not in (None, "uint8"):
            raise TypeError("out_dtype must be None or uint8 with color=True, got %r" % (out_dtype,))
        self.out_name = name
        self.device_index = t.cuda.current_device() if device_index is None else int(device_index)
        self.sos = np.ascontiguousarray(butter_bandpass_sos(freq_min, freq_max, fps, order=order), dtype=np.float64)
        self.zi = np.ascontiguousarray(sosfilt_zi(self.sos), dtype=np.float64) if start == 'steady' else None
        self._h = ctypes.c_void_p()
        _capi.check(self.lib, self.lib.rm_stream_create(self._ctx(), self.H, self.W, int(pyramid_levels), int(skip_levels_at_top),
                                                        ctypes.c_void_p(self.sos.ctypes.data), self.sos.shape[0],
                                                        None if self.zi is None else ctypes.c_void_p(self.zi.ctypes.data),
                                                        float(amplification), ctypes.byref(self._h)), "rm_stream_create")

    def _ctx(self):
        return device._CTX.get(self.device_index) or device.ctx(self.device_index)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.rm_stream_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _info(self):
        seen, n, b = ctypes.c_longlong(), ctypes.c_size_t(), ctypes.c_size_t()
        _capi.check(self.lib, self.lib.rm_stream_info(self._h, ctypes.byref(seen), ctypes.byref(n), ctypes.byref(b)), "rm_stream_info")
        return seen.value, n.value, b.value

    @property
    def frames_seen(self):
        return self._info()[0]

    @property
    def state_bytes(self):
        return self._info()[2]

    def reset(self):
        """The next push starts a new stream."""
        _capi.check(self.lib, self.lib.rm_stream_reset(self._ctx(), self._h), "rm_stream_reset")

    def push(self, frames):
        t = device.torch()
        x = device.to_device(frames)
        if x.device.index != self.device_index:
            raise ValueError("frames are on device %s, the magnifier on %d" % (x.device, self.device_index))
        single = (x.dim() == 2) or (x.dim() == 3 and x.shape[-1] == 3 and x.dtype == t.uint8 and tuple(x.shape[:2]) == (self.H, self.W))
        if single:
            x = x.unsqueeze(0)
        n, H, W = device.buffer_shape(x)
        if (H, W) != (self.H, self.W):
            raise ValueError("frames are %dx%d, the magnifier was made for %dx%d" % (H, W, self.H, self.W))
        code = device.buffer_dtype_code(x)
        if self.color:
            if code != _capi.RM_BGR8:
                raise ValueError("color=True needs [n,H,W,3] uint8 BGR frames, got %s %s" % (tuple(x.shape), x.dtype))
            out, out_code = t.empty_like(x), _capi.RM_BGR8
        else:
            name = self.out_name or ("uint8" if x.dtype == t.uint8 else "uint16" if x.dtype == t.uint16 else "float64")
            table = {"uint8": (t.uint8, _capi.RM_U8), "uint16": (t.uint16, _capi.RM_U16), "float32": (t.float32, _capi.RM_F32),
                     "float64": (t.float64, _capi.RM_F64)}
            out, out_code = t.empty((n, H, W), dtype=table[name][0], device=x.device), table[name][1]
        if n:
            _capi.check(self.lib, self.lib.rm_stream_push(self._ctx(), self._h, device.ptr(x), code, n, device.ptr(out), out_code,
                                                          ctypes.c_void_p(device.raw_stream(self.device_index))), "rm_stream_push")
        if single:
            out = out[0]
        return device.like_input(out, frames)


class PhaseMagnifier:
    """Phase-based motion magnification on the Riesz pyramid (Wadhwa, Rubinstein, Durand, Freeman, ICCP 2014; rm_phase_* of
    include/respmon_hip.h, where the rule is written out operation by operation).  Where LiveMagnifier adds amplification x band-passed
    INTENSITY -- valid only while amplification x displacement is small against the spatial wavelength, noise amplified alike, pixels
    leaving [0, 1] --, this shifts every processed Laplacian level by amplification x its band-passed local PHASE: larger motions,
    no intensity overshoot, and nothing to settle at the start (the filtered quantity starts at zero, so the first frame comes back as
    it is).  Causal like LiveMagnifier: each pushed frame comes back magnified, the state (5 + 4 x sections doubles per processed
    pyramid pixel) lives on the device, and the result does not depend on how the stream was cut into pushes.

    The band-pass is butter_bandpass_sos(freq_min, freq_max, fps, order) (order <= 8), from rest.  blur=False skips the
    amplitude-weighted blur of the phase (RM_PHASE_NO_BLUR).  Processed levels: skip_levels_at_top .. pyramid_levels - 2.

    Known limits: the three-tap Riesz pair is exact only near spatial frequency pi/2, and the phase blur averages across orientations.
    Prototype figures (numpy, not this library): on oriented structure the motion comes out at 0.74-0.85 of the nominal
    (1 + amplification); on isotropic texture at about 0.65 with the blur and about 0.85 without.

    push(frames): [n,H,W] or [H,W] of uint8 / uint16 / float16 / float32 / float64 (gray only); numpy in -> numpy out, device tensor
    in -> device tensor out.  out_dtype 'uint8' | 'uint16' | 'float32' | 'float64' (None: uint8 for uint8 input, uint16 for uint16 input,
    float64 otherwise) with eulerian_magnification_video's conversions.  A change of fps or band needs a new object."""

    def __init__(self, H, W, fps, freq_min=0.1, freq_max=1.0, amplification=10, pyramid_levels=5, skip_levels_at_top=0, order=1,
                 blur=True, out_dtype=None, device_index=None):
        from .transforms import butter_bandpass_sos
        t = device.require_gpu()
        self.lib = _capi.load()
        self.H, self.W = int(H), int(W)
        name = None if out_dtype is None else getattr(out_dtype, "__name__", str(out_dtype).replace("torch.", "").replace("numpy.", ""))
        if name not in (None, "uint8", "uint16", "float32", "float64"):
            raise TypeError("out_dtype must be uint8, uint16, float32 or float64, got %r" % (out_dtype,))
        self.out_name = name
        self.device_index = t.cuda.current_device() if device_index is None else int(device_index)
        self.sos = np.ascontiguousarray(butter_bandpass_sos(freq_min, freq_max, fps, order=order), dtype=np.float64)
        self._h = ctypes.c_void_p()
        _capi.check(self.lib, self.lib.rm_phase_create(self._ctx(), self.H, self.W, int(pyramid_levels), int(skip_levels_at_top),
                                                       ctypes.c_void_p(self.sos.ctypes.data), self.sos.shape[0], float(amplification),
                                                       0 if blur else _capi.RM_PHASE_NO_BLUR, ctypes.byref(self._h)), "rm_phase_create")

    def _ctx(self):
        return device._CTX.get(self.device_index) or device.ctx(self.device_index)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.rm_phase_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _info(self):
        seen, n, b = ctypes.c_longlong(), ctypes.c_size_t(), ctypes.c_size_t()
        _capi.check(self.lib, self.lib.rm_phase_info(self._h, ctypes.byref(seen), ctypes.byref(n), ctypes.byref(b)), "rm_phase_info")
        return seen.value, n.value, b.value

    @property
    def frames_seen(self):
        return self._info()[0]

    @property
    def state_bytes(self):
        return self._info()[2]

    def reset(self):
        """The next push starts a new sequence."""
        _capi.check(self.lib, self.lib.rm_phase_reset(self._ctx(), self._h), "rm_phase_reset")

    def push(self, frames):
        t = device.torch()
        x = device.to_device(frames)
        if x.device.index != self.device_index:
            raise ValueError("frames are on device %s, the magnifier on %d" % (x.device, self.device_index))
        single = x.dim() == 2
        if single:
            x = x.unsqueeze(0)
        if x.dim() != 3:
            raise ValueError("PhaseMagnifier takes gray frames [n,H,W] or [H,W], got %s" % (tuple(x.shape),))
        n, H, W = device.buffer_shape(x)
        if (H, W) != (self.H, self.W):
            raise ValueError("frames are %dx%d, the magnifier was made for %dx%d" % (H, W, self.H, self.W))
        code = device.buffer_dtype_code(x)
        name = self.out_name or ("uint8" if x.dtype == t.uint8 else "uint16" if x.dtype == t.uint16 else "float64")
        table = {"uint8": (t.uint8, _capi.RM_U8), "uint16": (t.uint16, _capi.RM_U16), "float32": (t.float32, _capi.RM_F32),
                 "float64": (t.float64, _capi.RM_F64)}
        out, out_code = t.empty((n, H, W), dtype=table[name][0], device=x.device), table[name][1]
        if n:
            _capi.check(self.lib, self.lib.rm_phase_push(self._ctx(), self._h, device.ptr(x), code, n, device.ptr(out), out_code,
                                                         ctypes.c_void_p(device.raw_stream(self.device_index))), "rm_phase_push")
        if single:
            out = out[0]
        return device.like_input(out, frames)
