"""Device-backed counterparts of the reference's transforms.py hot-path functions (same names,
argument meaning and return conventions).  numpy in -> numpy out; CUDA tensor in -> tensor out."""
import collections
import ctypes
import logging

import numpy as np

from . import _capi, device


def uint8_to_float(img):
    """reference transforms.py:20-23: img * (1./255) as float64."""
    t = device.require_gpu()
    lib = _capi.load()
    src = device.to_device(img, t.uint8)
    dst = t.empty(src.shape, dtype=t.float64, device=src.device)
    _capi.check(lib, lib.rm_uint8_to_float(device.ctx(), device.ptr(src), device.ptr(dst), src.numel(), device.stream_ptr()),
                "rm_uint8_to_float")
    return device.like_input(dst, img)


def float_to_uint8(img):
    """reference transforms.py:26-29: img*255 stored into uint8 (C truncation)."""
    t = device.require_gpu()
    lib = _capi.load()
    src = device.to_device(img, t.float64)
    dst = t.empty(src.shape, dtype=t.uint8, device=src.device)
    _capi.check(lib, lib.rm_float_to_uint8(device.ctx(), device.ptr(src), device.ptr(dst), src.numel(), device.stream_ptr()),
                "rm_float_to_uint8")
    return device.like_input(dst, img)


def uint16_to_float(img):
    """The 16-bit counterpart of uint8_to_float (ours; the reference has no 16-bit path): img * (1./65535) as float64, one
    multiplication by the rounded constant (rm_uint16_to_float).  It is the number every kernel makes of a uint16 pixel."""
    t = device.require_gpu()
    lib = _capi.load()
    src = device.to_device(img, t.uint16)
    dst = t.empty(src.shape, dtype=t.float64, device=src.device)
    _capi.check(lib, lib.rm_uint16_to_float(device.ctx(), device.ptr(src), device.ptr(dst), src.numel(), device.stream_ptr()),
                "rm_uint16_to_float")
    return device.like_input(dst, img)


def float_to_uint16(img):
    """The 16-bit counterpart of float_to_uint8: img*65535 stored into uint16 (C truncation, low 16 bits; NaN -> 0)."""
    t = device.require_gpu()
    lib = _capi.load()
    src = device.to_device(img, t.float64)
    dst = t.empty(src.shape, dtype=t.uint16, device=src.device)
    _capi.check(lib, lib.rm_float_to_uint16(device.ctx(), device.ptr(src), device.ptr(dst), src.numel(), device.stream_ptr()),
                "rm_float_to_uint16")
    return device.like_input(dst, img)


def bgr_buffer_to_gray(buf):
    """[T,H,W,3] uint8 -> [T,H,W] uint8: cv2.cvtColor(BGR2GRAY) of every frame (base.py:230) on the device (rm_bgr_to_gray) -- what the
    calibration kernels do on the fly with an RM_BGR8 buffer, for the entry points that take gray frames."""
    t = device.require_gpu()
    lib = _capi.load()
    src = device.to_device(buf)
    if not device.is_bgr_buffer(src):
        raise TypeError("expected a [T,H,W,3] uint8 buffer")
    gray = t.empty(tuple(src.shape[:3]), dtype=t.uint8, device=src.device)
    _capi.check(lib, lib.rm_bgr_to_gray(device.ctx(), device.ptr(src), gray.numel(), device.ptr(gray), device.stream_ptr()), "rm_bgr_to_gray")
    return gray


def temporal_operator(n, fps, freq_min, freq_max):
    """The reference's rfft / mask / Re(ifft) filter (transforms.py:86-98) as its explicit n x n matrix
    (without the amplification) plus (bound_low, bound_high).  Host only; needs no GPU."""
    lib = _capi.load()
    M = np.empty((n, n), dtype=np.float64)
    lo, hi = ctypes.c_int(), ctypes.c_int()
    _capi.check(lib, lib.rm_temporal_operator(int(n), float(fps), float(freq_min), float(freq_max),
                                              ctypes.c_void_p(M.ctypes.data), ctypes.byref(lo), ctypes.byref(hi)),
                "rm_temporal_operator")
    return M, lo.value, hi.value


def temporal_bandpass_filter_fft(data, fps, freq_min=0.833, freq_max=1, axis=0,
                                 amplification_factor=50, verbose=False, debug=''):
    """reference transforms.py:82-102 (packed-rfft mask quirk kept).  `data` is [T,h,w]; like the
    reference the inverse transform always runs along axis 0, so only axis=0 is accepted."""
    if axis != 0:
        raise NotImplementedError("the reference's ifft is hard-wired to axis 0 (transforms.py:98); only axis=0 is meaningful")
    t = device.require_gpu()
    lib = _capi.load()
    x = device.to_device(data, t.float64)
    T = x.shape[0]
    npix = x[0].numel()
    out = t.empty(x.shape, dtype=t.float64, device=x.device)
    _capi.check(lib, lib.rm_temporal_bandpass_filter_fft(device.ctx(), device.ptr(x), T, npix, float(fps), float(freq_min),
                                                         float(freq_max), float(amplification_factor), device.ptr(out),
                                                         device.stream_ptr()), "rm_temporal_bandpass_filter_fft")
    if verbose:
        print('{0}{1},{2}'.format(debug, float(out.min()), float(out.max())))
    return device.like_input(out, data)


def spectral_operator(T, fps, freq_min, freq_max, nfreq):
    """(A, freqs): the [2 nfreq, T] operator of spectral_peak -- row 2j / 2j+1 the Blackman-Harris windowed cosine / minus sine of
    freqs[j] with the mean removal folded in -- and its frequency grid (rm_spectral_operator).  Host only; needs no GPU."""
    from . import rate
    return rate.spectral_operator_host(T, fps, freq_min, freq_max, nfreq)


SpectralPeak = collections.namedtuple("SpectralPeak", "freq power total index")


def spectral_peak(data, fps, freq_min=0.1, freq_max=1.0, nfreq=64):
    """The frequency estimate of the reference's prototypes/temporal_analysis.py (Blackman-Harris window, spectrum of sig - sig.mean(),
    argmax, parabolic(log .)) for every column of `data` [T, ...] at once, on a grid of `nfreq` frequencies from freq_min to freq_max
    instead of the FFT bins (rm_spectral_peak; definition in include/respmon_hip.h).  Returns the named tuple (freq, power, total,
    index) shaped data.shape[1:]: the refined peak frequency in Hz (NaN for a column that never changes), the power at the peak's grid
    point, the power summed over the grid, and the grid point (-1 for such a column).  numpy in -> numpy out; device tensor in ->
    device tensors out."""
    t = device.require_gpu()
    lib = _capi.load()
    x = device.to_device(data, t.float64)
    T = x.shape[0]
    shape = tuple(x.shape[1:])
    freq = t.empty(shape, dtype=t.float64, device=x.device)
    power, total = t.empty_like(freq), t.empty_like(freq)
    index = t.empty(shape, dtype=t.int32, device=x.device)
    _capi.check(lib, lib.rm_spectral_peak(device.ctx(), device.ptr(x), T, freq.numel(), float(fps), float(freq_min), float(freq_max), int(nfreq),
                                          device.ptr(freq), device.ptr(power), device.ptr(total), device.ptr(index), device.stream_ptr()),
                "rm_spectral_peak")
    return SpectralPeak(*(device.like_input(v, data) for v in (freq, power, total, index)))


def butter_bandpass(_lowcut, _highcut, _fs, order=5):
    """reference transforms.py:38-44: Butterworth band-pass design (host, scipy like the reference)."""
    from scipy.signal import butter
    _nyq = 0.5 * _fs
    _b, _a = butter(order, [_lowcut / _nyq, _highcut / _nyq], btype='band', output='ba')
    return _b, _a


def butter_bandpass_filter(_data, _lowcut, _highcut, _fs, order=5):
    """reference transforms.py:47-50: lfilter along the LAST axis (1-D signals in the reference; host scipy)."""
    from scipy.signal import lfilter
    _b, _a = butter_bandpass(_lowcut, _highcut, _fs, order=order)
    return lfilter(_b, _a, _data)


def butter_bandpass_filter_fast(_data, _b, _a, axis=0):
    """reference transforms.py:53-55: scipy.signal.lfilter(b, a, data, axis).  Videos ([T,...], axis 0) run on the
    device (rm_lfilter: one lane per pixel, the recurrence in scipy's operation order); anything else is a small
    host-side signal and goes to scipy like the reference."""
    x_in = _data
    is_tensor = hasattr(_data, "is_cuda")
    if axis != 0 or (not is_tensor and np.ndim(_data) < 2):
        from scipy.signal import lfilter
        return lfilter(_b, _a, _data.cpu().numpy() if is_tensor else _data, axis=axis)
    t = device.require_gpu()
    lib = _capi.load()
    x = device.to_device(x_in, t.float64)
    T = x.shape[0]
    npix = x[0].numel()
    out = t.empty(x.shape, dtype=t.float64, device=x.device)
    b = np.ascontiguousarray(_b, dtype=np.float64)
    a = np.ascontiguousarray(_a, dtype=np.float64)
    n = max(len(b), len(a))
    b = np.concatenate([b, np.zeros(n - len(b))])
    a = np.concatenate([a, np.zeros(n - len(a))])
    _capi.check(lib, lib.rm_lfilter(device.ctx(), device.ptr(x), T, npix, ctypes.c_void_p(b.ctypes.data),
                                    ctypes.c_void_p(a.ctypes.data), n, 1.0, device.ptr(out), device.stream_ptr()), "rm_lfilter")
    return device.like_input(out, x_in)


def butter_lowpass(cutoff, fs, order=5):
    """reference transforms.py:58-63."""
    from scipy.signal import butter
    return butter(order, cutoff / (0.5 * fs), btype='low', analog=False)


def temporal_bandpass_filter(data, fps, freq_min=0.833, freq_max=1, axis=0,
                             amplification_factor=50, verbose=False, debug=''):
    """reference transforms.py:72-79: order-6 Butterworth band-pass (lfilter) along `axis`, times the
    amplification -- the IIR alternative to temporal_bandpass_filter_fft.

    The reference's `ba` form is numerically UNSTABLE at camera rates: in float64 the order-6 design has poles outside the unit
    circle (fps 30, 0.1-0.5 Hz: largest pole 1.056, |y| reaches 1.7e19 within 2 000 samples of uniform noise in [0, 1]; fps 30,
    0.1-1.0 Hz: 1.015 and 3e11; at fps 60 the output overflows; stable only at low rates such as fps 10, largest pole 0.986).  This
    function keeps the reference's behaviour; temporal_bandpass_filter_sos is the same design as second-order sections (largest pole
    0.9963 at fps 30, 0.1-0.5 Hz; |y| <= 0.29 on the same input)."""
    b, a = butter_bandpass(freq_min, freq_max, fps, order=6)
    result = butter_bandpass_filter_fast(data, b, a, axis=axis)
    result *= amplification_factor
    if verbose:
        print('{0}{1},{2}'.format(debug, float(result.min()), float(result.max())))
    return result


def butter_bandpass_sos(_lowcut, _highcut, _fs, order=6):
    """butter_bandpass's design (transforms.py:38-44) as second-order sections [order, 6] (host, scipy)."""
    from scipy.signal import butter
    _nyq = 0.5 * _fs
    return butter(order, [_lowcut / _nyq, _highcut / _nyq], btype='band', output='sos')


def sosfilt_device(data, sos, zi=None, scale=1.0):
    """scipy.signal.sosfilt(sos, data, axis=0) * scale on the device (rm_sosfilt: one lane per element, scipy's operation order);
    `zi` [n_sections, 2] (scipy.signal.sosfilt_zi): every element starts at zi * data[0], the steady state of its first sample."""
    t = device.require_gpu()
    lib = _capi.load()
    x = device.to_device(data, t.float64)
    out = t.empty(x.shape, dtype=t.float64, device=x.device)
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    z = None if zi is None else np.ascontiguousarray(zi, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or (z is not None and z.shape != (sos.shape[0], 2)):
        raise ValueError("sos must be [n_sections, 6] and zi [n_sections, 2]")
    _capi.check(lib, lib.rm_sosfilt(device.ctx(), device.ptr(x), x.shape[0], x[0].numel(), ctypes.c_void_p(sos.ctypes.data), sos.shape[0],
                                    None if z is None else ctypes.c_void_p(z.ctypes.data), float(scale), device.ptr(out),
                                    device.stream_ptr()), "rm_sosfilt")
    return device.like_input(out, data)


def temporal_bandpass_filter_sos(data, fps, freq_min=0.833, freq_max=1, axis=0,
                                 amplification_factor=50, verbose=False, debug=''):
    """temporal_bandpass_filter with its order-6 Butterworth band-pass as second-order sections: scipy.signal.sosfilt(sos, data,
    axis) * amplification, from rest.  The reference's filter signature, so eulerian_magnification_bandpass(temporal_filter_function=
    temporal_bandpass_filter_sos) takes it; stable where the `ba` form is not (see temporal_bandpass_filter).  Videos ([T,...], axis 0)
    run on the device (rm_sosfilt); anything else is a small host-side signal and goes to scipy, as in butter_bandpass_filter_fast."""
    sos = butter_bandpass_sos(freq_min, freq_max, fps, order=6)
    is_tensor = hasattr(data, "is_cuda")
    if axis != 0 or (not is_tensor and np.ndim(data) < 2):
        from scipy.signal import sosfilt
        result = sosfilt(sos, data.cpu().numpy() if is_tensor else data, axis=axis) * amplification_factor
    else:
        result = sosfilt_device(data, sos, scale=float(amplification_factor))
    if verbose:
        print('{0}{1},{2}'.format(debug, float(result.min()), float(result.max())))
    return result


def eulerian_magnification_bandpass(vid_data, fps, freq_min, freq_max, amplification,
                                    pyramid_levels=4, skip_levels_at_top=2, verbose=False,
                                    temporal_filter_function=None, threshold=0.7):
    """reference transforms.py:144-198 -> (bandpassed_data, raw_bandpassed_data), both [T,H,W] float64.
    This is the MATERIALISING form kept for API parity; calibration itself uses the fused path
    (RespiratoryMonitor.locate -> rm_calibrate) that never writes a [T,H,W] array.
    `temporal_filter_function` defaults to temporal_bandpass_filter_fft (one fused C-ABI call); any other
    callable with the reference's filter signature (e.g. temporal_bandpass_filter, or a plain scipy filter) runs the
    reference's own sequence -- pyramid, filter per level, collapse, mask; the callable is handed numpy levels when
    `vid_data` is numpy and device tensors when it is a device tensor."""
    t = device.require_gpu()
    lib = _capi.load()
    vid = device.to_device(vid_data)
    T, H, W = device.buffer_shape(vid)
    if vid.dim() == 4 and not (temporal_filter_function is None or temporal_filter_function is temporal_bandpass_filter_fft):
        vid = bgr_buffer_to_gray(vid)
    masked = t.empty((T, H, W), dtype=t.float64, device=vid.device)
    mm = (ctypes.c_double * 2)()
    if temporal_filter_function is None or temporal_filter_function is temporal_bandpass_filter_fft:
        raw = t.empty((T, H, W), dtype=t.float64, device=vid.device)
        _capi.check(lib, lib.rm_eulerian_magnification_bandpass(device.ctx(), device.ptr(vid), device.buffer_dtype_code(vid), T, H, W,
                                                                float(fps), float(freq_min), float(freq_max), float(amplification),
                                                                int(pyramid_levels), int(skip_levels_at_top), float(threshold),
                                                                device.ptr(masked), device.ptr(raw), mm, device.stream_ptr()),
                    "rm_eulerian_magnification_bandpass")
    else:
        from . import pyramid
        vid_pyramid = pyramid.create_laplacian_video_pyramid(vid, pyramid_levels)                    # transforms.py:148
        bandpassed = [t.zeros_like(lv) for lv in vid_pyramid]                                       # :150-152
        for i, lv in enumerate(vid_pyramid):                                                         # :156-170
            if i < skip_levels_at_top or i >= len(vid_pyramid) - 1:
                continue
            # the callable sees what the caller works in: numpy levels for numpy input (a scipy / numpy filter with the
            # reference's signature must run unchanged), device tensors for device input
            bandpassed[i] = device.to_device(temporal_filter_function(device.like_input(lv, vid_data), fps, freq_min=freq_min,
                                                                      freq_max=freq_max, amplification_factor=amplification,
                                                                      debug='{0},{1}:'.format('n/a', i), verbose=verbose), t.float64)
        raw = pyramid.collapse_laplacian_video_pyramid(bandpassed)                                   # :182
        _capi.check(lib, lib.rm_threshold_mask(device.ctx(), device.ptr(raw), raw.numel(), float(threshold), device.ptr(masked), mm,
                                               device.stream_ptr()), "rm_threshold_mask")           # :184-192
    if verbose:
        logging.info("eulerian_magnification_bandpass: min=%r max=%r", mm[0], mm[1])
    return device.like_input(masked, vid_data), device.like_input(raw, vid_data)


def eulerian_magnification_video(vid_data, fps, freq_min, freq_max, amplification,
                                 pyramid_levels=4, skip_levels_at_top=2, out_dtype=None, color=False):
    """The magnified video the reference computes and leaves unused: transforms.py:170 adds the band-passed levels into the video's own
    Laplacian pyramid, transforms.py:181 is the commented-out collapse of it.  [T,H,W] = frame + raw_bandpassed_data (what
    eulerian_magnification_bandpass returns second), one float64 addition per pixel, formed in one fused pass over the frame buffer
    (rm_magnify) without a [T,H,W] float64 intermediate.
    `vid_data`: [T,H,W] uint8 / uint16 / float16 / float32 / float64 or [T,H,W,3] uint8 BGR; numpy in -> numpy out, device tensor in ->
    device tensor out.  `out_dtype`: 'uint8' (clamped to [0, 1] first, then float_to_uint8's truncation -- the clamp is this library's),
    'uint16' (the same clamp, then float_to_uint16's truncation), 'float32' or 'float64' (numpy / torch dtypes are accepted too); None:
    uint8 for uint8 and BGR input, uint16 for uint16 input, float64 otherwise.
    `color=True` (rm_magnify_bgr): `vid_data` must be a [T,H,W,3] uint8 BGR buffer and the result is the [T,H,W,3] uint8 BGR video with
    the same band-passed motion (that of the gray image) added to the three channels -- luma magnified, chroma left alone; `out_dtype`
    None or uint8.  The default gives the gray video, also for BGR input."""
    t = device.require_gpu()
    lib = _capi.load()
    vid = device.to_device(vid_data)
    T, H, W = device.buffer_shape(vid)

    def dtype_name(d):
        return getattr(d, "__name__", str(d).replace("torch.", "").replace("numpy.", ""))

    if color:
        if not device.is_bgr_buffer(vid):
            raise ValueError("color=True needs a [T,H,W,3] uint8 BGR frame buffer, got %s %s" % (tuple(vid.shape), vid.dtype))
        if out_dtype is not None and dtype_name(out_dtype) != "uint8":
            raise TypeError("out_dtype must be None or uint8 with color=True, got %r" % (out_dtype,))
        out = t.empty_like(vid)
        _capi.check(lib, lib.rm_magnify_bgr(device.ctx(), device.ptr(vid), T, H, W, float(fps), float(freq_min), float(freq_max),
                                            float(amplification), int(pyramid_levels), int(skip_levels_at_top), device.ptr(out),
                                            device.stream_ptr()), "rm_magnify_bgr")
        return device.like_input(out, vid_data)
    if out_dtype is None:
        out_dtype = "uint8" if vid.dtype == t.uint8 else "uint16" if vid.dtype == t.uint16 else "float64"
    name = dtype_name(out_dtype)
    code = device.buffer_dtype_code(vid)
    table = {"uint8": (t.uint8, _capi.RM_U8), "uint16": (t.uint16, _capi.RM_U16), "float32": (t.float32, _capi.RM_F32),
             "float64": (t.float64, _capi.RM_F64)}
    if name not in table:
        raise TypeError("out_dtype must be uint8, uint16, float32 or float64, got %r" % (out_dtype,))
    out = t.empty((T, H, W), dtype=table[name][0], device=vid.device)
    _capi.check(lib, lib.rm_magnify(device.ctx(), device.ptr(vid), code, T, H, W, float(fps), float(freq_min), float(freq_max),
                                    float(amplification), int(pyramid_levels), int(skip_levels_at_top), device.ptr(out), table[name][1],
                                    device.stream_ptr()), "rm_magnify")
    return device.like_input(out, vid_data)


def phase_magnification_video(vid_data, fps, freq_min, freq_max, amplification, pyramid_levels=5, skip_levels_at_top=0, order=1,
                              blur=True, out_dtype=None):
    """Phase-based motion magnification of a whole clip (Riesz pyramid; rm_phase_* of include/respmon_hip.h): one
    live.PhaseMagnifier, one push.  Unlike eulerian_magnification_video it stays valid when amplification x displacement is no longer
    small against the spatial wavelength, does not amplify noise with the motion and keeps the pixels near the input's range; its
    band-pass is the causal Butterworth butter_bandpass_sos(freq_min, freq_max, fps, order) from rest, and the first frame comes back
    as it is.  `vid_data`: gray [T,H,W] uint8 / uint16 / float16 / float32 / float64; numpy in -> numpy out, device tensor in -> device
    tensor out; `out_dtype` as eulerian_magnification_video.
    Known limits: the three-tap Riesz pair is exact only near spatial frequency pi/2, and the phase blur averages across orientations.
    Prototype figures (numpy, not this library): 0.74-0.85 of the nominal (1 + amplification) on oriented structure; on isotropic
    texture about 0.65 with the blur and about 0.85 with blur=False."""
    from .live import PhaseMagnifier
    vid = device.to_device(vid_data)
    if vid.dim() != 3:
        raise ValueError("phase_magnification_video takes a gray [T,H,W] buffer, got %s" % (tuple(vid.shape),))
    with PhaseMagnifier(vid.shape[1], vid.shape[2], fps, freq_min, freq_max, amplification, pyramid_levels, skip_levels_at_top, order=order,
                        blur=blur, out_dtype=out_dtype, device_index=vid.device.index) as pm:
        return device.like_input(pm.push(vid), vid_data)


def stabilize_video(vid_data, out_dtype=None, return_shifts=False, model="shift", crop=False, **kw):
    """A clip of a shaky camera registered to its first frame (rm_stab_* of include/respmon_hip.h): one stabilize.Stabilizer(H, W,
    **kw), one push -- per frame the global shift against the first frame, then the bilinear warp by it.  `vid_data`: [T,H,W] gray or
    [T,H,W,3] uint8 BGR; numpy in -> numpy out, device tensor in -> device tensor out; **kw: max_shift, levels, iterations.
    return_shifts=True: (frames, shifts [T,2], flags [T]).
    model='similarity' (rm_stab_sim_*): rotation, zoom and shift, for a camera in a hand; **kw also max_linear, linear_level, and
    return_shifts gives params [T,4] (p0, p1, tx, ty).  crop=True: the frames cut to stabilize.valid_rect(), the part the replicated
    border cannot reach."""
    from .stabilize import stabilize_video as _stabilize_video
    return _stabilize_video(vid_data, out_dtype=out_dtype, return_shifts=return_shifts, model=model, crop=crop, **kw)


def butter_lowpass_filter(data, cutoff, fs, order=5):
    """reference transforms.py:58-69 (used by measure(), base.py:342): 128-sample 1-D signal, host scipy."""
    from scipy.signal import butter, filtfilt
    b, a = butter(order, cutoff / (0.5 * fs), btype='low', analog=False)
    return filtfilt(b, a, data)
