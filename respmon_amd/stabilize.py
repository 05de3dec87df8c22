"""A shaky camera taken out of the frames before anything else looks at them (rm_stab_* and rm_warp_shift of include/respmon_hip.h,
where the rule is written out operation by operation).

Every method of this package assumes a camera that stands still.  A webcam on a monitor arm, a phone leaned on a shelf moves by a
pixel or two from frame to frame; that motion is broadband, part of it falls into the breathing band, and locate() then finds
background texture.  Stabilizer estimates, per frame, the global shift against a FIXED reference frame (translation-only
Gauss-Newton, coarse to fine on the library's Gaussian pyramid) and resamples the frame by it (bilinear, replicated border).  The
reference is the first frame after construction or reset(), or the frame given to set_reference(); it never drifts, so a frame's
result depends on neither the other frames of a push nor on how a stream is cut into pushes.

Not covered: rotation, zoom, rolling shutter, a camera that pans on purpose (the reference would have to follow), cropping of the
replicated border the warp leaves at the frame's edge."""
import ctypes

import numpy as np

from . import _capi, device

FLAG_LEVEL_SKIPPED = 1   # a level had no usable gradient (a flat reference) or no region (a tiny frame): it did not contribute
FLAG_CLAMPED = 2         # the last update ran into max_shift: the frame has probably moved further than that


class Stabilizer:
    """Stabilizer(H, W, max_shift=8.0, levels=(3, 0), iterations=2): levels = (coarse, fine) pyramid levels of the estimate,
    `iterations` Gauss-Newton steps per level (a fixed count: nothing terminates on data), max_shift in pixels (at most 64).  Two
    iterations recover about one pixel of the coarsest level per level, so the coarse level should satisfy 2^coarse >= max_shift.

    push(frames, out_dtype=None) -> (frames, shifts [N,2], flags [N]); estimate(frames) -> (shifts, flags); warp(frames, shifts);
    set_reference(frame); reset().  Frames are [N,H,W] or [H,W] of uint8 / uint16 / float16 / float32 / float64, or [N,H,W,3] / [H,W,3]
    uint8 BGR (estimated on its gray value, warped channel by channel); numpy in -> numpy out, device tensor in -> device tensor out.
    out_dtype 'uint8' | 'uint16' | 'float32' | 'float64' (None: uint8 for uint8 input, uint16 for uint16 input, float64 otherwise);
    BGR frames come back as BGR uint8.  shifts[n] = (dx, dy): the displacement of frame n's content against the reference, positive
    toward +x / +y; flags: FLAG_LEVEL_SKIPPED, FLAG_CLAMPED."""

    def __init__(self, H, W, max_shift=8.0, levels=(3, 0), iterations=2, device_index=None):
        t = device.require_gpu()
        self.lib = _capi.load()
        self.H, self.W = int(H), int(W)
        self.device_index = t.cuda.current_device() if device_index is None else int(device_index)
        self._h = ctypes.c_void_p()
        _capi.check(self.lib, self.lib.rm_stab_create(self._ctx(), self.H, self.W, int(levels[0]), int(levels[1]), int(iterations), float(max_shift),
                                                      ctypes.byref(self._h)), "rm_stab_create")

    def _ctx(self):
        return device._CTX.get(self.device_index) or device.ctx(self.device_index)

    def _stream(self):
        return ctypes.c_void_p(device.raw_stream(self.device_index))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.rm_stab_destroy(self._h)
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
        seen, ref, b = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_size_t()
        _capi.check(self.lib, self.lib.rm_stab_info(self._h, ctypes.byref(seen), ctypes.byref(ref), ctypes.byref(b)), "rm_stab_info")
        return seen.value, bool(ref.value), b.value

    @property
    def frames_seen(self):
        return self._info()[0]

    @property
    def has_reference(self):
        return self._info()[1]

    @property
    def state_bytes(self):
        return self._info()[2]

    def reset(self):
        """The next frame becomes the reference."""
        _capi.check(self.lib, self.lib.rm_stab_reset(self._ctx(), self._h), "rm_stab_reset")

    def _frames(self, frames):
        """(device buffer [n,H,W(,3)], whether a single frame came in)"""
        t = device.torch()
        x = device.to_device(frames)
        if x.device.index != self.device_index:
            raise ValueError("frames are on device %s, the stabiliser on %d" % (x.device, self.device_index))
        single = x.dim() == 2 or (x.dim() == 3 and x.shape[-1] == 3 and x.dtype == t.uint8 and tuple(x.shape[:2]) == (self.H, self.W))
        if single:
            x = x.unsqueeze(0)
        n, h, w = device.buffer_shape(x)
        if (h, w) != (self.H, self.W):
            raise ValueError("frames are %dx%d, the stabiliser was made for %dx%d" % (h, w, self.H, self.W))
        return x, single

    @staticmethod
    def _out(x, out_dtype):
        """(an empty output buffer for x, its dtype code)"""
        t = device.torch()
        code = device.buffer_dtype_code(x)
        name = None if out_dtype is None else getattr(out_dtype, "__name__", str(out_dtype).replace("torch.", "").replace("numpy.", ""))
        if code == _capi.RM_BGR8:
            if name not in (None, "uint8"):
                raise TypeError("BGR frames come back as uint8 BGR, got out_dtype %r" % (out_dtype,))
            return t.empty_like(x), _capi.RM_BGR8
        table = {"uint8": (t.uint8, _capi.RM_U8), "uint16": (t.uint16, _capi.RM_U16), "float32": (t.float32, _capi.RM_F32),
                 "float64": (t.float64, _capi.RM_F64)}
        name = name or ("uint8" if x.dtype == t.uint8 else "uint16" if x.dtype == t.uint16 else "float64")
        if name not in table:
            raise TypeError("out_dtype must be uint8, uint16, float32 or float64, got %r" % (out_dtype,))
        return t.empty(tuple(x.shape), dtype=table[name][0], device=x.device), table[name][1]

    def set_reference(self, frame):
        """`frame` ([H,W], or [H,W,3] uint8 BGR) becomes the reference of every later frame."""
        x, single = self._frames(frame)
        if x.shape[0] != 1:
            raise ValueError("set_reference takes one frame, got %s" % (tuple(x.shape),))
        _capi.check(self.lib, self.lib.rm_stab_set_reference(self._ctx(), self._h, device.ptr(x), device.buffer_dtype_code(x), self._stream()),
                    "rm_stab_set_reference")

    def _push(self, frames, out_dtype, want_frames):
        x, single = self._frames(frames)
        n = int(x.shape[0])
        out, out_code = self._out(x, out_dtype) if want_frames else (None, _capi.RM_U8)
        shifts, flags = np.zeros((n, 2)), np.zeros(n, np.int32)
        if n:
            _capi.check(self.lib, self.lib.rm_stab_push(self._ctx(), self._h, device.ptr(x), device.buffer_dtype_code(x), n, device.ptr(out), out_code,
                                                        ctypes.c_void_p(shifts.ctypes.data), ctypes.c_void_p(flags.ctypes.data), self._stream()), "rm_stab_push")
        if out is not None:
            out = device.like_input(out[0] if single else out, frames)
        return out, shifts, flags

    def push(self, frames, out_dtype=None):
        """(stabilised frames, shifts [N,2], flags [N]); with no reference set the first frame becomes it and comes back with shift (0, 0)"""
        return self._push(frames, out_dtype, True)

    def estimate(self, frames):
        """(shifts [N,2], flags [N]) of push(frames), without the warp"""
        return self._push(frames, None, False)[1:]

    def warp(self, frames, shifts, out_dtype=None):
        """frames resampled by the caller's shifts [N,2] (rm_warp_shift): out[n][y][x] = bilinear(frames[n], x + dx, y + dy)"""
        x, single = self._frames(frames)
        n = int(x.shape[0])
        s = np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1, 2)
        if len(s) != n:
            raise ValueError("%d shifts for %d frames" % (len(s), n))
        out, out_code = self._out(x, out_dtype)
        if n:
            _capi.check(self.lib, self.lib.rm_warp_shift(self._ctx(), device.ptr(x), device.buffer_dtype_code(x), n, self.H, self.W,
                                                         ctypes.c_void_p(s.ctypes.data), device.ptr(out), out_code, self._stream()), "rm_warp_shift")
            return device.like_input(out[0] if single else out, frames)


def stabilize_video(vid, out_dtype=None, return_shifts=False, **kw):
    """A whole clip registered to its first frame: one Stabilizer(H, W, **kw), one push.  `vid`: [T,H,W] gray or [T,H,W,3] uint8 BGR;
    numpy in -> numpy out, device tensor in -> device tensor out.  return_shifts=True: (frames, shifts [T,2], flags [T])."""
    x = device.to_device(vid)
    T, H, W = device.buffer_shape(x)
    with Stabilizer(H, W, device_index=x.device.index, **kw) as st:
        out, shifts, flags = st.push(x, out_dtype)
    out = device.like_input(out, vid)
    return (out, shifts, flags) if return_shifts else out


class StabilizedCapture:
    """StabilizedCapture(cap, **kw): wraps any object with isOpened / read / get / release (cv2.VideoCapture, synth.FakeCapture) and
    delivers its frames stabilised against the first one read: read() returns (True, frame) with the frame as the capture delivers it
    -- [H,W,3] uint8 BGR, or 2-D uint16 --, resampled by its estimated shift.  RespiratoryMonitor(capture_target=StabilizedCapture(...))
    therefore works unchanged.  **kw: Stabilizer's max_shift, levels, iterations.  last_shift / last_flags: those of the last frame."""

    def __init__(self, cap, **kw):
        self.cap, self.kw = cap, kw
        self.stabilizer = None
        self.last_shift, self.last_flags = None, None

    def isOpened(self):
        return self.cap.isOpened()

    def get(self, prop):
        return self.cap.get(prop)

    def release(self):
        if self.stabilizer is not None:
            self.stabilizer.close()
            self.stabilizer = None
        return self.cap.release()

    def reset(self):
        """The next frame read becomes the reference."""
        if self.stabilizer is not None:
            self.stabilizer.reset()

    def read(self):
        ret, frame = self.cap.read()
        if not ret:
            return ret, frame
        f = np.asarray(frame)
        if self.stabilizer is None or (self.stabilizer.H, self.stabilizer.W) != f.shape[:2]:
            if self.stabilizer is not None:
                self.stabilizer.close()
            self.stabilizer = Stabilizer(f.shape[0], f.shape[1], **self.kw)
        out, shifts, flags = self.stabilizer.push(np.ascontiguousarray(f))
        self.last_shift, self.last_flags = (float(shifts[0, 0]), float(shifts[0, 1])), int(flags[0])
        return True, out
