"""A shaky camera taken out of the frames before anything else looks at them (rm_stab_* and rm_warp_shift of include/respmon_hip.h,
where the rule is written out operation by operation).

Every method of this package assumes a camera that stands still.  A webcam on a monitor arm, a phone leaned on a shelf moves by a
pixel or two from frame to frame; that motion is broadband, part of it falls into the breathing band, and locate() then finds
background texture.  Stabilizer estimates, per frame, the global shift against a FIXED reference frame (translation-only
Gauss-Newton, coarse to fine on the library's Gaussian pyramid) and resamples the frame by it (bilinear, replicated border).  The
reference is the first frame after construction or reset(), or the frame given to set_reference(); it never drifts, so a frame's
result depends on neither the other frames of a push nor on how a stream is cut into pushes.

A camera in a hand or on a flexible arm also rolls and zooms: one degree of roll moves the corners of a 1080p frame by 19 px.
Stabilizer(model='similarity') estimates rotation, zoom and shift together (rm_stab_sim_*, rm_warp_similarity): four parameters
p = (p0, p1, tx, ty) with p0 = s cos(theta) - 1, p1 = s sin(theta), by Gauss-Newton on the same pyramid; the levels above
`linear_level` estimate the shift alone, as the shift model does.  crop=True (stabilize_video, StabilizedCapture) cuts the frames to
valid_rect(), the part no replicated border can reach.

Not covered: shear, perspective, rolling shutter, a camera that pans on purpose (the reference would have to follow)."""
import ctypes
import math

import numpy as np

from . import _capi, device

FLAG_LEVEL_SKIPPED = 1   # a level had no usable gradient (a flat reference) or no region (a tiny frame): it did not contribute
FLAG_CLAMPED = 2         # the last update ran into max_shift: the frame has probably moved further than that
FLAG_LINEAR_CLAMPED = 4  # model 'similarity': the last update ran into max_linear: the frame has probably rolled or zoomed further
MODELS = ("shift", "similarity")


def valid_rect(H, W, max_shift, max_linear=0.0):
    """(x, y, w, h): the central rectangle of an H x W frame that no replicated border can reach while the parameters stay inside
    their clamps.  A pixel moves by at most max_shift + max_linear * (|u| + |v|) <= max_shift + max_linear * (cx + cy), so the margin is
    the ceiling of that on every side (max_linear 0: the shift model)."""
    m = int(math.ceil(float(max_shift) + float(max_linear) * ((W - 1) * 0.5 + (H - 1) * 0.5)))
    if W - 2 * m < 1 or H - 2 * m < 1:
        raise ValueError("a %dx%d frame has no pixel %d from every edge (max_shift %g, max_linear %g)" % (H, W, m, max_shift, max_linear))
    return m, m, W - 2 * m, H - 2 * m


def rotation_deg(params):
    """the roll angle in degrees of similarity parameters [N,4] (or [4])"""
    p = np.asarray(params, dtype=np.float64)
    return np.degrees(np.arctan2(p[..., 1], 1.0 + p[..., 0]))


def zoom(params):
    """the scale factor of similarity parameters [N,4] (or [4])"""
    p = np.asarray(params, dtype=np.float64)
    return np.hypot(1.0 + p[..., 0], p[..., 1])


class Stabilizer:
    """Stabilizer(H, W, max_shift=8.0, levels=(3, 0), iterations=2): levels = (coarse, fine) pyramid levels of the estimate,
    `iterations` Gauss-Newton steps per level (a fixed count: nothing terminates on data), max_shift in pixels (at most 64).  Two
    iterations recover about one pixel of the coarsest level per level, so the coarse level should satisfy 2^coarse >= max_shift.

    push(frames, out_dtype=None) -> (frames, shifts [N,2], flags [N]); estimate(frames) -> (shifts, flags); warp(frames, shifts);
    set_reference(frame); reset().  Frames are [N,H,W] or [H,W] of uint8 / uint16 / float16 / float32 / float64, or [N,H,W,3] / [H,W,3]
    uint8 BGR (estimated on its gray value, warped channel by channel); numpy in -> numpy out, device tensor in -> device tensor out.
    out_dtype 'uint8' | 'uint16' | 'float32' | 'float64' (None: uint8 for uint8 input, uint16 for uint16 input, float64 otherwise);
    BGR frames come back as BGR uint8.  shifts[n] = (dx, dy): the displacement of frame n's content against the reference, positive
    toward +x / +y; flags: FLAG_LEVEL_SKIPPED, FLAG_CLAMPED.

    model='similarity', max_linear=0.03, linear_level=1: rotation, zoom and shift.  push and estimate return params [N,4] (p0, p1,
    tx, ty) where the shift model returns shifts [N,2], and warp takes [N,4]; rotation_deg(params) and zoom(params) read them.
    max_linear (at most 0.25) clamps |p0| and |p1|: 0.03 is 1.7 degrees or 3 %; the levels above `linear_level` (-1 .. coarse)
    estimate the shift alone -- four parameters are not determined on the few pixels of a very coarse level; FLAG_LINEAR_CLAMPED."""

    def __init__(self, H, W, max_shift=8.0, levels=(3, 0), iterations=2, device_index=None, model="shift", max_linear=0.03, linear_level=1):
        if model not in MODELS:
            raise ValueError("model must be 'shift' or 'similarity', got %r" % (model,))
        t = device.require_gpu()
        self.lib = _capi.load()
        self.H, self.W = int(H), int(W)
        self.model, self.max_shift, self.max_linear = model, float(max_shift), float(max_linear) if model == "similarity" else 0.0
        self._np = 4 if model == "similarity" else 2                                       # parameters per frame
        self._pre = "rm_stab_sim_" if model == "similarity" else "rm_stab_"
        self.device_index = t.cuda.current_device() if device_index is None else int(device_index)
        self._h = ctypes.c_void_p()
        if model == "similarity":
            _capi.check(self.lib, self.lib.rm_stab_sim_create(self._ctx(), self.H, self.W, int(levels[0]), int(levels[1]), int(linear_level), int(iterations),
                                                              float(max_shift), float(max_linear), ctypes.byref(self._h)), "rm_stab_sim_create")
        else:
            _capi.check(self.lib, self.lib.rm_stab_create(self._ctx(), self.H, self.W, int(levels[0]), int(levels[1]), int(iterations), float(max_shift),
                                                          ctypes.byref(self._h)), "rm_stab_create")

    def _fn(self, name):
        return getattr(self.lib, self._pre + name)

    @property
    def valid_rect(self):
        """valid_rect(H, W, max_shift, max_linear) of this stabiliser"""
        return valid_rect(self.H, self.W, self.max_shift, self.max_linear)

    def _ctx(self):
        return device._CTX.get(self.device_index) or device.ctx(self.device_index)

    def _stream(self):
        return ctypes.c_void_p(device.raw_stream(self.device_index))

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
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
        _capi.check(self.lib, self._fn("info")(self._h, ctypes.byref(seen), ctypes.byref(ref), ctypes.byref(b)), self._pre + "info")
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
        _capi.check(self.lib, self._fn("reset")(self._ctx(), self._h), self._pre + "reset")

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
        _capi.check(self.lib, self._fn("set_reference")(self._ctx(), self._h, device.ptr(x), device.buffer_dtype_code(x), self._stream()),
                    self._pre + "set_reference")

    def _push(self, frames, out_dtype, want_frames):
        x, single = self._frames(frames)
        n = int(x.shape[0])
        out, out_code = self._out(x, out_dtype) if want_frames else (None, _capi.RM_U8)
        shifts, flags = np.zeros((n, self._np)), np.zeros(n, np.int32)
        if n:
            _capi.check(self.lib, self._fn("push")(self._ctx(), self._h, device.ptr(x), device.buffer_dtype_code(x), n, device.ptr(out), out_code,
                                                   ctypes.c_void_p(shifts.ctypes.data), ctypes.c_void_p(flags.ctypes.data), self._stream()), self._pre + "push")
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
        """frames resampled by the caller's shifts [N,2] (rm_warp_shift): out[n][y][x] = bilinear(frames[n], x + dx, y + dy); with
        model 'similarity' by the caller's parameters [N,4] (rm_warp_similarity)"""
        x, single = self._frames(frames)
        n = int(x.shape[0])
        s = np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1, self._np)
        if len(s) != n:
            raise ValueError("%d parameter sets for %d frames" % (len(s), n))
        out, out_code = self._out(x, out_dtype)
        if n:
            name = "rm_warp_similarity" if self.model == "similarity" else "rm_warp_shift"
            _capi.check(self.lib, getattr(self.lib, name)(self._ctx(), device.ptr(x), device.buffer_dtype_code(x), n, self.H, self.W,
                                                          ctypes.c_void_p(s.ctypes.data), device.ptr(out), out_code, self._stream()), name)
            return device.like_input(out[0] if single else out, frames)


def stabilize_video(vid, out_dtype=None, return_shifts=False, crop=False, **kw):
    """A whole clip registered to its first frame: one Stabilizer(H, W, **kw), one push.  `vid`: [T,H,W] gray or [T,H,W,3] uint8 BGR;
    numpy in -> numpy out, device tensor in -> device tensor out.  return_shifts=True: (frames, shifts [T,2], flags [T]) -- with
    model='similarity' params [T,4].  crop=True: the frames cut to valid_rect()."""
    x = device.to_device(vid)
    T, H, W = device.buffer_shape(x)
    with Stabilizer(H, W, device_index=x.device.index, **kw) as st:
        out, shifts, flags = st.push(x, out_dtype)
        if crop:
            cx, cy, cw, ch = st.valid_rect
            out = out[:, cy:cy + ch, cx:cx + cw].contiguous()
    out = device.like_input(out, vid)
    return (out, shifts, flags) if return_shifts else out


_CAP_PROP_FRAME_WIDTH, _CAP_PROP_FRAME_HEIGHT = 3, 4   # cv2's (and synth.FakeCapture's)


class StabilizedCapture:
    """StabilizedCapture(cap, **kw): wraps any object with isOpened / read / get / release (cv2.VideoCapture, synth.FakeCapture) and
    delivers its frames stabilised against the first one read: read() returns (True, frame) with the frame as the capture delivers it
    -- [H,W,3] uint8 BGR, or 2-D uint16 --, resampled by its estimated shift.  RespiratoryMonitor(capture_target=StabilizedCapture(...))
    therefore works unchanged.  **kw: Stabilizer's max_shift, levels, iterations, model, max_linear, linear_level.  crop=True: the
    frames cut to valid_rect(), and get() reports the cut width and height.  last_shift (tx, ty), last_transform (p0, p1, tx, ty) and
    last_flags: those of the last frame."""

    def __init__(self, cap, crop=False, **kw):
        self.cap, self.kw, self.crop = cap, kw, bool(crop)
        self.stabilizer = None
        self.last_shift, self.last_transform, self.last_flags = None, None, None

    def isOpened(self):
        return self.cap.isOpened()

    def get(self, prop):
        v = self.cap.get(prop)
        if self.crop and prop in (_CAP_PROP_FRAME_WIDTH, _CAP_PROP_FRAME_HEIGHT) and v > 0:
            H, W = int(self.cap.get(_CAP_PROP_FRAME_HEIGHT)), int(self.cap.get(_CAP_PROP_FRAME_WIDTH))
            rect = valid_rect(H, W, self.kw.get("max_shift", 8.0), self.kw.get("max_linear", 0.03) if self.kw.get("model", "shift") == "similarity" else 0.0)
            return float(rect[2] if prop == _CAP_PROP_FRAME_WIDTH else rect[3])
        return v

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
        p = [float(v) for v in shifts[0]]
        self.last_transform = tuple(p) if len(p) == 4 else (0.0, 0.0, p[0], p[1])
        self.last_shift, self.last_flags = self.last_transform[2:], int(flags[0])
        if self.crop:
            x, y, w, h = self.stabilizer.valid_rect
            out = np.ascontiguousarray(out[y:y + h, x:x + w])
        return True, out
