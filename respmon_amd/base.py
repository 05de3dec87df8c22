"""
RespiratoryMonitor -- drop-in for the reference's base.py surface on the hot path
(run / locate / calibrate / measure / extract_motion / skip_calibration), backed by the
gfx950 HIP library.  Reference lines are cited per method (paths relative to the reference).

Differences from the reference that are deliberate and documented in DESIGN.md:
  * no pyqtgraph UI (`visualize` must be None or 'pyqtgraph'; the latter is accepted and ignored),
    no cv2.VideoWriter / np.save side outputs (out of scope: capture / codec I/O);
  * `capture_target` may be any object with the cv2.VideoCapture duck type
    (isOpened / read / get / release); a path or camera index needs cv2 at run time;
  * the calibration buffer lives in HBM (`calibration_buffer` is a CUDA tensor);
  * `run_on_init=True` keeps the reference's "constructor blocks in run()" behaviour
    (base.py:164); pass False to drive the object step by step;
  * `reset()` also forgets the flow state (`previous_cropped_image`, `motion_key_points`).  This DIFFERS from the reference:
    its reset() (base.py:515-533) never sets `previous_cropped_image` back to None, so after a reset and a new calibration it
    keeps tracking from the stale crop and the stale points (base.py:371) -- and `calcOpticalFlowPyrLK` fails outright if the
    new ROI has another size.  Here the first frame after a recalibration initialises the corners again (a bug fix, listed
    under "deliberate behavioural differences" in DESIGN.md);
  * after a calibration that finds no ROI the retry goes through `update_ui()` / `sync_to_fps()` like every other
    iteration; the reference `continue`s past them (base.py:451-454) -- no effect on the data path (the UI is a no-op here);
  * the default operation order of the calibration commutes two linear stages (`reference_operation_order`).
"""
import logging
import time
from collections import deque

import numpy as np

from . import _capi, device, rate
from .tools import Benchmarker, reduce_bounding_box
from .measure import BreathSignal

THRESH_BINARY = 0  # cv2.THRESH_BINARY


class FlowState:
    """Owner of one rm_flow_state (the device-resident tracking session of extract_motion('flow')); released with the object."""

    def __init__(self, lib):
        import ctypes
        self._lib = lib
        self.handle = ctypes.c_void_p()
        _capi.check(lib, lib.rm_flow_state_create(device.ctx(), ctypes.byref(self.handle)), "rm_flow_state_create")

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self._lib.rm_flow_state_destroy(self.handle)
            self.handle.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


class PhaseMotionState:
    """Owner of one rm_phase_motion (the session of extract_motion('phase'): the previous frame's pyramid level of one rectangle size);
    released with the object."""

    def __init__(self, lib, w, h, level):
        import ctypes
        self._lib = lib
        self.w, self.h, self.level = int(w), int(h), int(level)
        self.handle = ctypes.c_void_p()
        _capi.check(lib, lib.rm_phase_motion_create(device.ctx(), self.w, self.h, self.level, ctypes.byref(self.handle)), "rm_phase_motion_create")

    def reset(self):
        """The next frame begins a new sequence: it returns zeros and becomes the state."""
        _capi.check(self._lib, self._lib.rm_phase_motion_reset(device.ctx(), self.handle), "rm_phase_motion_reset")

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self._lib.rm_phase_motion_destroy(self.handle)
            self.handle.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


class _Backend:
    """The only door from the state machine to compute: every method is one C-ABI call.
    Tests of the host logic replace it with a recording double; there is no CPU implementation."""

    def __init__(self):
        import ctypes
        self.lib = _capi.load()
        self.t = device.require_gpu()
        self._xywh = (ctypes.c_int32 * 4)()

    # -- calibration ------------------------------------------------------------------
    def locate(self, buf, fps, freq_min, freq_max, amplification, pyramid_levels, skip_levels_at_top,
               temporal_threshold, threshold, flags=0):
        import ctypes
        T, H, W = device.buffer_shape(buf)
        xywh = self._xywh
        # (this call sits on the host path between two calibrations: the context of the buffer's device is looked up without asking
        #  the runtime, the stream is the current one of that device)
        idx = buf.device.index
        ctx = device._CTX.get(idx) or device.ctx(idx)
        stream = ctypes.c_void_p(device.raw_stream(idx))
        rc = self.lib.rm_locate(ctx, ctypes.c_void_p(buf.data_ptr()), device.buffer_dtype_code(buf), T, H, W,
                                float(fps), float(freq_min), float(freq_max), float(amplification),
                                int(pyramid_levels), int(skip_levels_at_top), float(temporal_threshold),
                                int(threshold), int(flags), xywh, stream)
        if rc < 0:
            _capi.check(self.lib, rc, "rm_locate")
        if rc == _capi.RM_NO_CONTOUR:
            return None
        return xywh[0], xywh[1], xywh[2], xywh[3]

    def locate_submit(self, buf, fps, freq_min=0.1, freq_max=1.0, amplification=500, pyramid_levels=9, skip_levels_at_top=4,
                      temporal_threshold=0.7, threshold=20, flags=0):
        """locate() without the wait: the device work is enqueued and a ticket returned (rm_locate_submit).  Up to
        _capi.RM_LOCATE_TICKETS buffers per GPU may be in flight; `buf` must stay alive and unchanged until locate_result."""
        import ctypes
        T, H, W = device.buffer_shape(buf)
        idx = buf.device.index
        ctx = device._CTX.get(idx) or device.ctx(idx)
        stream = ctypes.c_void_p(device.raw_stream(idx))
        ticket = ctypes.c_int(-1)
        rc = self.lib.rm_locate_submit(ctx, ctypes.c_void_p(buf.data_ptr()), device.buffer_dtype_code(buf), T, H, W,
                                       float(fps), float(freq_min), float(freq_max), float(amplification),
                                       int(pyramid_levels), int(skip_levels_at_top), float(temporal_threshold),
                                       int(threshold), int(flags), stream, ctypes.byref(ticket))
        if rc < 0:
            _capi.check(self.lib, rc, "rm_locate_submit")
        return (idx, ticket.value, buf)     # (the buffer rides along: it must outlive the submission)

    def locate_result(self, ticket):
        """The ROI of a locate_submit: (x, y, w, h) or None, bit-identical to locate() on the same buffer (rm_locate_result)."""
        idx, tk, _buf = ticket
        ctx = device._CTX.get(idx) or device.ctx(idx)
        xywh = self._xywh
        rc = self.lib.rm_locate_result(ctx, tk, xywh)
        if rc < 0:
            _capi.check(self.lib, rc, "rm_locate_result")
        if rc == _capi.RM_NO_CONTOUR:
            return None
        return xywh[0], xywh[1], xywh[2], xywh[3]

    def locate_multi(self, buf, fps, freq_min=0.1, freq_max=1.0, amplification=500, pyramid_levels=9, skip_levels_at_top=4,
                     temporal_threshold=0.7, threshold=20, flags=0, max_rois=4, min_area=0.0, with_areas=False):
        """The `max_rois` largest contours of locate()'s thresholded heat map as a list of (x, y, w, h), largest first (rm_locate_multi);
        [] where locate() returns None.  with_areas: (rois, areas)."""
        import ctypes
        T, H, W = device.buffer_shape(buf)
        idx = buf.device.index
        ctx = device._CTX.get(idx) or device.ctx(idx)
        stream = ctypes.c_void_p(device.raw_stream(idx))
        cap = max(int(max_rois), 1)
        xywh = np.zeros((cap, 4), dtype=np.int32)
        area = np.zeros(cap, dtype=np.float64)
        n = ctypes.c_int(0)
        rc = self.lib.rm_locate_multi(ctx, ctypes.c_void_p(buf.data_ptr()), device.buffer_dtype_code(buf), T, H, W,
                                      float(fps), float(freq_min), float(freq_max), float(amplification),
                                      int(pyramid_levels), int(skip_levels_at_top), float(temporal_threshold),
                                      int(threshold), int(flags), int(max_rois), float(min_area),
                                      ctypes.c_void_p(xywh.ctypes.data), ctypes.c_void_p(area.ctypes.data), ctypes.byref(n), stream)
        if rc < 0:
            _capi.check(self.lib, rc, "rm_locate_multi")
        rois = [tuple(int(v) for v in xywh[i]) for i in range(n.value)]
        return (rois, [float(a) for a in area[:n.value]]) if with_areas else rois

    # -- ingest -----------------------------------------------------------------------
    def bgr_to_gray(self, bgr_u8_host):
        t = self.t
        src = t.from_numpy(np.ascontiguousarray(bgr_u8_host)).cuda()
        H, W = src.shape[0], src.shape[1]
        gray = t.empty((H, W), dtype=t.uint8, device=src.device)
        _capi.check(self.lib, self.lib.rm_bgr_to_gray(device.ctx(), device.ptr(src), H * W, device.ptr(gray),
                                                      device.stream_ptr()), "rm_bgr_to_gray")
        self.last_bgr = src     # the frame as captured, on the device: what a 'bgr8' calibration buffer stores (store_frame's `bgr`)
        return gray

    def gray16(self, y16_host):
        """a 2-D uint16 frame of the capture (Y16) as it is, on the device: no cvtColor, no narrowing"""
        return self.t.from_numpy(np.ascontiguousarray(y16_host)).cuda()

    def store_frame(self, buf, idx, gray_u8, bgr=None):
        """calibration_buffer[idx][:] = uint8_to_float(gray) (base.py:231, 431).
        A uint16 frame (Y16) goes into a 'uint16' buffer as it is, or through rm_uint16_to_float (k * (1./65535)) into a float buffer:
        float64 exact, a narrower one rounded once.  An 8-bit buffer has no place for it, and a 'uint16' buffer none for an 8-bit frame
        (the two scales differ: include/respmon_hip.h RM_U16): TypeError.
        A 'bgr8' buffer ([T,H,W,3] uint8) stores the frame AS CAPTURED: pass the device BGR tensor the gray frame came from as
        `bgr` (RespiratoryMonitor.step does: the tensor next_frame() kept).  Without it -- a gray frame from another source:
        replayed, processed, another backend's ingest -- the gray value goes into all three planes, which base.py:230's
        conversion maps back to exactly that gray value (Y(x, x, x) == x), so the calibration reads the same frame either way."""
        t = self.t
        frame16, buf16 = gray_u8.dtype == t.uint16, buf.dtype == t.uint16
        if (frame16 and buf.dtype == t.uint8) or (buf16 and not frame16):
            raise TypeError("a %s frame does not go into a %s calibration buffer (uint16 frames: buffer_dtype 'uint16' or a float dtype; "
                            "uint8 / BGR frames: any other buffer_dtype)"
                            % (str(gray_u8.dtype).replace("torch.", ""), "bgr8" if buf.dim() == 4 else str(buf.dtype).replace("torch.", "")))
        if buf.dim() == 4:
            # buffer_dtype 'bgr8': rm_locate applies base.py:230-231 when it reads the buffer (RM_BGR8)
            if bgr is not None:
                buf[idx].copy_(bgr)
            else:
                buf[idx].copy_(gray_u8.unsqueeze(-1).expand(-1, -1, 3))
        elif buf.dtype == t.uint8 or buf16:
            buf[idx].copy_(gray_u8)
        else:
            dst64 = buf[idx] if buf.dtype == t.float64 else t.empty(gray_u8.shape, dtype=t.float64, device=gray_u8.device)
            fn = "rm_uint16_to_float" if frame16 else "rm_uint8_to_float"
            _capi.check(self.lib, getattr(self.lib, fn)(device.ctx(), device.ptr(gray_u8), device.ptr(dst64),
                                                        gray_u8.numel(), device.stream_ptr()), fn)
            if buf.dtype != t.float64:   # narrower float buffer: round the float64 value to the storage dtype
                buf[idx].copy_(dst64)

    # -- measurement ------------------------------------------------------------------
    def roi_mean(self, gray_u8, x, y, w, h):
        import ctypes
        H, W = gray_u8.shape
        out = ctypes.c_double()
        _capi.check(self.lib, self.lib.rm_roi_mean(device.ctx(), device.ptr(gray_u8), device.dtype_code(gray_u8), H, W,
                                                   x, y, w, h, ctypes.byref(out), device.stream_ptr()), "rm_roi_mean")
        return out.value

    def roi_to_uint8(self, gray_u8, x, y, w, h):
        t = self.t
        H, W = gray_u8.shape
        dst = t.empty((h, w), dtype=t.uint8, device=gray_u8.device)
        _capi.check(self.lib, self.lib.rm_roi_to_uint8(device.ctx(), device.ptr(gray_u8), device.dtype_code(gray_u8), H, W,
                                                       x, y, w, h, device.ptr(dst), device.stream_ptr()), "rm_roi_to_uint8")
        return dst

    def good_features_to_track(self, img_u8, maxCorners, qualityLevel, minDistance, blockSize):
        import ctypes
        h, w = img_u8.shape
        cap = int(maxCorners) if maxCorners > 0 else h * w        # (maxCorners <= 0: no limit)
        pts = np.empty((cap, 2), dtype=np.float32)
        n = ctypes.c_int()
        _capi.check(self.lib, self.lib.rm_good_features_to_track(device.ctx(), device.ptr(img_u8), h, w, int(maxCorners),
                                                                 float(qualityLevel), float(minDistance), int(blockSize),
                                                                 ctypes.c_void_p(pts.ctypes.data), ctypes.byref(n),
                                                                 device.stream_ptr()), "rm_good_features_to_track")
        if n.value == 0:
            return None
        return pts[:n.value].reshape(-1, 1, 2).copy()

    def calc_optical_flow_pyr_lk(self, prev_u8, next_u8, pts, winSize, maxLevel, criteria):
        import ctypes
        h, w = prev_u8.shape
        p0 = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        n = len(p0)
        p1 = np.empty((n, 2), dtype=np.float32)
        st = np.empty(n, dtype=np.uint8)
        ctype, max_count, eps = criteria
        if not (ctype & 1):
            max_count = 30
        if not (ctype & 2):
            eps = 0.01
        _capi.check(self.lib, self.lib.rm_calc_optical_flow_pyr_lk(device.ctx(), device.ptr(prev_u8), device.ptr(next_u8), h, w,
                                                                   ctypes.c_void_p(p0.ctypes.data), n, int(winSize[0]),
                                                                   int(winSize[1]), int(maxLevel), int(max_count), float(eps),
                                                                   ctypes.c_void_p(p1.ctypes.data), ctypes.c_void_p(st.ctypes.data),
                                                                   device.stream_ptr()), "rm_calc_optical_flow_pyr_lk")
        return p1.reshape(-1, 1, 2), st.reshape(-1, 1)

    def mean_flow(self, old_pts, new_pts, status):
        import ctypes
        o = np.ascontiguousarray(old_pts, dtype=np.float32).reshape(-1, 2)
        nw = np.ascontiguousarray(new_pts, dtype=np.float32).reshape(-1, 2)
        st = np.ascontiguousarray(status, dtype=np.uint8).reshape(-1)
        mean = np.empty(2, dtype=np.float32)
        ng = ctypes.c_int()
        _capi.check(self.lib, self.lib.rm_mean_flow(device.ctx(), ctypes.c_void_p(o.ctypes.data), ctypes.c_void_p(nw.ctypes.data),
                                                    ctypes.c_void_p(st.ctypes.data), len(o), ctypes.c_void_p(mean.ctypes.data),
                                                    ctypes.byref(ng), device.stream_ptr()), "rm_mean_flow")
        return mean, ng.value

    # -- extract_motion('flow') with the crops and points resident on the device: one C-ABI call per frame --------------------
    # -- resident flow session (include/respmon_hip.h rm_flow_state): one handle per monitor -----------------------------
    def flow_state(self):
        """A new rm_flow_state on the current device: previous crop, its LK pyramid, the tracked points of ONE tracking session."""
        return FlowState(self.lib)

    def flow_begin(self, state, gray_u8, x, y, w, h, maxCorners, qualityLevel, minDistance, blockSize):
        import ctypes
        H, W = gray_u8.shape
        pts = np.empty((int(maxCorners) if maxCorners > 0 else w * h, 2), dtype=np.float32)        # (maxCorners <= 0: no limit)
        n = ctypes.c_int()
        _capi.check(self.lib, self.lib.rm_flow_begin(device.ctx(), state.handle, device.ptr(gray_u8), device.dtype_code(gray_u8), H, W, x, y, w, h,
                                                     int(maxCorners), float(qualityLevel), float(minDistance), int(blockSize),
                                                     ctypes.c_void_p(pts.ctypes.data), ctypes.byref(n), device.stream_ptr()),
                    "rm_flow_begin")
        return None if n.value == 0 else pts[:n.value].reshape(-1, 1, 2).copy()

    def flow_step(self, state, gray_u8, x, y, w, h, winSize, maxLevel, criteria):
        import ctypes
        H, W = gray_u8.shape
        ctype, max_count, eps = criteria
        if not (ctype & 1):
            max_count = 30
        if not (ctype & 2):
            eps = 0.01
        mean = np.empty(2, dtype=np.float32)
        ng = ctypes.c_int()
        _capi.check(self.lib, self.lib.rm_flow_step(device.ctx(), state.handle, device.ptr(gray_u8), device.dtype_code(gray_u8), H, W, x, y, w, h,
                                                    int(winSize[0]), int(winSize[1]), int(maxLevel), int(max_count), float(eps),
                                                    ctypes.c_void_p(mean.ctypes.data), ctypes.byref(ng), device.stream_ptr()),
                    "rm_flow_step")
        return mean, ng.value

    def flow_points(self, state, cap):
        import ctypes
        pts = np.empty((max(int(cap), 1), 2), dtype=np.float32)
        n = ctypes.c_int()
        _capi.check(self.lib, self.lib.rm_flow_points(device.ctx(), state.handle, ctypes.c_void_p(pts.ctypes.data), len(pts), ctypes.byref(n),
                                                      device.stream_ptr()), "rm_flow_points")
        return pts[:min(n.value, len(pts))].reshape(-1, 1, 2).copy()

    def pca_reduce(self, motion_data):
        import ctypes
        m = np.ascontiguousarray(motion_data, dtype=np.float32).reshape(-1, 2)
        out = ctypes.c_double()
        _capi.check(self.lib, self.lib.rm_pca_reduce(device.ctx(), ctypes.c_void_p(m.ctypes.data), len(m), ctypes.byref(out),
                                                     device.stream_ptr()), "rm_pca_reduce")
        return out.value

    # -- a whole resident [N,H,W] clip per call: one host synchronisation each (include/respmon_hip.h) ------------------------
    def roi_mean_clip(self, frames, x, y, w, h):
        import ctypes
        frames = frames.contiguous()
        N, H, W = frames.shape
        out = np.empty(N, dtype=np.float64)
        _capi.check(self.lib, self.lib.rm_roi_mean_clip(device.ctx(), device.ptr(frames), device.dtype_code(frames), N, H, W, x, y, w, h,
                                                        ctypes.c_void_p(out.ctypes.data), device.stream_ptr()), "rm_roi_mean_clip")
        return out

    def roi_mean_multi_clip(self, frames, rois):
        """ndarray [N, K]: the ROI mean of every frame of the resident clip and every rectangle (x, y, w, h) of `rois`, one call."""
        import ctypes
        frames = frames.contiguous()
        N, H, W = frames.shape
        r = np.ascontiguousarray(rois, dtype=np.int32).reshape(-1, 4)
        out = np.empty((N, len(r)), dtype=np.float64)
        _capi.check(self.lib, self.lib.rm_roi_mean_multi_clip(device.ctx(), device.ptr(frames), device.dtype_code(frames), N, H, W,
                                                              ctypes.c_void_p(r.ctypes.data), len(r), ctypes.c_void_p(out.ctypes.data),
                                                              device.stream_ptr()), "rm_roi_mean_multi_clip")
        return out

    def flow_clip(self, state, frames, x, y, w, h, winSize, maxLevel, criteria):
        import ctypes
        frames = frames.contiguous()
        N, H, W = frames.shape
        ctype, max_count, eps = criteria
        if not (ctype & 1):
            max_count = 30
        if not (ctype & 2):
            eps = 0.01
        mean = np.empty((N, 2), dtype=np.float32)
        ng = np.empty(N, dtype=np.int32)
        _capi.check(self.lib, self.lib.rm_flow_clip(device.ctx(), state.handle, device.ptr(frames), device.dtype_code(frames), N, H, W, x, y, w, h,
                                                    int(winSize[0]), int(winSize[1]), int(maxLevel), int(max_count), float(eps),
                                                    ctypes.c_void_p(mean.ctypes.data), ctypes.c_void_p(ng.ctypes.data), device.stream_ptr()),
                    "rm_flow_clip")
        return mean, ng

    def pca_reduce_windows(self, motion_data, first, window):
        import ctypes
        m = np.ascontiguousarray(motion_data, dtype=np.float32).reshape(-1, 2)
        out = np.empty(len(m) - int(first), dtype=np.float64)
        _capi.check(self.lib, self.lib.rm_pca_reduce_windows(device.ctx(), ctypes.c_void_p(m.ctypes.data), len(m), int(first), int(window),
                                                             ctypes.c_void_p(out.ctypes.data), device.stream_ptr()), "rm_pca_reduce_windows")
        return out

    # -- several subjects per clip: K flow_clip calls, K pca_reduce_windows calls as one call each ------------------------------
    def flow_multi_clip(self, states, frames, rois, winSize, maxLevel, criteria):
        """(mean [N,K,2] float32, n_good [N,K] int32): flow_clip of subject k on states[k] with rectangle rois[k], in one call."""
        import ctypes
        frames = frames.contiguous()
        N, H, W = frames.shape
        r = np.ascontiguousarray(rois, dtype=np.int32).reshape(-1, 4)
        K = len(r)
        assert len(states) == K, "one flow state per rectangle"
        handles = (ctypes.c_void_p * K)(*[st.handle for st in states])
        ctype, max_count, eps = criteria
        if not (ctype & 1):
            max_count = 30
        if not (ctype & 2):
            eps = 0.01
        mean = np.empty((N, K, 2), dtype=np.float32)
        ng = np.empty((N, K), dtype=np.int32)
        _capi.check(self.lib, self.lib.rm_flow_multi_clip(device.ctx(), handles, device.ptr(frames), device.dtype_code(frames), N, H, W,
                                                          ctypes.c_void_p(r.ctypes.data), K, int(winSize[0]), int(winSize[1]), int(maxLevel),
                                                          int(max_count), float(eps), ctypes.c_void_p(mean.ctypes.data),
                                                          ctypes.c_void_p(ng.ctypes.data), device.stream_ptr()), "rm_flow_multi_clip")
        return mean, ng

    # -- extract_motion('phase'): the phase sums of a rectangle, per frame (a clip of one) or per clip, for one or several subjects ------
    def phase_motion_state(self, w, h, level):
        """A new rm_phase_motion on the current device for w x h rectangles at pyramid level `level`."""
        return PhaseMotionState(self.lib, w, h, level)

    def phase_motion_clip(self, state, frames, x, y):
        """ndarray [N, 3]: Sw, Sc, Ss of every frame of the resident [N,H,W] clip for the state's rectangle at (x, y), one call."""
        import ctypes
        frames = frames.contiguous()
        N, H, W = frames.shape
        out = np.empty((N, 3), dtype=np.float64)
        _capi.check(self.lib, self.lib.rm_phase_motion_clip(device.ctx(), state.handle, device.ptr(frames), device.dtype_code(frames), N, H, W,
                                                            int(x), int(y), ctypes.c_void_p(out.ctypes.data), device.stream_ptr()),
                    "rm_phase_motion_clip")
        return out

    def phase_motion_multi_clip(self, states, frames, rois):
        """ndarray [N, K, 3]: phase_motion_clip of subject k on states[k] with rectangle rois[k], in one call."""
        import ctypes
        frames = frames.contiguous()
        N, H, W = frames.shape
        r = np.ascontiguousarray(rois, dtype=np.int32).reshape(-1, 4)
        K = len(r)
        assert len(states) == K, "one phase state per rectangle"
        handles = (ctypes.c_void_p * K)(*[st.handle for st in states])
        out = np.empty((N, K, 3), dtype=np.float64)
        _capi.check(self.lib, self.lib.rm_phase_motion_multi_clip(device.ctx(), handles, device.ptr(frames), device.dtype_code(frames), N, H, W,
                                                                  ctypes.c_void_p(r.ctypes.data), K, ctypes.c_void_p(out.ctypes.data),
                                                                  device.stream_ptr()), "rm_phase_motion_multi_clip")
        return out

    def pca_reduce_windows_multi(self, rows_list, firsts, window):
        """[pca_reduce_windows(rows_list[k], firsts[k], window) for every k], in one call."""
        import ctypes
        rows = [np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 2) for m in rows_list]
        seg = np.empty((len(rows), 3), dtype=np.int32)
        at = 0
        for k, m in enumerate(rows):
            seg[k] = (at, len(m), int(firsts[k]))
            at += len(m)
        allrows = np.concatenate(rows) if rows else np.empty((0, 2), np.float32)
        counts = [int(n - f) for _, n, f in seg]
        out = np.empty(max(sum(counts), 1), dtype=np.float64)
        _capi.check(self.lib, self.lib.rm_pca_reduce_windows_multi(device.ctx(), ctypes.c_void_p(allrows.ctypes.data), ctypes.c_void_p(seg.ctypes.data),
                                                                   len(rows), int(window), ctypes.c_void_p(out.ctypes.data), device.stream_ptr()),
                    "rm_pca_reduce_windows_multi")
        return [a.copy() for a in np.split(out[:sum(counts)], np.cumsum(counts)[:-1])]


class RespiratoryMonitor(BreathSignal):
    CAP_PROP_FRAME_WIDTH, CAP_PROP_FRAME_HEIGHT, CAP_PROP_FPS = 3, 4, 5
    TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS = 1, 2

    def __init__(self, capture_target=0, save_calibration_image=False, visualize='pyqtgraph', fig_size=None,
                 fps_limit=10, error_reset_delay=10.0, save_all_data=True,
                 motion_extraction_method='average', buffer_dtype='float64', run_on_init=True, backend=None, relocate_every=0,
                 phase_params=None):
        """Arguments as reference base.py:24-34, plus (not in the reference):
        buffer_dtype -- element type of the calibration buffer in HBM: 'float64' (the reference's, base.py:119), 'float32',
            'float16', 'uint8' (the gray frame as ingested; uint8_to_float happens where the buffer is read), 'uint16' (the same for
            the 2-D uint16 frames of a Y16 capture -- infrared, thermal, depth: k * (1./65535) where the buffer is read; such frames
            also go into the float dtypes, and neither into nor out of the 8-bit ones: TypeError.  White is 65535: the 'flow' method
            crops trunc(x * 255) of a frame, so right-aligned 10 / 12 / 14-bit samples should be shifted up first; 'average' and the
            calibration do not care) or 'bgr8' (a
            [T,H,W,3] uint8 buffer of the frames AS CAPTURED: cvtColor + uint8_to_float happen where the buffer is read; next_frame()
            keeps the device copy of the captured frame for step(), a frame from anywhere else is stored as its gray value in
            three planes -- the same calibration either way);
        motion_extraction_method -- 'average' and 'flow' are the reference's; 'phase' (not in the reference) measures the
            amplitude-weighted mean phase velocity of one Riesz-pyramid level of the ROI (include/respmon_hip.h rm_phase_motion_*): the
            signal for a region that moves a fraction of a pixel at constant brightness and offers texture, not corners.  A frame
            yields a 2-vector as the flow path's mean flow does, and goes through the same motion_data / PCA bookkeeping;
            phase_params -- dict(level=1): the pyramid level (0 .. 8) of the 'phase' method;
        run_on_init -- False: construct without entering run(); backend -- a stand-in for the device backend (tests);
        relocate_every -- 0 (default): the reference's one-shot calibration buffer, nothing else.  n > 0: every frame that is stored or
            measured also goes into a sliding window on the device (respmon_amd/window.py SlidingCalibration: a ring of per-frame
            pyramid rows, calibration_buffer_target_length frames long); once the first locate() has put the monitor into 'measure',
            the ROI is taken again from the ring every n measured frames (kept when the ring shows no contour), and after a reset()
            the ring is still there: the next ROI comes from it with the next frame instead of after a refill of the buffer.
            step_clip() cuts its clips where the ROI is refreshed, so clips and single frames give the same ROIs.  In 'flow' mode
            a refresh that changes the ROI starts the tracking again on the new rectangle (new corners, motion_data emptied), as
            a reset() does; the value of that frame and of the next is 0.0, as on the first two frames of any tracking session.
            Two things to know: while a full ring shows no contour, every calibration frame tries the ring again (one
            host-synchronous call per frame) until an ROI turns up, alongside the refill of the buffer; and no frame is pushed in
            the 'error' state, so after such a pause the ring holds frames from both sides of a gap of error_reset_delay seconds,
            which the band-pass reads as consecutive until T new frames have replaced them."""
        # argument contract of reference base.py:24-34
        assert isinstance(fps_limit, (int, float)) and fps_limit > 0, "fps_limit must be a positive int or float"
        assert isinstance(save_calibration_image, bool), "save_calibration_image must be bool"
        assert visualize == 'pyqtgraph' or visualize is None, "visualize must be 'pyqtgraph' or None"
        assert fig_size is None or (isinstance(fig_size, (tuple, list)) and len(fig_size) == 2), \
            "fig_size should be None or length 2 tuple or list"
        assert isinstance(error_reset_delay, (int, float)) and error_reset_delay >= 0, \
            "error_reset_delay must be a positive int or float"
        assert isinstance(save_all_data, bool), "save_all_data should be bool"
        assert motion_extraction_method in ("average", "flow", "phase"), "motion_extraction_method must be 'average', 'flow' or 'phase'"
        assert buffer_dtype in ("float64", "float32", "float16", "uint8", "uint16", "bgr8")
        assert isinstance(relocate_every, int) and relocate_every >= 0, "relocate_every must be a non-negative int"

        self.benchmarker = Benchmarker()
        self.error_reset_delay = error_reset_delay
        self.save_all_data = save_all_data
        self.fig_size = fig_size
        self.save_calibration_image = save_calibration_image
        self.capture_target = capture_target
        self.visualize = visualize
        self.motion_extraction_method = motion_extraction_method
        self.buffer_dtype = buffer_dtype
        self._backend = backend if backend is not None else _Backend()
        self.relocate_every = relocate_every
        self._window = None              # SlidingCalibration, made with the first frame it is given (relocate_every > 0)
        self._window_stage = None        # staging buffer of the calibration buffer's dtype for the frames of 'measure'
        self._since_relocate = 0

        self.cap = self._open_capture(capture_target)                       # base.py:48
        self.fps = int(self.cap.get(self.CAP_PROP_FPS))                     # base.py:49
        self.width = int(self.cap.get(self.CAP_PROP_FRAME_WIDTH))
        self.height = int(self.cap.get(self.CAP_PROP_FRAME_HEIGHT))

        # hyperparameters, reference base.py:80-106
        self.maximum_bounding_box_area = np.inf
        self.calibration_buffer_target_length = 128
        self.freq_min = 0.1
        self.freq_max = 1.0
        self.temporal_threshold = 0.7
        self.threshold = 0.08
        self.measure_buffer_length = 128
        self.confidence_interval = 0.95
        self.feature_params = dict(maxCorners=100, qualityLevel=0.3, minDistance=7, blockSize=7)
        self.lk_params = dict(winSize=(15, 15), maxLevel=2,
                              criteria=(self.TERM_CRITERIA_EPS | self.TERM_CRITERIA_COUNT, 10, 0.03))
        self.phase_params = dict(level=1)
        self.phase_params.update(phase_params or {})
        self._phase_state, self._phase_begun = None, False
        self.gaussian_cutoff = 10.0
        self.filter_order = 3
        self.peak_minimum_sample_distance = 0
        self.measure_initialization_length = 12
        if self.fps == 0:
            self.fps = np.nan                                               # base.py:109-110
        self.fps_limit = fps_limit

        self.x, self.y, self.w, self.h = None, None, None, None
        self.disable_error_detection = False
        self.calibration_buffer_idx = 0
        self.calibration_buffer = self._alloc_buffer()                      # base.py:119-120, in HBM
        self.all_data = []
        self.data = deque()
        self.t = deque()
        self.freq = deque()
        self.confidence = deque()
        self.num_peaks = deque()
        self.num_peaks_mean = deque()
        self.motion_data = deque()
        self.filtered_data = []
        self.peak_indices = []
        self.peak_times = []
        self._frame_u8 = None            # current gray frame, device uint8 [H,W]
        self._frame_bgr = None           # ... and, for buffer_dtype 'bgr8' only, the captured frame it came from, device uint8 [H,W,3]
        self.cropped_image = None        # (x, y, w, h) view descriptor of the current frame
        self.previous_cropped_image = None
        self.display_frame = None
        self.motion_key_points = None
        self.video_out = None
        self.error_message = None
        self.buffers = [self.data, self.confidence, self.t, self.freq, self.num_peaks, self.num_peaks_mean,
                        self.motion_data]
        self.state = 'initialize'
        logging.info("Capturing {0} calibration frames.".format(self.calibration_buffer_target_length))
        self.calibration_start_time = np.nan
        self.loop_start_time = np.nan
        self.reset_start_time = np.nan
        self.frames_consumed = 0
        if run_on_init:
            self.run()                                                      # base.py:164

    # ------------------------------------------------------------------ plumbing
    def _open_capture(self, target):
        if all(hasattr(target, a) for a in ("isOpened", "read", "get", "release")):
            return target
        try:
            import cv2  # not part of this build's dependencies; only needed for real cameras / files
        except ImportError:
            raise _capi.RespmonError("capture_target=%r needs OpenCV's VideoCapture, which is not installed; pass an "
                                     "object with isOpened/read/get/release (e.g. respmon_amd.synth.FakeCapture)" % (target,))
        return cv2.VideoCapture(target)

    def _alloc_buffer(self):
        if isinstance(self._backend, _Backend):
            t = device.require_gpu()
            if self.buffer_dtype == "bgr8":    # north_star's [T,H,W,C] frame buffer: frames as captured, 3 bytes per pixel
                return t.zeros((self.calibration_buffer_target_length, self.height, self.width, 3), dtype=t.uint8, device="cuda")
            shape = (self.calibration_buffer_target_length, self.height, self.width)
            if self.buffer_dtype == "uint16":  # (zeroed through its bits: torch fills few unsigned types wider than a byte on the device)
                return t.zeros(shape, dtype=t.int16, device="cuda").view(t.uint16)
            dt = {"float64": t.float64, "float32": t.float32, "float16": t.float16, "uint8": t.uint8}[self.buffer_dtype]
            return t.zeros(shape, dtype=dt, device="cuda")
        return self._backend.alloc_buffer(self.calibration_buffer_target_length, self.height, self.width, self.buffer_dtype)

    @property
    def current_frame(self):
        """float64 [H,W] host copy of the current frame (uint8_to_float(gray), base.py:231; a uint16 frame: k * (1./65535))."""
        if self._frame_u8 is None:
            return None
        g = self._frame_u8
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        return g * (1. / 65535) if g.dtype == np.uint16 else g * (1. / 255)

    # ------------------------------------------------------------------ reference methods
    def skip_calibration(self, x, y, w, h):
        """base.py:166-172."""
        self.x, self.y, self.w, self.h = x, y, w, h
        self.peak_minimum_sample_distance = int(np.floor(self.fps / self.freq_max))
        self.state = 'measure'

    def next_frame(self):
        """base.py:227-233: read -> BGR2GRAY -> (uint8_to_float is applied by the consumers); False at end.
        A 2-D uint16 frame (a Y16 capture with CAP_PROP_CONVERT_RGB off) is gray already: it stays uint16, on the device."""
        ret, frame = self.cap.read()
        if ret and getattr(frame, "ndim", 0) == 2 and frame.dtype == np.uint16:
            self._frame_u8, self._frame_bgr = self._backend.gray16(frame), None
            self.frames_consumed += 1
            return self._frame_u8
        if ret:
            self._frame_u8 = self._backend.bgr_to_gray(frame)
            # a 'bgr8' calibration buffer stores the frame as captured: keep the device copy the backend made of it for step()
            # (only then: nothing else needs it, and it is released with the next frame)
            self._frame_bgr = getattr(self._backend, "last_bgr", None) if self.buffer_dtype == "bgr8" else None
            self.frames_consumed += 1
            return self._frame_u8
        return False

    def initialize(self):
        """base.py:299-301."""
        self.calibration_start_time = time.time()
        self.calibration_buffer_idx = 0

    def detect_fps(self):
        """base.py:303-310: measured fps if the capture reports none, then clamp to fps_limit."""
        if self.fps == 0 or self.fps is np.nan:
            self.fps = self.calibration_buffer_target_length / (time.time() - self.calibration_start_time)
            logging.info("Computer FPS as {0}.".format(self.fps))
        if self.fps > self.fps_limit:
            self.fps = self.fps_limit
            logging.info("FPS Limited to {0}.".format(self.fps))
        logging.info("Final FPS is {0}.".format(self.fps))

    def trigger_error(self, message):
        """base.py:249-253."""
        self.error_message = message
        self.reset_start_time = time.time()
        logging.warning(message)
        self.state = 'error'

    def detect_errors(self):
        """base.py:543-545 (identity test against np.nan, as the reference does)."""
        if self.data[-1] is np.nan:
            return True

    def reset(self):
        """base.py:515-533 without the UI calls."""
        self.state = 'initialize'
        for b in self.buffers:
            b.clear()
        self.filtered_data = []
        self.peak_indices = []
        self.peak_times = []
        self.calibration_buffer_idx = 0
        self.previous_cropped_image = None
        self.motion_key_points = None
        self._phase_state, self._phase_begun = None, False

    def sync_to_fps(self):
        """base.py:535-541."""
        fps_x = self.fps_limit if self.fps is np.nan else self.fps
        sleep_time = (1.0 / fps_x) - (time.time() - self.loop_start_time)
        if sleep_time > 0:
            time.sleep(sleep_time)

    def update_ui(self):
        """base.py:255-297: no UI in this build."""

    # BPM estimation (find_peaks / measure, base.py:312-352) and the per-frame bookkeeping of the 'measure' state (_pop_full_buffers /
    # _record_value, base.py:473-497) live in respmon_amd/measure.py BreathSignal, shared with respmon_amd.subjects.SubjectTracker.

    # ------------------------------------------------------------------ hot path B
    def extract_motion(self):
        """base.py:354-407."""
        x, y, w, h = self.cropped_image
        if self.motion_extraction_method == "average":
            return self._backend.roi_mean(self._frame_u8, x, y, w, h)       # np.average(crop), base.py:357
        be = self._backend
        if self.motion_extraction_method == "phase":
            return self._extract_motion_phase(be, x, y, w, h)
        if self.fused_flow_step and hasattr(be, "flow_step"):
            return self._extract_motion_flow_resident(be, x, y, w, h)
        if self.previous_cropped_image is None:                            # base.py:363-369
            self.previous_cropped_image = be.roi_to_uint8(self._frame_u8, x, y, w, h)
            self.motion_key_points = be.good_features_to_track(self.previous_cropped_image, **self.feature_params)
            if self.motion_key_points is None or len(self.motion_key_points) < 1:
                self.trigger_error("No motion key points found.")
            return 0.0
        cur = be.roi_to_uint8(self._frame_u8, x, y, w, h)
        if self.motion_key_points is None or len(self.motion_key_points) == 0:
            return np.nan
        p1, st = be.calc_optical_flow_pyr_lk(self.previous_cropped_image, cur, self.motion_key_points, **self.lk_params)
        mean, n_good = be.mean_flow(self.motion_key_points, p1, st)         # base.py:377-378, 388
        self.previous_cropped_image = cur                                   # base.py:381
        self.motion_key_points = p1[st == 1].reshape(-1, 1, 2)              # base.py:382
        if n_good == 0:
            return np.nan                                                   # base.py:385-386
        self.motion_data.append([mean[0], mean[1]])                         # base.py:389
        if len(self.motion_data) >= 2:
            return be.pca_reduce(np.array(self.motion_data, dtype=np.float32))  # base.py:396-405
        return 0.0

    # One C-ABI call per frame (rm_flow_begin / rm_flow_step): the previous crop and the tracked points stay on the device, so
    # `previous_cropped_image` only marks that tracking has begun and `motion_key_points` is fetched when somebody reads it.
    # False: the reference's four steps as four calls, points and status through host memory (same numbers).
    fused_flow_step = True
    _RESIDENT = "on the device (rm_flow_step)"

    def _extract_motion_flow_resident(self, be, x, y, w, h):
        if self.previous_cropped_image is None:                            # base.py:363-369
            if getattr(self, "_flow_state", None) is None:
                self._flow_state = be.flow_state()                         # this monitor's own tracking session
            self.motion_key_points = be.flow_begin(self._flow_state, self._frame_u8, x, y, w, h, **self.feature_params)
            self.previous_cropped_image = self._RESIDENT
            self._flow_cap = max(int(self.feature_params["maxCorners"]), 1)
            self._flow_n = 0 if self.motion_key_points is None else len(self.motion_key_points)
            if self._flow_n < 1:
                self.trigger_error("No motion key points found.")
            return 0.0
        if self.previous_cropped_image is not self._RESIDENT:              # tracking was begun by the four-call path
            self.fused_flow_step = False
            return self.extract_motion()
        if self._flow_n == 0:
            be.flow_step(self._flow_state, self._frame_u8, x, y, w, h, **self.lk_params)     # (the previous image still advances, base.py:381)
            return np.nan
        mean, n_good = be.flow_step(self._flow_state, self._frame_u8, x, y, w, h, **self.lk_params)   # base.py:371-388
        self._flow_n = n_good
        self._points_stale = True
        if n_good == 0:
            return np.nan                                                   # base.py:385-386
        self.motion_data.append([mean[0], mean[1]])                         # base.py:389
        if len(self.motion_data) >= 2:
            return be.pca_reduce(np.array(self.motion_data, dtype=np.float32))  # base.py:396-405
        return 0.0

    # 'phase': one rm_phase_motion_clip call of N == 1 per frame on a session the monitor owns.  The session's first frame only becomes
    # its state (value 0.0); a frame without amplitude (Sw == 0) takes the path n_good == 0 takes in 'flow' mode; every other frame
    # appends float32(v) to motion_data, and from the second row on the value is the PCA of the rows: the flow bookkeeping.
    def _phase_session(self, be, w, h):
        st = self._phase_state
        if st is None or (st.w, st.h) != (w, h):
            st = self._phase_state = be.phase_motion_state(w, h, int(self.phase_params["level"]))
            self._phase_begun = False
        return st

    def _extract_motion_phase(self, be, x, y, w, h):
        st = self._phase_session(be, w, h)
        begins = not self._phase_begun
        Sw, Sc, Ss = be.phase_motion_clip(st, self._frame_u8[None], x, y)[0]
        self._phase_begun = True
        if begins:
            return 0.0
        if not Sw > 0:
            return np.nan
        self.motion_data.append([np.float32(Sc / Sw), np.float32(Ss / Sw)])
        if len(self.motion_data) >= 2:
            return be.pca_reduce(np.array(self.motion_data, dtype=np.float32))
        return 0.0

    def _phase_clip_values(self, be, frames, x, y, w, h):
        """The device work of a clip in 'phase' mode: one rm_phase_motion_clip call plus one rm_pca_reduce_windows call; returns
        value(i) as _flow_clip_values does.  The session runs to the clip's end even if the replay stops at an error frame: reset()
        discards it before measuring begins again."""
        st = self._phase_session(be, w, h)
        begins = not self._phase_begun
        sums = be.phase_motion_clip(st, frames, x, y)
        self._phase_begun = True
        rows, first = self._phase_clip_rows(sums, begins)
        pca = be.pca_reduce_windows(rows, first, self.measure_buffer_length) if len(rows) > first else []
        return self._phase_clip_replay(sums, begins, pca)

    @property
    def motion_key_points(self):
        if getattr(self, "_points_stale", False):
            self._motion_key_points = self._backend.flow_points(self._flow_state, self._flow_cap)
            self._points_stale = False
        return getattr(self, "_motion_key_points", None)

    @motion_key_points.setter
    def motion_key_points(self, value):
        self._motion_key_points = value
        self._points_stale = False

    # Which cv2.findContours the ROI stage reproduces (the reference pins no OpenCV version, README.md:12): False = OpenCV >= 3.2
    # (pixels on the image frame count), True = OpenCV <= 3.1 (the 1-pixel frame is zeroed before tracing; base.py:567's
    # `thresh_copy` exists because that version mutated its input).  include/respmon_hip.h rm_set_contour_clip_frame.
    opencv_contours_clip_frame = False
    # Operation order of the calibration.  False (default): the temporal filter runs on the Gaussian level G_S and the Laplacians are
    # taken of the filtered images -- the linear stages commuted, results within ~1e-15 of the band-passed magnitudes of the
    # reference's order.  True: the reference's own order (Laplacians first, transforms.py:148-170; RM_FLAG_FILTER_LAPLACIANS),
    # bit-identical to the per-level kernels, a few per cent slower.  locate() is a static method (as in the reference, base.py:547):
    # both switches are read from RespiratoryMonitor itself, not from a subclass.
    reference_operation_order = False

    # ------------------------------------------------------------------ hot path A
    @staticmethod
    def locate(calibration_video_data, fps,
               freq_min=0.1, freq_max=1.0, amplification=500,
               pyramid_levels=9, skip_levels_at_top=4, temporal_threshold=0.7,
               threshold=20, threshold_type=THRESH_BINARY,
               verbose=False, save_calibration_image=False):
        """base.py:547-601 -> (x, y, w, h) or None.  Fused device path: the frame buffer is read once
        and no [T,H,W] intermediate is written (rm_locate)."""
        if threshold_type != THRESH_BINARY:
            raise NotImplementedError("only cv2.THRESH_BINARY is used by the reference (base.py:448,551)")
        logging.info("Beginning processing calibration frames...")
        buf = device.to_device(calibration_video_data)
        roi = _Backend().locate(buf, fps, freq_min, freq_max, amplification, pyramid_levels, skip_levels_at_top,
                                temporal_threshold, threshold,
                                flags=(_capi.RM_FLAG_CONTOUR_CLIP_FRAME if RespiratoryMonitor.opencv_contours_clip_frame else 0) |
                                      (_capi.RM_FLAG_FILTER_LAPLACIANS if RespiratoryMonitor.reference_operation_order else 0))
        if save_calibration_image and roi is not None:     # base.py:577-596 (the reference returns before it when no contour)
            from . import montage
            logging.info('Creating calibration image.')
            path, _ = montage.save_calibration_image(buf, fps, freq_min=freq_min, freq_max=freq_max, amplification=amplification,
                                                     pyramid_levels=pyramid_levels, skip_levels_at_top=skip_levels_at_top,
                                                     temporal_threshold=temporal_threshold, threshold=threshold)
            logging.info('Calibration image saved: %s', path)
        if verbose and roi is not None:
            print('x:{0}, y:{1}, w:{2}, h:{3}'.format(*roi))
        return roi

    @staticmethod
    def locate_all(calibration_video_data, fps,
                   freq_min=0.1, freq_max=1.0, amplification=500,
                   pyramid_levels=9, skip_levels_at_top=4, temporal_threshold=0.7,
                   threshold=20, threshold_type=THRESH_BINARY,
                   verbose=False, max_rois=4, min_area=0.0):
        """locate() for a frame that holds several subjects: where base.py:571 keeps max(contours, key=cv2.contourArea), this returns
        the bounding rectangles of the `max_rois` largest contours with contourArea >= min_area, largest first, as a list of
        (x, y, w, h) -- empty where locate() returns None.  Equal areas rank in the order of cv2.findContours' list, so with
        min_area == 0 the first entry is locate()'s ROI.  One calibration pass (rm_locate_multi); not a reference function."""
        if threshold_type != THRESH_BINARY:
            raise NotImplementedError("only cv2.THRESH_BINARY is used by the reference (base.py:448,551)")
        buf = device.to_device(calibration_video_data)
        rois = _Backend().locate_multi(buf, fps, freq_min, freq_max, amplification, pyramid_levels, skip_levels_at_top,
                                       temporal_threshold, threshold,
                                       flags=(_capi.RM_FLAG_CONTOUR_CLIP_FRAME if RespiratoryMonitor.opencv_contours_clip_frame else 0) |
                                             (_capi.RM_FLAG_FILTER_LAPLACIANS if RespiratoryMonitor.reference_operation_order else 0),
                                       max_rois=max_rois, min_area=min_area)
        if verbose:
            for roi in rois:
                print('x:{0}, y:{1}, w:{2}, h:{3}'.format(*roi))
        return rois

    @rate.static_or_instance
    def rate_map(self, frames=None, fps=None, level=None, nfreq=64, freq_min=None, freq_max=None):
        """How fast each part of the frame breathes: a rate.RateMap (bpm, periodicity, roi_bpm(roi)) at pyramid level `level` (default
        4) -- the dominant frequency of the band per pixel and the share of the band's power in it (rm_rate_map).  On a monitor the
        defaults are its calibration buffer, fps, freq_min and freq_max; RespiratoryMonitor.rate_map(frames, fps) is the static form,
        like locate(), with the band of locate()'s defaults.  Feed roi_bpm the rectangles of locate_all()."""
        if frames is None:
            if self is None:
                raise TypeError("RespiratoryMonitor.rate_map(frames, fps): the static form needs the frames")
            frames = self.calibration_buffer
        if fps is None:
            if self is None:
                raise TypeError("RespiratoryMonitor.rate_map(frames, fps): the static form needs fps")
            fps = self.fps
        if freq_min is None:
            freq_min = self.freq_min if self is not None else 0.1
        if freq_max is None:
            freq_max = self.freq_max if self is not None else 1.0
        return rate.buffer_rate_map(frames, fps, freq_min, freq_max, 4 if level is None else level, nfreq)

    @rate.static_or_instance
    def pulse_map(self, frames=None, fps=None, block=16, window=None, freq_min=0.7, freq_max=3.0, nfreq=64):
        """Where the pulse shows and how fast it is: a rate.RateMap over blocks of `block` x `block` pixels (level = log2(block)) from
        the POS projection of the three colour channels (pulse.pulse_map, rm_pulse_map) -- skin is where `periodicity` is high, and
        roi_bpm takes the rectangles of locate_all().  On a monitor the defaults are its calibration buffer and fps;
        RespiratoryMonitor.pulse_map(frames, fps) is the static form.  The band is the pulse's (0.7 - 3.0 Hz), not the monitor's
        breathing band.  Needs buffer_dtype 'bgr8': a gray buffer holds no pulse signal for POS (ValueError)."""
        from . import pulse
        if frames is None:
            if self is None:
                raise TypeError("RespiratoryMonitor.pulse_map(frames, fps): the static form needs the frames")
            frames = self.calibration_buffer
        if fps is None:
            if self is None:
                raise TypeError("RespiratoryMonitor.pulse_map(frames, fps): the static form needs fps")
            fps = self.fps
        return pulse.pulse_map(frames, fps, block, window, freq_min, freq_max, nfreq)

    calibrate = locate  # north_star names a calibrate(); the reference's calibration entry is locate()

    def magnified_calibration_video(self, out_dtype=None, color=False, method='linear', amplification=None):
        """The current calibration buffer with its breathing motion amplified -- what locate() looks at, frame by frame: the frames plus
        the band-passed signal of locate()'s defaults (amplification 500, pyramid_levels 9, skip_levels_at_top 4) at the monitor's fps,
        freq_min and freq_max (transforms.eulerian_magnification_video).  A device tensor [T,H,W]; `out_dtype` None: uint8 for a uint8 or
        'bgr8' buffer, uint16 for a uint16 one, float64 otherwise.  `color=True` (buffer_dtype 'bgr8' only): the frames as captured with
        that motion laid over them, [T,H,W,3] uint8 BGR.
        `method='phase'`: the buffer through transforms.phase_magnification_video instead (phase-based magnification on the Riesz pyramid
        at the monitor's fps and band, its own defaults otherwise: `amplification` 10 unless given, pyramid_levels 5, every level but
        the residual processed); gray only -- a 'bgr8' buffer is converted first, color=True is refused.  `amplification` is read by
        this method alone."""
        from .transforms import eulerian_magnification_video
        if method == 'phase':
            from .transforms import bgr_buffer_to_gray, phase_magnification_video
            if color:
                raise ValueError("magnified_calibration_video(method='phase') is gray only (color=True is not supported)")
            buf = self.calibration_buffer
            if device.is_bgr_buffer(buf):
                buf = bgr_buffer_to_gray(buf)
            return phase_magnification_video(buf, self.fps, self.freq_min, self.freq_max, 10 if amplification is None else amplification,
                                             out_dtype=out_dtype)
        if method != 'linear':
            raise ValueError("method must be 'linear' or 'phase', got %r" % (method,))
        if color and not device.is_bgr_buffer(self.calibration_buffer):
            raise ValueError("magnified_calibration_video(color=True) needs buffer_dtype='bgr8'; this monitor's buffer_dtype is %r"
                             % (getattr(self, "buffer_dtype", str(self.calibration_buffer.dtype).replace("torch.", "")),))
        return eulerian_magnification_video(self.calibration_buffer, self.fps, self.freq_min, self.freq_max, 500,
                                            pyramid_levels=9, skip_levels_at_top=4, out_dtype=out_dtype, color=color)

    # ------------------------------------------------------------------ state machine
    def run(self):
        """base.py:409-513.  Frame accounting: frame 0 is consumed by 'initialize', the next
        T fill the buffer, one more triggers locate() and is dropped, measurement starts after that."""
        self._add_benchmark_tags()
        while self.cap.isOpened():
            self.loop_start_time = time.time()
            self.benchmarker.tick_start('Frame Capture')
            frame = self.next_frame()
            if isinstance(frame, bool):
                break
            self.benchmarker.tick_end('Frame Capture')
            if self.measure_clip_length > 1 and self.state == 'measure':
                if not self._run_clip(frame):
                    break
            else:
                self.step(frame)
            self.update_ui()
            self.sync_to_fps()
        logging.info("Capture closed.")
        self.cap.release()

    def _add_benchmark_tags(self):
        for tag in ('Measurement Loop', 'Frame Capture', 'Calibration Measurement'):
            if not self.benchmarker.has_tag(tag):
                self.benchmarker.add_tag(tag)

    # Frames of the 'measure' state that run() collects into one device buffer and hands to step_clip() in one go.  1: run() steps
    # frame by frame, as the reference does.
    measure_clip_length = 1

    def _run_clip(self, frame):
        """`frame` and up to measure_clip_length - 1 further captured frames as one clip; False when the capture ended."""
        K = int(self.measure_clip_length)
        buf = getattr(self, "_clip_buf", None)
        if buf is None or len(buf) != K or tuple(buf.shape[1:]) != tuple(frame.shape) or buf.dtype != frame.dtype:
            if isinstance(frame, np.ndarray):
                buf = np.empty((K,) + tuple(frame.shape), dtype=frame.dtype)
            else:
                t = device.torch()
                buf = t.empty((K,) + tuple(frame.shape), dtype=frame.dtype, device=frame.device)
            self._clip_buf = buf
        buf[0] = frame
        n, open_ = 1, True
        while n < K:
            self.benchmarker.tick_start('Frame Capture')
            frame = self.next_frame()
            if isinstance(frame, bool):
                open_ = False
                break
            self.benchmarker.tick_end('Frame Capture')
            buf[n] = frame
            n += 1
        done = 0
        while done < n:
            done += self.step_clip(buf[done:n])
        return open_

    def step_clip(self, frames):
        """`for f in frames: step(f)` (each f being the current frame, as after next_frame()) with the device work of the 'measure'
        state done per clip: one rm_roi_mean_clip call, or one rm_flow_clip / rm_phase_motion_clip plus one rm_pca_reduce_windows call, then the per-frame
        host bookkeeping replayed in order.  frames: [N,H,W] gray frames, a device tensor or a numpy array.  Returns the number of
        frames consumed: it stops behind the frame on which the state leaves 'measure'; frames met in any other state go through
        step() one by one."""
        self._add_benchmark_tags()
        if isinstance(frames, np.ndarray) and isinstance(self._backend, _Backend):
            frames = device.to_device(frames)
        n, done = len(frames), 0
        while done < n:
            if self.state != 'measure':
                self._step_frame(frames[done])
                done += 1
                continue
            done += self._measure_clip(frames[done:])
            if self.state != 'measure':
                break
        return done

    def _step_frame(self, frame):
        self._frame_u8, self._frame_bgr = frame, None
        self.step(frame)

    def _measure_clip(self, frames):
        x, y, w, h = self.x, self.y, self.w, self.h
        be = self._backend
        if self.relocate_every > 0:
            frames = frames[:self.relocate_every - self._since_relocate]    # a clip ends where the ROI is taken again
        n = len(frames)
        if self.motion_extraction_method == "average":
            means = be.roi_mean_clip(frames, x, y, w, h)
            value_of = lambda i: float(means[i])
        elif self.motion_extraction_method == "phase":
            if len(self.motion_data) > self.measure_buffer_length:
                for i in range(n):                                           # the per-frame calls (a deque longer than the popleft rule keeps it)
                    self._step_frame(frames[i])
                    if self.state != 'measure':
                        return i + 1
                return n
            value_of = self._phase_clip_values(be, frames, x, y, w, h)
        else:
            begun = self.previous_cropped_image
            if (not self.fused_flow_step or not hasattr(be, "flow_clip") or (begun is not None and begun is not self._RESIDENT)
                    or len(self.motion_data) > self.measure_buffer_length):
                for i in range(n):                                           # the per-frame calls (four-call path, or a backend without clips)
                    self._step_frame(frames[i])
                    if self.state != 'measure':
                        return i + 1
                return n
            if begun is None:                                               # base.py:363-369: the corners come from the first frame
                self._step_frame(frames[0])
                if n == 1 or self.state != 'measure':
                    return 1
                return 1 + self._measure_clip(frames[1:])
            value_of = self._flow_clip_values(be, frames, x, y, w, h)
        for i in range(n):
            self.benchmarker.tick_start('Measurement Loop')
            self._frame_u8, self._frame_bgr = frames[i], None
            self.cropped_image = (x, y, w, h)
            self._pop_full_buffers()
            self._record_value(value_of(i))
            self.benchmarker.tick_end('Measurement Loop')
            if self.state != 'measure':
                n = i + 1
                break
        if self.relocate_every > 0:
            self._window_measured(frames[:n])
        return n

    def _flow_clip_values(self, be, frames, x, y, w, h):
        """The device work of a clip in 'flow' mode; returns value(i) = what extract_motion() returns for frame i, to be called once
        per frame, in order, behind the popleft rule of base.py:473-475 (it does extract_motion's bookkeeping on motion_data).
        The clip is tracked to its end even if the replay then stops at an error frame.  That is harmless: both error causes ("No
        motion key points found.", a NaN value) leave the state without points, so the frames behind the error only advanced its
        previous image, and reset() discards the flow state before tracking begins again."""
        had_points = self._flow_n > 0
        mean, n_good = be.flow_clip(self._flow_state, frames, x, y, w, h, **self.lk_params)
        if not had_points:
            return lambda i: np.nan
        self._points_stale = True
        rows, first = self._flow_clip_rows(mean, n_good)
        pca = be.pca_reduce_windows(rows, first, self.measure_buffer_length) if len(rows) > first else []
        return self._flow_clip_replay(mean, n_good, pca)

    def step(self, frame):
        """One iteration of the reference's state dispatch (base.py:423-500) on an already captured frame."""
        if self.state == 'initialize':
            self.initialize()
            self.state = 'calibration'
        elif self.state == 'calibration':
            if self.calibration_buffer_idx < self.calibration_buffer_target_length:
                if self.buffer_dtype == "bgr8":
                    bgr = self._frame_bgr if frame is getattr(self, "_frame_u8", None) else None   # (a frame step() was handed from elsewhere: its gray value, three planes)
                    self._backend.store_frame(self.calibration_buffer, self.calibration_buffer_idx, frame, bgr=bgr)
                else:
                    self._backend.store_frame(self.calibration_buffer, self.calibration_buffer_idx, frame)
                self.calibration_buffer_idx += 1
                if self.relocate_every > 0:
                    was_full = self._window is not None and self._window.count >= self._window.T
                    self._window_push(self.calibration_buffer[self.calibration_buffer_idx - 1:self.calibration_buffer_idx])
                    if was_full:   # a reset() kept the ring: the ROI comes from it now, not after a refill
                        self._enter_measure(self._locate_window())
            else:
                logging.info("Finished capturing calibration frames. Beginning calibration...")
                self.detect_fps()
                self.peak_minimum_sample_distance = int(np.floor(self.fps / self.freq_max))
                self.benchmarker.tick_start('Calibration Measurement')
                location = self._locate_buffer()
                self.benchmarker.tick_end('Calibration Measurement')
                if location is None:
                    logging.info("Failed finding ROI during calibration. Retrying...")
                    self.calibration_buffer_idx = 0
                    return
                self.x, self.y, self.w, self.h = reduce_bounding_box(*location, self.maximum_bounding_box_area)
                self._since_relocate = 0
                logging.info("Finished calibration.")
                logging.info("Beginning measuring...")
                self.state = 'measure'
        elif self.state == 'measure':
            self.benchmarker.tick_start('Measurement Loop')
            self.cropped_image = (self.x, self.y, self.w, self.h)           # base.py:471 (a view descriptor)
            self._pop_full_buffers()
            self._record_value(self.extract_motion())
            self.benchmarker.tick_end('Measurement Loop')
            if self.relocate_every > 0:
                self._window_measured([frame])
        elif self.state == 'error':
            if time.time() - self.reset_start_time >= self.error_reset_delay:
                logging.info('Benchmark Report...\r\n' + self.benchmarker.get_report())
                self.reset()
                self.state = 'calibration'

    # ------------------------------------------------------------------ sliding window (relocate_every > 0)
    def _window_push(self, frames):
        if self._window is None:
            assert isinstance(self._backend, _Backend), "relocate_every > 0 needs the device backend"
            from .window import SlidingCalibration
            self._window = SlidingCalibration(self.calibration_buffer_target_length, self.height, self.width, 9, 4)
        self._window.push(frames, bgr=self.buffer_dtype == "bgr8")

    def _window_measured(self, frames):
        """The frames just measured go into the ring -- through a staging buffer of the calibration buffer's dtype, so the ring sees
        what store_frame stores -- and after relocate_every of them the ROI is taken again."""
        n = len(frames)
        stage = self._window_stage
        if stage is None or len(stage) < n:
            stage = self._window_stage = self.calibration_buffer.new_empty((n,) + tuple(self.calibration_buffer.shape[1:]))
        for i in range(n):
            if self.buffer_dtype == "bgr8":
                bgr = self._frame_bgr if frames[i] is getattr(self, "_frame_u8", None) else None
                self._backend.store_frame(stage, i, frames[i], bgr=bgr)
            else:
                self._backend.store_frame(stage, i, frames[i])
        self._window_push(stage[:n])
        self._since_relocate += n
        if self._since_relocate >= self.relocate_every:
            self._since_relocate = 0
            self._set_roi(self._locate_window())

    def _set_roi(self, location):
        """the ROI of a refresh; None (no contour in the ring) keeps the one held"""
        if location is None:
            return
        roi = tuple(reduce_bounding_box(*location, self.maximum_bounding_box_area))
        if roi != (self.x, self.y, self.w, self.h) and self.motion_extraction_method == "phase":
            # the previous level and the velocities gathered so far belong to the old rectangle: the session is discarded
            self._phase_state, self._phase_begun = None, False
            self.motion_data.clear()
        if roi != (self.x, self.y, self.w, self.h) and self.motion_extraction_method == "flow":
            # the crop, its corners and the displacements gathered so far belong to the old rectangle: tracking begins again
            # (rm_flow_begin, or goodFeaturesToTrack on the four-call path) with the next frame
            self.previous_cropped_image = None
            self.motion_key_points = None
            self.motion_data.clear()
        self.x, self.y, self.w, self.h = roi

    def _locate_window(self):
        """_locate_buffer on the frames the ring holds"""
        return self._window.locate(self.fps, self.freq_min, self.freq_max, 500, self.temporal_threshold, int(np.round(self.threshold * 255)))

    def _enter_measure(self, location):
        if location is None:
            return
        self.peak_minimum_sample_distance = int(np.floor(self.fps / self.freq_max))
        self.x, self.y, self.w, self.h = reduce_bounding_box(*location, self.maximum_bounding_box_area)
        self._since_relocate = 0
        self.state = 'measure'

    def _locate_buffer(self):
        """the locate() call of run(), base.py:444-448: threshold = int(round(0.08*255)) = 20; pyramid_levels=9,
        skip_levels_at_top=4, amplification=500 are locate's defaults."""
        thr = int(np.round(self.threshold * 255))
        roi = self._backend.locate(self.calibration_buffer, self.fps, self.freq_min, self.freq_max, 500, 9, 4,
                                   self.temporal_threshold, thr)
        if self.save_calibration_image and roi is not None:     # base.py:448 passes the flag on; montage at base.py:577-596
            from . import montage
            path, _ = montage.save_calibration_image(self.calibration_buffer, self.fps, freq_min=self.freq_min, freq_max=self.freq_max,
                                                     temporal_threshold=self.temporal_threshold, threshold=thr)
            logging.info('Calibration image saved: %s', path)
        return roi
