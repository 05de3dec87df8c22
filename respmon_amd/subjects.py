"""
Several subjects in one camera frame (a ward, a nursery, a sleep lab): RespiratoryMonitor.locate_all() finds their regions in
one calibration pass, SubjectTracker measures them all from every clip of gray frames with ONE device call.

    rois = RespiratoryMonitor.locate_all(calibration_frames, fps, max_rois=4)
    tracker = SubjectTracker(rois, fps)
    for clip in clips:                      # [N,H,W] gray frames, device tensor or numpy
        tracker.step_clip(clip)
    print(tracker.bpm)                      # each subject's last breaths-per-minute estimate, None where there is none yet

Not a reference class: the reference follows one region per camera (base.py:571 keeps the largest contour).  A subject here is the
'measure' state of a RespiratoryMonitor after skip_calibration(x, y, w, h) with motion_extraction_method='average' -- the same
pop-left rule, value bookkeeping, low-pass filter and peak search (respmon_amd/measure.py BreathSignal, the code the monitor itself
runs) -- without the monitor's capture, state machine and [128,H,W] calibration buffer.

    tracker = SubjectTracker(rois, fps, motion_extraction_method='flow')

follows the subjects by optical flow instead (Lucas-Kanade tracks of corners, then PCA: the method for regions whose mean is a weak
signal).  Every subject owns one device-resident tracking session; a clip still costs ONE rm_flow_multi_clip call and ONE
rm_pca_reduce_windows_multi call for all of them.  Subject k then equals a RespiratoryMonitor(motion_extraction_method='flow') in the
'measure' state after skip_calibration(*roi_k), up to and including the frame on which that monitor would leave 'measure' ("No
motion key points found.", or a NaN value once the last point is lost): there the subject is marked `lost` and ignored until
SubjectTracker.restart(k) begins its tracking again.

    tracker = SubjectTracker(rois, fps, motion_extraction_method='phase', phase_params=dict(level=1))

measures the amplitude-weighted mean phase velocity of one Riesz-pyramid level of every region (the method for regions that move a
fraction of a pixel at constant brightness and offer texture, not corners): ONE rm_phase_motion_multi_clip call and ONE
rm_pca_reduce_windows_multi call per clip, every subject on a session of its own, subject k equal to a
RespiratoryMonitor(motion_extraction_method='phase') after skip_calibration(*roi_k) in the same sense.
"""
from collections import deque

import numpy as np

from .measure import BreathSignal


class Subject(BreathSignal):
    """The breathing signal of one region: `data`, `t`, `freq`, `filtered_data`, `peak_indices`, `peak_times` as on a
    RespiratoryMonitor (hyperparameters: base.py:80-106)."""

    def __init__(self, roi, fps, freq_max=1.0, measure_buffer_length=128, measure_initialization_length=12, filter_order=3,
                 gaussian_cutoff=10.0, save_all_data=False, flow_state=None, phase_state=None):
        self.x, self.y, self.w, self.h = (int(v) for v in roi)
        self.fps = fps
        self.freq_max = freq_max
        self.measure_buffer_length = measure_buffer_length
        self.measure_initialization_length = measure_initialization_length
        self.filter_order = filter_order
        self.gaussian_cutoff = gaussian_cutoff
        self.peak_minimum_sample_distance = int(np.floor(fps / freq_max))      # base.py:168 (skip_calibration)
        self.save_all_data = save_all_data
        self.disable_error_detection = True     # (a NaN value is the 'flow' method's; the mean of a region is always a number)
        self.all_data = []
        self.data, self.t, self.freq = deque(), deque(), deque()
        self.filtered_data, self.peak_indices, self.peak_times = [], [], []
        self.buffers = [self.data, self.t, self.freq]
        self.lost, self.error_message = False, None
        if flow_state is not None:              # 'flow': one tracking session (rm_flow_state) and the displacement list of base.py:389
            self._flow_state, self._flow_begun, self._flow_n = flow_state, False, 0
            self.motion_data = deque()
            self.buffers.append(self.motion_data)                           # base.py:473-475 reaches it as in the reference
            self.disable_error_detection = False
        if phase_state is not None:             # 'phase': one session (rm_phase_motion) and the list of mean phase velocities
            self._phase_state, self._phase_begun = phase_state, False
            self.motion_data = deque()
            self.buffers.append(self.motion_data)
            self.disable_error_detection = False

    def detect_errors(self):
        """base.py:543-545 (the monitor's identity test against np.nan)."""
        if self.data[-1] is np.nan:
            return True

    def trigger_error(self, message):
        """Where a monitor leaves 'measure' (base.py:249-253) the subject is lost."""
        self.error_message = message
        self.lost = True

    @property
    def roi(self):
        return self.x, self.y, self.w, self.h

    @property
    def bpm(self):
        return self.freq[-1] if len(self.freq) else None


class SubjectTracker:
    def __init__(self, rois, fps, freq_max=1.0, measure_buffer_length=128, measure_initialization_length=12, filter_order=3,
                 gaussian_cutoff=10.0, save_all_data=False, backend=None, motion_extraction_method='average', feature_params=None,
                 lk_params=None, phase_params=None):
        """rois: a sequence of (x, y, w, h), e.g. what RespiratoryMonitor.locate_all returned (1 .. RM_MAX_ROIS = 64 of them);
        fps: frames per second of the clips; the other arguments are the monitor's hyperparameters of the same names.
        motion_extraction_method: 'average' (the region means), 'flow' (optical flow + PCA) or 'phase' (mean phase velocity + PCA);
        feature_params / lk_params: the arguments of goodFeaturesToTrack / calcOpticalFlowPyrLK in 'flow' mode, by default the monitor's
        (base.py:91-98); phase_params: dict(level=1), the pyramid level of the 'phase' mode.
        backend -- a stand-in for the device backend (tests): an object with roi_mean_multi_clip(frames, rois) -> ndarray [N, K],
        in 'flow' mode with flow_state / flow_begin / flow_points / flow_multi_clip / pca_reduce_windows_multi of _Backend, in 'phase'
        mode with phase_motion_state / phase_motion_multi_clip / pca_reduce_windows_multi."""
        assert motion_extraction_method in ("average", "flow", "phase"), "motion_extraction_method must be 'average', 'flow' or 'phase'"
        rois = [tuple(int(v) for v in r) for r in rois]
        if not rois:
            raise ValueError("SubjectTracker needs at least one region")
        if backend is None:
            from .base import _Backend
            backend = _Backend()
        self._backend = backend
        self.motion_extraction_method = motion_extraction_method
        self.feature_params = dict(feature_params) if feature_params else dict(maxCorners=100, qualityLevel=0.3, minDistance=7, blockSize=7)
        self.lk_params = dict(lk_params) if lk_params else dict(winSize=(15, 15), maxLevel=2, criteria=(3, 10, 0.03))
        self.phase_params = dict(level=1)
        self.phase_params.update(phase_params or {})
        flow, phase = motion_extraction_method == "flow", motion_extraction_method == "phase"
        self.subjects = [Subject(r, fps, freq_max, measure_buffer_length, measure_initialization_length, filter_order, gaussian_cutoff,
                                 save_all_data, flow_state=backend.flow_state() if flow else None,
                                 phase_state=self._phase_state(r) if phase else None) for r in rois]
        self._rois = np.array(rois, dtype=np.int32).reshape(-1, 4)

    @property
    def rois(self):
        return [s.roi for s in self.subjects]

    @property
    def bpm(self):
        """Each subject's last frequency estimate in breaths per minute (None until measure() has found two peaks)."""
        return [s.bpm for s in self.subjects]

    @property
    def lost(self):
        """Per subject: True once its tracking has failed ('flow' mode; see restart)."""
        return [s.lost for s in self.subjects]

    def __len__(self):
        return len(self.subjects)

    def __getitem__(self, k):
        return self.subjects[k]

    def step_clip(self, frames):
        """frames: [N,H,W] gray frames of a frame dtype (device tensor, or numpy -- copied to the device).  The region means of every
        frame and subject come from one rm_roi_mean_multi_clip call -- in 'flow' mode the mean displacements from one
        rm_flow_multi_clip call and the PCA values from one rm_pca_reduce_windows_multi call --; then each subject's bookkeeping of
        the 'measure' state is replayed frame by frame, as RespiratoryMonitor.step_clip does for its one region.  Returns the number
        of frames consumed."""
        from .base import _Backend
        if isinstance(frames, np.ndarray) and isinstance(self._backend, _Backend):
            from . import device
            frames = device.to_device(frames)
        if self.motion_extraction_method in ("flow", "phase"):
            live = [k for k, s in enumerate(self.subjects) if not s.lost]
            if live:
                (self._flow_clip if self.motion_extraction_method == "flow" else self._phase_clip)(frames, live)
            return len(frames)
        means = self._backend.roi_mean_multi_clip(frames, self._rois)
        n = len(means)
        for i in range(n):
            for k, s in enumerate(self.subjects):
                s._pop_full_buffers()                                       # base.py:473-475
                s._record_value(float(means[i][k]))                         # base.py:477-497
        return n

    def restart(self, k, roi=None):
        """Subject k begins again with the next frame: its signals are cleared as RespiratoryMonitor.reset() clears them (all_data
        is kept), it is no longer lost, and in 'flow' mode its corners are taken anew -- inside `roi` (x, y, w, h), e.g. a rectangle
        of SlidingCalibration.locate_all, if one is given."""
        s = self.subjects[k]
        if roi is not None:
            s.x, s.y, s.w, s.h = (int(v) for v in roi)
            self._rois[k] = s.roi
        for b in s.buffers:
            b.clear()
        s.filtered_data, s.peak_indices, s.peak_times = [], [], []
        s.lost, s.error_message = False, None
        if self.motion_extraction_method == "flow":
            s._flow_begun, s._flow_n = False, 0
        if self.motion_extraction_method == "phase":   # a new session: the rectangle may have another size
            s._phase_state, s._phase_begun = self._phase_state(s.roi), False

    def motion_key_points(self, k):
        """The points subject k still tracks ('flow' mode), [n,1,2] float32 in the ROI's coordinates as rm_flow_points returns them;
        None before its tracking has begun."""
        s = self.subjects[k]
        if not s._flow_begun:
            return None
        return self._backend.flow_points(s._flow_state, max(int(self.feature_params["maxCorners"]), 1))

    # ---- 'flow' mode -----------------------------------------------------------------------------------------------------------
    def _flow_clip(self, frames, ks):
        """The frames of a clip for the subjects `ks` (none of them lost)."""
        be = self._backend
        if len(frames) == 0 or not ks:
            return
        fresh = [k for k in ks if not self.subjects[k]._flow_begun]
        if fresh:
            # base.py:363-369: a subject's corners come from the first frame it sees; the value of that frame is 0.0.  Once per
            # session and subject.  Subjects already under way (the others were restarted) take that frame as a clip of their own.
            self._flow_clip(frames[:1], [k for k in ks if k not in fresh])
            for k in fresh:
                s = self.subjects[k]
                pts = be.flow_begin(s._flow_state, frames[0], s.x, s.y, s.w, s.h, **self.feature_params)
                s._flow_begun = True
                s._flow_n = 0 if pts is None else len(pts)
                s._pop_full_buffers()
                if s._flow_n < 1:
                    s.trigger_error("No motion key points found.")
                s._record_value(0.0)
            return self._flow_clip(frames[1:], [k for k in ks if not self.subjects[k].lost])
        subs = [self.subjects[k] for k in ks]
        mean, n_good = be.flow_multi_clip([s._flow_state for s in subs], frames, self._rois[ks], **self.lk_params)
        tracked = [s._flow_n > 0 for s in subs]
        rows, firsts = [], []
        for j, s in enumerate(subs):
            r, first = s._flow_clip_rows(mean[:, j], n_good[:, j]) if tracked[j] else (np.empty((0, 2), np.float32), 0)
            rows.append(r)
            firsts.append(first)
        if any(len(r) > f for r, f in zip(rows, firsts)):
            pca = be.pca_reduce_windows_multi(rows, firsts, subs[0].measure_buffer_length)
        else:
            pca = [[] for _ in subs]
        for j, s in enumerate(subs):
            value_of = s._flow_clip_replay(mean[:, j], n_good[:, j], pca[j]) if tracked[j] else (lambda i: np.nan)
            for i in range(len(frames)):
                s._pop_full_buffers()                                       # base.py:473-475
                s._record_value(value_of(i))                                # base.py:477-497
                if s.lost:
                    break                                                   # later frames are ignored for this subject

    # ---- 'phase' mode ----------------------------------------------------------------------------------------------------------
    def _phase_state(self, roi):
        return self._backend.phase_motion_state(int(roi[2]), int(roi[3]), int(self.phase_params["level"]))

    def _phase_clip(self, frames, ks):
        """The frames of a clip for the subjects `ks` (none of them lost): RespiratoryMonitor._phase_clip_values for all of them at once."""
        be = self._backend
        if len(frames) == 0 or not ks:
            return
        subs = [self.subjects[k] for k in ks]
        sums = be.phase_motion_multi_clip([s._phase_state for s in subs], frames, self._rois[ks])
        begins = [not s._phase_begun for s in subs]
        rows, firsts = [], []
        for j, s in enumerate(subs):
            s._phase_begun = True
            r, first = s._phase_clip_rows(sums[:, j], begins[j])
            rows.append(r)
            firsts.append(first)
        if any(len(r) > f for r, f in zip(rows, firsts)):
            pca = be.pca_reduce_windows_multi(rows, firsts, subs[0].measure_buffer_length)
        else:
            pca = [[] for _ in subs]
        for j, s in enumerate(subs):
            value_of = s._phase_clip_replay(sums[:, j], begins[j], pca[j])
            for i in range(len(frames)):
                s._pop_full_buffers()                                       # base.py:473-475
                s._record_value(value_of(i))                                # base.py:477-497
                if s.lost:
                    break                                                   # later frames are ignored for this subject
