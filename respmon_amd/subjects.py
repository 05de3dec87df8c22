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
runs) -- without the monitor's capture, state machine and [128,H,W] calibration buffer.  extract_motion('flow') keeps one device
state per subject and is not batched: use one RespiratoryMonitor per subject for it.
"""
from collections import deque

import numpy as np

from .measure import BreathSignal


class Subject(BreathSignal):
    """The breathing signal of one region: `data`, `t`, `freq`, `filtered_data`, `peak_indices`, `peak_times` as on a
    RespiratoryMonitor (hyperparameters: base.py:80-106)."""

    def __init__(self, roi, fps, freq_max=1.0, measure_buffer_length=128, measure_initialization_length=12, filter_order=3,
                 gaussian_cutoff=10.0, save_all_data=False):
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

    @property
    def roi(self):
        return self.x, self.y, self.w, self.h

    @property
    def bpm(self):
        return self.freq[-1] if len(self.freq) else None


class SubjectTracker:
    def __init__(self, rois, fps, freq_max=1.0, measure_buffer_length=128, measure_initialization_length=12, filter_order=3,
                 gaussian_cutoff=10.0, save_all_data=False, backend=None):
        """rois: a sequence of (x, y, w, h), e.g. what RespiratoryMonitor.locate_all returned (1 .. RM_MAX_ROIS = 64 of them);
        fps: frames per second of the clips; the other arguments are the monitor's hyperparameters of the same names.
        backend -- a stand-in for the device backend (tests): an object with roi_mean_multi_clip(frames, rois) -> ndarray [N, K]."""
        rois = [tuple(int(v) for v in r) for r in rois]
        if not rois:
            raise ValueError("SubjectTracker needs at least one region")
        self.subjects = [Subject(r, fps, freq_max, measure_buffer_length, measure_initialization_length, filter_order, gaussian_cutoff,
                                 save_all_data) for r in rois]
        self._rois = np.array(rois, dtype=np.int32).reshape(-1, 4)
        if backend is None:
            from .base import _Backend
            backend = _Backend()
        self._backend = backend

    @property
    def rois(self):
        return [s.roi for s in self.subjects]

    @property
    def bpm(self):
        """Each subject's last frequency estimate in breaths per minute (None until measure() has found two peaks)."""
        return [s.bpm for s in self.subjects]

    def __len__(self):
        return len(self.subjects)

    def __getitem__(self, k):
        return self.subjects[k]

    def step_clip(self, frames):
        """frames: [N,H,W] gray frames of a frame dtype (device tensor, or numpy -- copied to the device).  The region means of every
        frame and subject come from one rm_roi_mean_multi_clip call; then each subject's bookkeeping of the 'measure' state is
        replayed frame by frame, as RespiratoryMonitor.step_clip does for its one region.  Returns the number of frames consumed."""
        from .base import _Backend
        if isinstance(frames, np.ndarray) and isinstance(self._backend, _Backend):
            from . import device
            frames = device.to_device(frames)
        means = self._backend.roi_mean_multi_clip(frames, self._rois)
        n = len(means)
        for i in range(n):
            for k, s in enumerate(self.subjects):
                s._pop_full_buffers()                                       # base.py:473-475
                s._record_value(float(means[i][k]))                         # base.py:477-497
        return n
