"""
The breathing signal of ONE region and what the 'measure' state does with it: the per-frame bookkeeping of reference
base.py:473-497 and the BPM estimation of base.py:312-352.  RespiratoryMonitor (respmon_amd/base.py) is one such signal plus the
capture / calibration state machine; respmon_amd.subjects.SubjectTracker holds one per subject of a frame.  Both run THIS code.

A user of the mixin provides: fps, freq_max, filter_order, gaussian_cutoff, peak_minimum_sample_distance, measure_buffer_length,
measure_initialization_length, save_all_data, all_data, disable_error_detection, the deques data / t / freq, the list `buffers` of
the deques the pop-left rule applies to, and -- unless disable_error_detection is set -- detect_errors() / trigger_error().
For the 'flow' method's clips (_flow_clip_rows / _flow_clip_replay) also the deque motion_data and _flow_n, the number of points the
tracking session still has.  For the 'phase' method's clips (_phase_clip_rows / _phase_clip_replay) the deque motion_data.
"""
import numpy as np

from .transforms import butter_lowpass_filter


class BreathSignal:
    # ------------------------------------------------------------------ BPM estimation ("next" row f2)
    def find_peaks(self):
        """base.py:312-338 with own restatements of peakutils.indexes / gaussian_fit (peakutils is an
        un-pinned dependency that is not installable here: parity unpinned)."""
        from . import peaks
        width = self.peak_minimum_sample_distance
        idxs = peaks.indexes(np.asarray(self.filtered_data), min_dist=width)
        final, fits = [], []
        t_arr = np.array(self.t)
        f_arr = np.array(self.filtered_data)
        for idx in idxs:
            w = width
            if idx - width < 0:
                w = idx
            if idx + w > len(self.t):
                w = len(self.t) - idx
            ti, di = t_arr[idx - w:idx + w], f_arr[idx - w:idx + w]
            try:
                params = peaks.gaussian_fit(ti, di)
                fits.append(0.0)  # the reference's r2 is identically 0 (ssr == sst, base.py:330-332)
                if params[2] < self.gaussian_cutoff:
                    final.append(idx)
            except (RuntimeError, TypeError, ValueError):
                pass
        return final, fits

    def measure(self):
        """base.py:340-352."""
        self.filtered_data = np.array(butter_lowpass_filter(self.data, self.freq_max * 0.5, self.fps, self.filter_order))
        self.peak_indices, _fits = self.find_peaks()
        self.peak_times = np.take(self.t, self.peak_indices)
        diffs = [a - b for b, a in zip(self.peak_times, self.peak_times[1:])]
        if len(diffs) > 0:
            self.freq.append(60.0 / np.mean(diffs))

    def _pop_full_buffers(self):
        for b in self.buffers:                                              # base.py:473-475
            if len(b) >= self.measure_buffer_length:
                b.popleft()

    def _record_value(self, value):
        """What the 'measure' state does with the value of one frame (base.py:477-497)."""
        self.data.append(value)
        if len(self.t) == 0:
            self.t.append(0.)
        else:
            self.t.append(self.t[-1] + (1. / self.fps))
        if self.save_all_data:
            self.all_data.append((self.t[-1], value))
        if len(self.data) > self.measure_initialization_length:
            self.measure()
            if not self.disable_error_detection and self.detect_errors():
                self.trigger_error("error detection found poor signal")

    # ------------------------------------------------------------------ a clip of extract_motion('flow'), base.py:371-407
    def _flow_clip_rows(self, mean, n_good):
        """(rows, first): motion_data followed by the rows a tracked clip appends to it -- the frames in front of the one that loses
        the last point -- and the index of the first new row.  The deque holds at most measure_buffer_length rows (popleft before
        every frame), so frame i's PCA runs over that many rows ending in its own: pca_reduce_windows(rows, first, that length)."""
        k = 0
        while k < len(n_good) and n_good[k] > 0:
            k += 1
        first = len(self.motion_data)
        rows = np.array(list(self.motion_data) + [[mean[i][0], mean[i][1]] for i in range(k)], dtype=np.float32).reshape(-1, 2)
        return rows, first

    def _flow_clip_replay(self, mean, n_good, pca):
        """value(i) = what extract_motion() returns for frame i of a clip tracked from a state with points: mean [N,2] and n_good [N]
        of the clip, pca the values of its new rows.  To be called once per frame, in order, behind the popleft rule."""
        def value(i):
            if self._flow_n == 0:
                return np.nan
            self._flow_n = int(n_good[i])
            if self._flow_n == 0:
                return np.nan                                               # base.py:385-386 (the object np.nan: detect_errors tests identity)
            self.motion_data.append([mean[i][0], mean[i][1]])               # base.py:389
            if len(self.motion_data) >= 2:
                return float(pca[i])                                        # base.py:396-405
            return 0.0
        return value

    # ------------------------------------------------------------------ a clip of extract_motion('phase')
    # sums [N,3]: Sw, Sc, Ss of every frame (rm_phase_motion_clip).  A frame yields the 2-vector v = (Sc / Sw, Ss / Sw), the mean phase
    # velocity, where the flow path's frame yields its mean flow; behind that the bookkeeping is the flow path's.  `begins`: the clip's
    # first frame is the session's first (zeros; it only becomes the state).
    def _phase_clip_rows(self, sums, begins):
        """(rows, first): motion_data followed by the rows the clip appends to it -- one per frame with Sw > 0 -- and the index of the
        first new row; frame i's PCA runs over the measure_buffer_length rows ending in its own (see _flow_clip_rows)."""
        new = [[s[1] / s[0], s[2] / s[0]] for i, s in enumerate(sums) if not (begins and i == 0) and s[0] > 0]
        first = len(self.motion_data)
        rows = np.array(list(self.motion_data) + new, dtype=np.float32).reshape(-1, 2)
        return rows, first

    def _phase_clip_replay(self, sums, begins, pca):
        """value(i) = what extract_motion() returns for frame i of the clip: pca holds the values of its new rows.  To be called once
        per frame, in order, behind the popleft rule."""
        taken = [0]

        def value(i):
            if begins and i == 0:
                return 0.0
            Sw, Sc, Ss = sums[i]
            if not Sw > 0:
                return np.nan                                               # (the object np.nan: detect_errors tests identity)
            self.motion_data.append([np.float32(Sc / Sw), np.float32(Ss / Sw)])
            j = taken[0]
            taken[0] += 1
            if len(self.motion_data) >= 2:
                return float(pca[j])
            return 0.0
        return value
