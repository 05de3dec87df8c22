"""Shared cases of tests/test_emu_flow_multi.py (host-emulated build) and tests/test_gpu_flow_multi.py (the MI355X): builders of
frames, rectangles and call schedules for rm_flow_multi_clip / rm_pca_reduce_windows_multi / SubjectTracker(motion_extraction_method=
'flow'), and the comparison of a schedule against the per-subject calls it stands for.  Every comparison is bit for bit.  The
reference of a comparison is always the per-frame form ("step": rm_flow_step, kernels and host code of its own): rm_flow_clip is
the one-subject entry of the code behind rm_flow_multi_clip, so it stands beside "multi" as a subject, never as its reference.
No test functions here.

An `api` is one of the two adapters below: the same calls on numpy arrays through the emulated C-ABI, or on device tensors through
respmon_amd.base._Backend."""
import ctypes

import numpy as np

from respmon_amd import _capi, synth

WIN, LVL, CRIT = (15, 15), 2, (3, 10, 0.03)
LK = dict(winSize=WIN, maxLevel=LVL, criteria=CRIT)
BEGIN = (100, 0.3, 7, 7)
# rectangles on the 80 x 100 frames whose LK pyramids have 1, 2 and 3 levels, and the second one again
ROIS_EMU = [(30, 25, 24, 20), (12, 9, 70, 51), (0, 0, 100, 80), (12, 9, 70, 51)]


def lk_levels(h, w, win=WIN, lvl=LVL):
    """number of LK pyramid levels of an h x w crop (buildOpticalFlowPyramid: levels while the next one stays larger than the window)"""
    top, sh, sw = lvl, h, w
    for l in range(lvl + 1):
        sw, sh = (sw + 1) // 2, (sh + 1) // 2
        if sw <= win[0] or sh <= win[1]:
            top = l
            break
    return top + 1


def slot_bytes(h, w, win=WIN, lvl=LVL):
    """include/respmon_hip_debug.h "flow_clip_bytes": 5 bytes per pixel of every LK pyramid level of the ROI"""
    n, sh, sw = 0, h, w
    for _ in range(lk_levels(h, w, win, lvl)):
        n += sh * sw * 5
        sh, sw = (sh + 1) // 2, (sw + 1) // 2
    return n


def chunk_bytes(rois, frames_per_chunk):
    """the flow_clip_bytes at which a chunk of rm_flow_multi_clip holds that many frames of all these subjects"""
    return (frames_per_chunk + 1) * sum(slot_bytes(r[3], r[2]) for r in rois)


def frames_emu(amp=1.0, n=9):
    render = synth.synth_texture(80, 100, seed=99)
    return np.stack([render(amp * np.sin(0.5 * t), 0.5 * amp * np.cos(0.4 * t)) for t in range(n)])


def frames_unequal_lives(n=9, at=4, roi=ROIS_EMU[0]):
    """frames on which the subject `roi` loses every point in frame `at` (its whole crop is flat there: nothing to track on) while a
    larger subject keeps the points whose windows lie elsewhere"""
    f = frames_emu(1.0, n)
    x, y, w, h = roi
    f[at, y:y + h, x:x + w] = 9
    return f


def grid_rois(K, H, W, rw=351, rh=235):
    """the rectangles of tools/bench_subjects.py: K of rw x rh on a grid over the frame (they overlap from K = 16 on at 1080p)"""
    nx = int(np.ceil(np.sqrt(K)))
    ny = (K + nx - 1) // nx
    return [(int(round((k % nx) * (W - rw) / max(nx - 1, 1))), int(round((k // nx) * (H - rh) / max(ny - 1, 1))), rw, rh) for k in range(K)]


# ---- the two adapters ------------------------------------------------------------------------------------------------------------
class EmuApi:
    def __init__(self, emu):
        self.emu = emu

    def dev(self, a):
        return np.ascontiguousarray(a)

    def state(self):
        return self.emu.flow_state()

    def begin(self, st, frame, roi, begin=BEGIN):
        f = np.ascontiguousarray(frame)
        from tests.emu_harness import DT, ptr
        pts = np.empty((max(int(begin[0]), 1), 2), np.float32)
        n = ctypes.c_int()
        self.emu.ck(self.emu.lib.rm_flow_begin(self.emu.ctx, st, ptr(f), DT[f.dtype], f.shape[0], f.shape[1], *roi, int(begin[0]), float(begin[1]),
                                               float(begin[2]), int(begin[3]), ptr(pts), ctypes.byref(n), None), "flow_begin")
        return None if n.value == 0 else pts[:n.value].reshape(-1, 1, 2).copy()

    def step(self, st, frame, roi, win=None):
        f = np.ascontiguousarray(frame)
        win = win or WIN
        from tests.emu_harness import DT, ptr
        m = np.empty(2, np.float32); ng = ctypes.c_int()
        self.emu.ck(self.emu.lib.rm_flow_step(self.emu.ctx, st, ptr(f), DT[f.dtype], f.shape[0], f.shape[1], *roi, win[0], win[1], LVL, CRIT[1],
                                              float(CRIT[2]), ptr(m), ctypes.byref(ng), None), "flow_step")
        return m, ng.value

    def clip(self, st, frames, roi, win=None):
        f = np.ascontiguousarray(frames)
        win = win or WIN
        from tests.emu_harness import DT, ptr
        N, H, W = f.shape
        m = np.empty((N, 2), np.float32); ng = np.empty(N, np.int32)
        self.emu.ck(self.emu.lib.rm_flow_clip(self.emu.ctx, st, ptr(f), DT[f.dtype], N, H, W, *roi, win[0], win[1], LVL, CRIT[1], float(CRIT[2]),
                                              ptr(m), ptr(ng), None), "flow_clip")
        return m, ng

    def multi_rc(self, states, frames, rois, win=WIN, lvl=LVL, n=None, k=None, dtype=None, null=()):
        """the raw return code of rm_flow_multi_clip with outputs prefilled by a sentinel; `null`: argument names passed as NULL"""
        f = np.ascontiguousarray(frames)
        from tests.emu_harness import DT, ptr
        N, H, W = f.shape
        n = N if n is None else n
        r = np.ascontiguousarray(rois, np.int32).reshape(-1, 4)
        K = len(r) if k is None else k
        handles = (ctypes.c_void_p * max(len(states), 1))(*[getattr(s, "value", s) for s in states])
        rows, cols = max(min(n, N), 1), max(min(K, len(r)), 1)      # (a count the call must refuse is never written to)
        m = np.full((rows, cols, 2), 7, np.float32); ng = np.full((rows, cols), -7, np.int32)
        rc = self.emu.lib.rm_flow_multi_clip(self.emu.ctx, None if "states" in null else handles, None if "frames" in null else ptr(f),
                                             DT[f.dtype] if dtype is None else dtype, n, H, W, None if "rois" in null else ptr(r), K, win[0], win[1],
                                             lvl, CRIT[1], float(CRIT[2]), None if "mean" in null else ptr(m), None if "n_good" in null else ptr(ng), None)
        return rc, m, ng

    def multi(self, states, frames, rois, win=None):
        rc, m, ng = self.multi_rc(states, frames, rois, win=win or WIN)
        self.emu.ck(rc, "flow_multi_clip")
        return m, ng

    def points(self, st, cap=100):
        return self.emu.flow_points(cap, state=st)

    def set_bytes(self, n):
        self.emu.debug_set("flow_clip_bytes", n)

    def pca_one(self, rows):
        return self.emu.pca_reduce(rows)

    def pca(self, rows, first, window):
        from tests.emu_harness import ptr
        m = np.ascontiguousarray(rows, np.float32).reshape(-1, 2)
        out = np.empty(len(m) - first)
        self.emu.ck(self.emu.lib.rm_pca_reduce_windows(self.emu.ctx, ptr(m), len(m), first, window, ptr(out), None), "pca_reduce_windows")
        return out

    def pca_multi_rc(self, allrows, seg, window, k=None):
        from tests.emu_harness import ptr
        m = np.ascontiguousarray(allrows, np.float32).reshape(-1, 2)
        seg = np.ascontiguousarray(seg, np.int32).reshape(-1, 3)
        nout = max(int(sum(max(int(n) - int(f), 0) for _, n, f in seg)), 1)
        out = np.full(nout, -7.0)
        rc = self.emu.lib.rm_pca_reduce_windows_multi(self.emu.ctx, ptr(m), ptr(seg), len(seg) if k is None else k, window, ptr(out), None)
        return rc, out

    def pca_multi(self, rows_list, firsts, window):
        rows = [np.ascontiguousarray(m, np.float32).reshape(-1, 2) for m in rows_list]
        seg, at = [], 0
        for m, f in zip(rows, firsts):
            seg.append((at, len(m), int(f)))
            at += len(m)
        rc, out = self.pca_multi_rc(np.concatenate(rows) if rows else np.empty((0, 2), np.float32), seg, window)
        self.emu.ck(rc, "pca_reduce_windows_multi")
        counts = [n - f for _, n, f in seg]
        return [a.copy() for a in np.split(out[:sum(counts)], np.cumsum(counts)[:-1])]


class GpuApi:
    def __init__(self, be):
        self.be = be

    def dev(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def state(self):
        return self.be.flow_state()

    def begin(self, st, frame, roi, begin=BEGIN):
        return self.be.flow_begin(st, frame, *roi, *begin)

    def step(self, st, frame, roi, win=None):
        return self.be.flow_step(st, frame, *roi, **dict(LK, winSize=win or WIN))

    def clip(self, st, frames, roi, win=None):
        return self.be.flow_clip(st, frames, *roi, **dict(LK, winSize=win or WIN))

    def multi(self, states, frames, rois, win=None):
        return self.be.flow_multi_clip(states, frames, rois, **dict(LK, winSize=win or WIN))

    def points(self, st, cap=100):
        return self.be.flow_points(st, cap)

    def set_bytes(self, n):
        from respmon_amd import device
        device.debug_set("flow_clip_bytes", n)

    def pca_one(self, rows):
        return self.be.pca_reduce(rows)

    def pca(self, rows, first, window):
        return self.be.pca_reduce_windows(rows, first, window)

    def pca_multi(self, rows_list, firsts, window):
        return self.be.pca_reduce_windows_multi(rows_list, firsts, window)


# ---- a schedule of calls against the per-subject loop ------------------------------------------------------------------------------
def begin_all(api, frame0, rois, begins=None):
    """one fresh state per rectangle, begun on frame0 (begins[k]: the goodFeaturesToTrack arguments, or a frame to begin on instead)"""
    states, pts = [], []
    for k, roi in enumerate(rois):
        st = api.state()
        b = BEGIN if begins is None else begins[k]
        if isinstance(b, tuple):
            pts.append(api.begin(st, frame0, roi, b))
        else:
            pts.append(api.begin(st, b, roi))
        states.append(st)
    return states, pts


def run(api, frames, rois, schedule, begins=None, caps=None, win=None):
    """States begun on frames[0], then the schedule over the following frames.  An entry is (form, n): 'multi' = one
    rm_flow_multi_clip of n frames for all subjects, 'clip' = one rm_flow_clip of n frames per subject, 'step' = n rm_flow_step per
    subject.  No subject ever skips a frame: only the call form changes.  win: the LK window of every call (None: WIN).
    -> dict(states, pts0, mean [T,K,2], n_good [T,K], points [K] as rm_flow_points returns them afterwards)"""
    K = len(rois)
    states, pts0 = begin_all(api, frames[0], rois, begins)
    means, ngs, t = [], [], 1
    for form, n in schedule:
        f = frames[t:t + n]
        if form == "multi":
            m, ng = api.multi(states, f, rois, win)
            m, ng = np.array(m, np.float32), np.array(ng, np.int32)
        else:
            m, ng = np.zeros((n, K, 2), np.float32), np.zeros((n, K), np.int32)
            for k in range(K):
                if form == "clip":
                    mk, nk = api.clip(states[k], f, rois[k], win)
                    m[:, k], ng[:, k] = mk, nk
                else:
                    for i in range(n):
                        mk, nk = api.step(states[k], f[i], rois[k], win)
                        m[i, k], ng[i, k] = mk, nk
        means.append(m); ngs.append(ng)
        t += n
    caps = caps or [100] * K
    return dict(states=states, pts0=pts0, mean=np.concatenate(means), n_good=np.concatenate(ngs),
                points=[api.points(states[k], caps[k]) for k in range(K)])


def assert_same(got, want, what=""):
    assert np.array_equal(got["mean"], want["mean"]), ("mean_xy", what)
    assert np.array_equal(got["n_good"], want["n_good"]), ("n_good", what)
    for k, (a, b) in enumerate(zip(got["points"], want["points"])):
        assert np.array_equal(a, b), ("points of subject %d" % k, what)


def assert_same_next_step(api, frame, rois, got, want, what=""):
    """one further rm_flow_step from every state of both runs: the crops, pyramids and points the calls left agree
    (got: one run, or a list of runs that are each compared with `want`)"""
    for k, roi in enumerate(rois):
        b = api.step(want["states"][k], frame, roi)
        for i, g in enumerate(got if isinstance(got, list) else [got]):
            a = api.step(g["states"][k], frame, roi)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], ("next step of subject %d, run %d" % (k, i), what)


def check_alternating_one_subject_clips(api, frames):
    """One-subject rm_flow_clip calls share the chunk workspace of their context: two states with different pyramid depths (1 and 3
    LK levels) advance by alternating calls -- A 3 frames, B 3, A 4, B 4 -- unchunked and with 2 frames per chunk, and each must
    come out as its own 7 rm_flow_step calls: outputs, rm_flow_points and one further step.  frames: 9 of the 80 x 100 frames."""
    rois = [ROIS_EMU[0], ROIS_EMU[2]]
    assert [lk_levels(r[3], r[2]) for r in rois] == [1, 3]
    want = run(api, frames, rois, [("step", 7)])
    assert all(p is not None and len(p) > 0 for p in want["pts0"]) and (want["n_good"][-1] > 0).all()
    runs = []
    for per_chunk in (0, 2):
        states, pts0 = begin_all(api, frames[0], rois)
        mean, n_good = np.zeros((7, 2, 2), np.float32), np.zeros((7, 2), np.int32)
        try:
            for t, n in ((1, 3), (4, 4)):
                for k, roi in enumerate(rois):
                    api.set_bytes(chunk_bytes([roi], per_chunk) if per_chunk else 0)
                    m, ng = api.clip(states[k], frames[t:t + n], roi)
                    mean[t - 1:t - 1 + n, k], n_good[t - 1:t - 1 + n, k] = m, ng
        finally:
            api.set_bytes(0)
        got = dict(states=states, pts0=pts0, mean=mean, n_good=n_good, points=[api.points(st, 100) for st in states])
        assert_same(got, want, ("alternating clips", per_chunk))
        runs.append(got)
    assert_same_next_step(api, frames[8], rois, runs, want, "alternating clips")


def check_pca_windows_multi(api):
    """rm_pca_reduce_windows_multi on lists of 0, 1, 2, 5 and 129 rows, each from first = 0, n // 2 and n, at windows of 128 and 5.  The
    reference is rm_pca_reduce window by window (another kernel); rm_pca_reduce_windows, the K = 1 entry of the same body, beside it.
    -> the lists {n: rows}"""
    rng = np.random.default_rng(12)
    lists = {n: (rng.standard_normal((n, 2)) * rng.uniform(0.01, 2, 2) + rng.uniform(-1, 1, 2)).astype(np.float32) for n in (0, 1, 2, 5, 129)}
    for window in (128, 5):
        rows, firsts = [], []
        for n, md in lists.items():
            for first in (0, n // 2, n):
                rows.append(md); firsts.append(first)
        got = api.pca_multi(rows, firsts, window)
        assert len(got) == len(rows)
        for md, first, g in zip(rows, firsts, got):
            want = np.array([api.pca_one(md[max(0, j + 1 - window):j + 1]) for j in range(first, len(md))])
            assert np.array_equal(g, want, equal_nan=True), (len(md), first, window)
            assert np.array_equal(g, api.pca(md, first, window) if len(md) > first else np.empty(0), equal_nan=True), (len(md), first, window)
        one = api.pca_multi([lists[129]], [3], window)
        want = np.array([api.pca_one(lists[129][max(0, j + 1 - window):j + 1]) for j in range(3, 129)])
        assert len(one) == 1 and np.array_equal(one[0], want) and np.array_equal(one[0], api.pca(lists[129], 3, window))
    return lists


# ---- SubjectTracker('flow') against stand-alone monitors ------------------------------------------------------------------------------
SIGNALS = ("data", "t", "freq", "filtered_data", "peak_indices", "peak_times")


def tracker_frames(n=30, lost_at=20, lost_roi=ROIS_EMU[0]):
    """30 frames; the crop of `lost_roi` is flat in frame `lost_at`, so that subject loses every point there (behind the
    initialisation length of 12 frames: the monitor leaves 'measure' on that frame)"""
    render = synth.synth_texture(80, 100, seed=99)
    f = np.stack([render(1.5 * np.sin(0.5 * t), 0.7 * np.cos(0.4 * t)) for t in range(n)])
    x, y, w, h = lost_roi
    f[lost_at, y:y + h, x:x + w] = 9
    return f


def assert_subject_equals_monitor(sub, points, mon, what=""):
    """the equality contract: signals, motion_data, all_data and the tracked points; NaN objects at the same positions"""
    def arr(v):
        return np.array(v, dtype=np.float64)
    for name in SIGNALS:
        assert np.array_equal(arr(getattr(sub, name)), arr(getattr(mon, name)), equal_nan=True), (name, what)
    assert [v is np.nan for v in sub.data] == [v is np.nan for v in mon.data], what
    assert np.array_equal(np.array(sub.motion_data, np.float32).reshape(-1, 2), np.array(mon.motion_data, np.float32).reshape(-1, 2)), what
    assert len(sub.all_data) == len(mon.all_data) and np.array_equal(arr(sub.all_data), arr(mon.all_data), equal_nan=True), what
    assert sub.lost == (mon.state != 'measure') and sub.error_message == mon.error_message, what
    mp = mon.motion_key_points
    assert (points is None or len(points) == 0) == (mp is None or len(mp) == 0), what
    if mp is not None and len(mp):
        assert np.array_equal(points, mp), what


def step_in_clips(obj, frames, sizes):
    """step_clip over consecutive clips of the given sizes (a monitor stops consuming where it leaves 'measure')"""
    t = 0
    for n in sizes:
        if getattr(obj, "state", "measure") != "measure":
            break
        obj.step_clip(frames[t:t + n])
        t += n


# ---- the instances of the clip driver that the cases above do not select -----------------------------------------------------------
def check_schedule_and_oracle(api, frames, rois, begins, caps, win, n):
    """n frames after frames[0] with the LK window `win`: one rm_flow_multi_clip and the per-subject clips against the rm_flow_step loop,
    bit for bit, and that loop against the oracle's calcOpticalFlowPyrLK on the crops the reference forms (base.py:364-388): the same
    survivors, and the mean of old - new over them, bit for bit.  -> the loop's run"""
    from tests import geometry_cases as gc
    oracle = gc.oracle()
    dev = api.dev(frames)
    steps = run(api, dev, rois, [("step", n)], begins, caps, win)
    assert_same(run(api, dev, rois, [("multi", n)], begins, caps, win), steps, ("multi", win))
    assert_same(run(api, dev, rois, [("clip", n)], begins, caps, win), steps, ("clip", win))
    for k, (x, y, w, h) in enumerate(rois):
        crops = [np.ascontiguousarray(oracle.float_to_uint8(oracle.uint8_to_float(f)[y:y + h, x:x + w])) for f in frames[:n + 1]]
        cur = steps["pts0"][k]
        assert cur is not None and len(cur) > 0, k
        for t in range(1, n + 1):
            r1, rs, _ = oracle.calcOpticalFlowPyrLK(crops[t - 1], crops[t], cur, None, winSize=tuple(win), maxLevel=LVL, criteria=CRIT)
            good = rs.ravel() == 1
            assert steps["n_good"][t - 1, k] == int(good.sum()) and good.any(), (k, t)
            assert np.array_equal(steps["mean"][t - 1, k], np.mean(cur.reshape(-1, 2)[good] - r1.reshape(-1, 2)[good], axis=0)), (k, t)   # base.py:388
            cur = r1[good].reshape(-1, 1, 2)
        assert np.array_equal(np.asarray(steps["points"][k]).reshape(-1, 2), cur.reshape(-1, 2)), k
    return steps


WIDE_WINDOWS = ((17, 17), (21, 21))          # win_w * win_h > 256: the sixteen-pixels-per-lane instance of the clip tracker


def check_wide_window(api, win):
    check_schedule_and_oracle(api, frames_emu(1.0, 5), ROIS_EMU[:3], None, None, win, 4)


MANY = dict(H=440, W=460, begin=(7000, 0.0001, 1, 3), win=(3, 3))      # more points than the LDS staging of the finish holds (FLOW_FINISH_MAX = 6000)


def check_many_points(api):
    """a subject of 7000 points (the sequential finish of rm_flow_step and of rm_flow_multi_clip) beside one of a few"""
    render = synth.synth_texture(MANY["H"], MANY["W"], seed=5)
    frames = np.stack([render(0.7 * np.sin(0.5 * t), 0.3 * np.cos(0.4 * t)) for t in range(3)])
    steps = check_schedule_and_oracle(api, frames, [(0, 0, MANY["W"], MANY["H"]), (10, 10, 24, 20)], [MANY["begin"], BEGIN], [MANY["begin"][0], 100], MANY["win"], 2)
    assert len(steps["pts0"][0]) == MANY["begin"][0] and steps["n_good"][-1, 0] > 6000      # still above the staging after the last step
