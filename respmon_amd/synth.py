"""
Seeded synthetic inputs for tests and bench.py.  numpy only; runs on
both the build container and the GPU box.  Also a fake capture object with the duck type
`run()` needs (reference base.py:48-51, 227-233: isOpened/read/get/release).
"""
import numpy as np

CAP_PROP_FRAME_WIDTH = 3
CAP_PROP_FRAME_HEIGHT = 4
CAP_PROP_FPS = 5


def _lowpass_noise(rng, h, w, cutoff=0.06):
    """Seeded low-pass noise in [-1, 1]."""
    n = rng.standard_normal((h, w))
    fy = np.fft.fftfreq(h)[:, None]
    fx = np.fft.rfftfreq(w)[None, :]
    filt = np.exp(-(fy * fy + fx * fx) / (2 * cutoff * cutoff))
    t = np.fft.irfft2(np.fft.rfft2(n) * filt, s=(h, w))
    t -= t.mean()
    m = np.abs(t).max()
    return t / m if m > 0 else t


def synth_breathing(T, H, W, seed=1234, fps=10.0, breath_hz=0.4, amplitude=0.2, noise=0.02,
                    center=(0.6, 0.4), sigma=(0.10, 0.08), block=8):
    """uint8 [T,H,W] gray video: static low-pass texture + a Gaussian blob whose brightness
    oscillates at `breath_hz` (inside the 0.1-1.0 Hz calibration band) + white noise.
    The blob is off-centre so bounding-box bugs show.  Frames enter the path as
    uint8_to_float(g) like reference base.py:231.  Generated `block` frames at a time to
    bound host memory at 1080p x 256."""
    rng = np.random.Generator(np.random.PCG64(seed))
    tex = _lowpass_noise(rng, H, W)
    yy = (np.arange(H)[:, None] - center[0] * H) / (sigma[0] * H)
    xx = (np.arange(W)[None, :] - center[1] * W) / (sigma[1] * W)
    blob = (amplitude * 255.0 * np.exp(-0.5 * (yy * yy + xx * xx))).astype(np.float32)
    base = (255.0 * (0.5 + 0.25 * tex)).astype(np.float32)
    sig = np.float32(255.0 * noise)
    out = np.empty((T, H, W), dtype=np.uint8)
    for t0 in range(0, T, block):
        t1 = min(T, t0 + block)
        s = np.sin(2 * np.pi * breath_hz * np.arange(t0, t1) / fps).astype(np.float32)[:, None, None]
        g = rng.standard_normal((t1 - t0, H, W), dtype=np.float32)
        g *= sig
        g += base[None]
        g += blob[None] * s
        np.rint(g, out=g)
        np.clip(g, 0, 255, out=g)
        out[t0:t1] = g.astype(np.uint8)
    return out


def synth_breathing16(T, H, W, seed=1234, bits=16, **kw):
    """uint16 [T,H,W] gray video as a 16-bit camera delivers it (Y16): synth_breathing(T, H, W, seed, **kw) in the upper byte and seeded
    uniform noise in the lower one, so that every bit of a sample carries information.  `bits` < 16: the sample of a 10 / 12 / 14-bit
    sensor stored right-aligned in its 16-bit word, i.e. the 16-bit sample shifted down by 16 - bits (shift it up again for the
    left-aligned form: the calibration finds the same ROI either way, include/respmon_hip.h RM_U16)."""
    if not 1 <= bits <= 16:
        raise ValueError("bits must be 1..16, got %r" % (bits,))
    hi = synth_breathing(T, H, W, seed=seed, **kw).astype(np.uint16)
    rng = np.random.Generator(np.random.PCG64([seed, 16]))
    lo = rng.integers(0, 256, size=(T, H, W), dtype=np.uint16)
    return ((hi << 8) | lo) >> np.uint16(16 - bits)


def synth_breathing_blocks(T, H, W, seed=1234, fps=10.0, breath_hz=0.4, amplitude=0.2, noise=0.02,
                           center=(0.6, 0.4), sigma=(0.10, 0.08), block=8, workers=None):
    """The same video model as synth_breathing for the large configurations (4K x 512 is 4.2 G samples): every `block`
    frames draw their noise from their own child generator (SeedSequence(seed).spawn), so blocks are filled by a thread
    pool (numpy releases the GIL) and the result depends only on (T, H, W, seed, block), not on the worker count.
    NOT sample-identical to synth_breathing (one sequential generator there; the goldens use that one)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    rng0 = np.random.Generator(np.random.PCG64(seed))
    tex = _lowpass_noise(rng0, H, W)
    yy = (np.arange(H)[:, None] - center[0] * H) / (sigma[0] * H)
    xx = (np.arange(W)[None, :] - center[1] * W) / (sigma[1] * W)
    blob = (amplitude * 255.0 * np.exp(-0.5 * (yy * yy + xx * xx))).astype(np.float32)
    base = (255.0 * (0.5 + 0.25 * tex)).astype(np.float32)
    sig = np.float32(255.0 * noise)
    out = np.empty((T, H, W), dtype=np.uint8)
    starts = list(range(0, T, block))
    children = np.random.SeedSequence(seed).spawn(len(starts))

    def fill(k):
        t0 = starts[k]
        t1 = min(T, t0 + block)
        rng = np.random.Generator(np.random.PCG64(children[k]))
        s = np.sin(2 * np.pi * breath_hz * np.arange(t0, t1) / fps).astype(np.float32)[:, None, None]
        g = rng.standard_normal((t1 - t0, H, W), dtype=np.float32)
        g *= sig
        g += base[None]
        g += blob[None] * s
        np.rint(g, out=g)
        np.clip(g, 0, 255, out=g)
        out[t0:t1] = g.astype(np.uint8)

    if workers is None:
        workers = max(1, min(32, (os.cpu_count() or 1)))
    with ThreadPoolExecutor(workers) as ex:
        list(ex.map(fill, range(len(starts))))
    return out


def synth_breathing_dense(T, H, W, seed=4321, fps=10.0, breath_hz=0.4, amplitude=0.2, noise=0.06, block=8, workers=None,
                          centers=None, sigma=(0.10, 0.08), phase_step=np.pi / 2):
    """A stream that is hard on the pruning of the collapse passes (bench.py `dense_stream`): FOUR breathing blobs spread
    over the frame, a quarter period apart, and three times the sensor noise of synth_breathing -- low-tail voxels
    of the band-passed video are no longer confined to one corner of the image.  Block-parallel like
    synth_breathing_blocks."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    rng0 = np.random.Generator(np.random.PCG64(seed))
    tex = _lowpass_noise(rng0, H, W)
    if centers is None:
        centers = [(0.25, 0.2), (0.3, 0.75), (0.7, 0.35), (0.75, 0.8)]
    sig_y, sig_x = sigma
    blobs = []
    for (cy, cx) in centers:
        yy = (np.arange(H)[:, None] - cy * H) / (sig_y * H)
        xx = (np.arange(W)[None, :] - cx * W) / (sig_x * W)
        blobs.append((amplitude * 255.0 * np.exp(-0.5 * (yy * yy + xx * xx))).astype(np.float32))
    base = (255.0 * (0.5 + 0.25 * tex)).astype(np.float32)
    sig = np.float32(255.0 * noise)
    out = np.empty((T, H, W), dtype=np.uint8)
    starts = list(range(0, T, block))
    children = np.random.SeedSequence(seed).spawn(len(starts))

    def fill(k):
        t0 = starts[k]
        t1 = min(T, t0 + block)
        rng = np.random.Generator(np.random.PCG64(children[k]))
        g = rng.standard_normal((t1 - t0, H, W), dtype=np.float32)
        g *= sig
        g += base[None]
        for q, blob in enumerate(blobs):
            s = np.sin(2 * np.pi * breath_hz * np.arange(t0, t1) / fps + q * phase_step).astype(np.float32)[:, None, None]
            g += blob[None] * s
        np.rint(g, out=g)
        np.clip(g, 0, 255, out=g)
        out[t0:t1] = g.astype(np.uint8)

    if workers is None:
        workers = max(1, min(32, (os.cpu_count() or 1)))
    with ThreadPoolExecutor(workers) as ex:
        list(ex.map(fill, range(len(starts))))
    return out


def synth_noise_only(T, H, W, seed=777, noise=0.1, workers=None):
    """Worst case of the collapse passes' pruning (bench.py `worst_case`): the static texture plus sensor noise of sigma 0.1 in
    EVERY pixel and no breathing region at all -- low-tail voxels of the band-passed video turn up in every tile."""
    return synth_breathing_dense(T, H, W, seed=seed, noise=noise, workers=workers, centers=[])


def synth_breathing_16(T, H, W, seed=888, noise=0.04, workers=None):
    """Sixteen small breathing blobs on a 4 x 4 lattice, a sixteenth of a period apart, twice the noise of synth_breathing."""
    centers = [((2 * i + 1) / 8.0, (2 * j + 1) / 8.0) for i in range(4) for j in range(4)]
    return synth_breathing_dense(T, H, W, seed=seed, noise=noise, workers=workers, centers=centers, sigma=(0.05, 0.04), phase_step=np.pi / 8)


def synth_brightness_video(T, H, W, fps=10.0, hz=0.4):
    """Config 1: whole-frame brightness 0.5 + 0.2 sin(2 pi hz t / fps), BGR uint8 [T,H,W,3]."""
    t = np.arange(T)
    lvl = np.clip(np.round(255 * (0.5 + 0.2 * np.sin(2 * np.pi * hz * t / fps))), 0, 255).astype(np.uint8)
    return np.broadcast_to(lvl[:, None, None, None], (T, H, W, 3)).copy()


def synth_pulse_bgr(N, H, W, fps=20.0, seed=0, pulse_hz=1.25, flicker_hz=0.9, skin=(110.0, 140.0, 200.0), background=(120.0, 120.0, 120.0),
                    pulse=(0.53, 0.77, 0.33), pulse_depth=0.004, flicker_depth=0.02, noise=1.0):
    """A pulse under a flickering lamp, BGR uint8 [N,H,W,3]: the left half of the frame is skin of colour `skin` (B, G, R) whose channels
    carry the relative pulsatile term pulse_depth * pulse * sin(2 pi pulse_hz t), the right half a gray wall; every pixel is multiplied
    by the lamp's 1 + flicker_depth * sin(2 pi flicker_hz t), Gaussian noise of `noise` levels is added and the result rounded.  The
    flicker is five times the pulse in every channel: a gray or single-channel mean sees the lamp, POS sees the pulse."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / float(fps)
    base = np.empty((H, W, 3))
    base[:, :W // 2] = skin
    base[:, W // 2:] = background
    mod = np.ones((N, 1, W, 3))
    mod[:, :, :W // 2, :] += pulse_depth * np.asarray(pulse, dtype=np.float64)[None, None, None, :] * np.sin(2 * np.pi * pulse_hz * t)[:, None, None, None]
    lamp = 1.0 + flicker_depth * np.sin(2 * np.pi * flicker_hz * t)
    out = np.empty((N, H, W, 3), np.uint8)
    for n in range(N):
        out[n] = np.clip(np.rint(base * mod[n] * lamp[n] + noise * rng.standard_normal((H, W, 3))), 0, 255).astype(np.uint8)
    return out


def synth_texture(H, W, seed=4321, n_waves=12, n_spots=40):
    """Config 3: analytic texture (random 2-D sinusoids + Gaussian spots) as a callable
    f(dx, dy) -> uint8 [H,W] rendered at a sub-pixel shift, so ground-truth flow is known."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kx = rng.uniform(-0.9, 0.9, n_waves)
    ky = rng.uniform(-0.9, 0.9, n_waves)
    ph = rng.uniform(0, 2 * np.pi, n_waves)
    am = rng.uniform(0.3, 1.0, n_waves)
    sx = rng.uniform(0, W, n_spots)
    sy = rng.uniform(0, H, n_spots)
    ss = rng.uniform(1.5, 4.0, n_spots)
    sa = rng.uniform(-1.0, 1.0, n_spots)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def at(x, y):
        """the texture at scene coordinates x, y [H,W] (no resampling: the analytic form is evaluated there)"""
        v = np.zeros((H, W))
        for i in range(n_waves):
            v += am[i] * np.sin(kx[i] * x + ky[i] * y + ph[i])
        v /= max(1.0, am.sum() / 2)
        for i in range(n_spots):
            v += sa[i] * np.exp(-0.5 * ((x - sx[i]) ** 2 + (y - sy[i]) ** 2) / (ss[i] * ss[i]))
        g = 0.5 + 0.22 * v
        return np.clip(np.round(255 * g), 0, 255).astype(np.uint8)

    def render(dx=0.0, dy=0.0):
        return at(xx - dx, yy - dy)

    render.at = at
    return render


def synth_shaky_breathing(T, H, W, jitter, seed=7, fps=10.0, breath_hz=0.4, amplitude=0.04, noise=0.02, center=(0.6, 0.4),
                          sigma=(0.10, 0.08)):
    """A breathing subject seen by a camera that shakes: synth_texture(H, W, seed) plus a Gaussian blob whose brightness oscillates at
    `breath_hz` plus white pixel noise, the whole scene (texture and blob) displaced per frame by a shift drawn uniformly from
    +-`jitter` pixels in x and y.  The first frame is not displaced: it is the frame a stabiliser registers the others to.
    Returns (still, shaken, shifts): the uint8 [T,H,W] clip of the camera at rest, the clip of the shaking camera with the same
    breathing and the same noise, and the true shifts [T,2] (dx, dy) of the scene content, positive toward +x / +y."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x5ab1]))
    render = synth_texture(H, W, seed=seed)
    shifts = rng.uniform(-jitter, jitter, size=(T, 2))
    shifts[0] = 0.0
    s = np.sin(2 * np.pi * breath_hz * np.arange(T) / fps)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def blob(dx, dy):
        y = (yy - dy - center[0] * H) / (sigma[0] * H)
        x = (xx - dx - center[1] * W) / (sigma[1] * W)
        return amplitude * np.exp(-0.5 * (y * y + x * x))

    still, shaken = np.empty((T, H, W), np.uint8), np.empty((T, H, W), np.uint8)
    base0, blob0 = render(0.0, 0.0) / 255.0, blob(0.0, 0.0)
    for t in range(T):
        n = noise * rng.standard_normal((H, W))
        still[t] = np.clip(np.rint(255 * (base0 + blob0 * s[t] + n)), 0, 255).astype(np.uint8)
        dx, dy = shifts[t]
        shaken[t] = np.clip(np.rint(255 * (render(dx, dy) / 255.0 + blob(dx, dy) * s[t] + n)), 0, 255).astype(np.uint8)
    return still, shaken, shifts


def similarity_params(theta_deg, scale, tx, ty):
    """[N,4] (p0, p1, tx, ty) of rm_stab_sim_* (include/respmon_hip.h): p0 = s cos(theta) - 1, p1 = s sin(theta)"""
    th = np.deg2rad(np.asarray(theta_deg, dtype=np.float64))
    s = np.asarray(scale, dtype=np.float64)
    return np.stack(np.broadcast_arrays(s * np.cos(th) - 1.0, s * np.sin(th), np.asarray(tx, dtype=np.float64), np.asarray(ty, dtype=np.float64)), axis=-1)


def similarity_scene_coords(H, W, p):
    """The scene coordinates (x, y) [H,W] that a camera moved by p = (p0, p1, tx, ty) shows at its pixels: the inverse of
    fx = cx + ((1 + p0) u - p1 v) + tx, fy = cy + (p1 u + (1 + p0) v) + ty with u = x - cx, v = y - cy, cx = (W - 1) / 2, cy = (H - 1) / 2."""
    cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a, b = 1.0 + p[0], p[1]
    X, Y = xx - cx - p[2], yy - cy - p[3]
    n = a * a + b * b
    return cx + (a * X + b * Y) / n, cy + (a * Y - b * X) / n


def synth_shaky_breathing_similarity(T, H, W, jitter, rot_deg, zoom, seed=7, fps=10.0, breath_hz=0.4, amplitude=0.04, noise=0.02, center=(0.6, 0.4),
                                     sigma=(0.10, 0.08)):
    """synth_shaky_breathing seen by a hand-held camera: per frame the whole scene (texture and blob) is rolled about the frame's centre by
    an angle uniform in +-`rot_deg` degrees, zoomed by a factor uniform in 1 +- `zoom` and displaced by a shift uniform in +-`jitter`
    pixels.  The analytic texture and the blob are evaluated at the inverse-transformed coordinates, exactly: nothing is resampled.  The
    first frame is not moved.  Returns (still, shaken, params): the uint8 [T,H,W] clip of the camera at rest, the clip of the moving
    camera with the same breathing and the same noise, and the true parameters [T,4] (p0, p1, tx, ty) of rm_stab_sim_*."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x51a1]))
    render = synth_texture(H, W, seed=seed)
    params = similarity_params(rng.uniform(-rot_deg, rot_deg, T), rng.uniform(1.0 - zoom, 1.0 + zoom, T), rng.uniform(-jitter, jitter, T),
                               rng.uniform(-jitter, jitter, T))
    params[0] = 0.0
    s = np.sin(2 * np.pi * breath_hz * np.arange(T) / fps)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def blob(x, y):
        by = (y - center[0] * H) / (sigma[0] * H)
        bx = (x - center[1] * W) / (sigma[1] * W)
        return amplitude * np.exp(-0.5 * (by * by + bx * bx))

    still, shaken = np.empty((T, H, W), np.uint8), np.empty((T, H, W), np.uint8)
    base0, blob0 = render.at(xx, yy) / 255.0, blob(xx, yy)
    for t in range(T):
        n = noise * rng.standard_normal((H, W))
        still[t] = np.clip(np.rint(255 * (base0 + blob0 * s[t] + n)), 0, 255).astype(np.uint8)
        x, y = (xx, yy) if t == 0 else similarity_scene_coords(H, W, params[t])
        shaken[t] = np.clip(np.rint(255 * (render.at(x, y) / 255.0 + blob(x, y) * s[t] + n)), 0, 255).astype(np.uint8)
    return still, shaken, params


class FakeCapture:
    """Stands in for cv2.VideoCapture (reference base.py:48-51, 227-233).
    frames: uint8 [T,H,W,3] BGR (or [T,H,W] gray, returned as 3 equal channels); uint16 [T,H,W] frames are returned as they are, 2-D,
    as a Y16 capture with CAP_PROP_CONVERT_RGB off delivers them."""

    def __init__(self, frames, fps=10):
        self._frames = frames
        self._i = 0
        self._fps = fps
        self._open = True

    def isOpened(self):
        return self._open

    def get(self, prop):
        f = self._frames
        if prop == CAP_PROP_FPS:
            return float(self._fps)
        if prop == CAP_PROP_FRAME_WIDTH:
            return float(f.shape[2])
        if prop == CAP_PROP_FRAME_HEIGHT:
            return float(f.shape[1])
        return 0.0

    def read(self):
        if self._i >= len(self._frames):
            return False, None
        f = self._frames[self._i]
        self._i += 1
        if f.ndim == 2 and f.dtype != np.uint16:
            f = np.repeat(f[:, :, None], 3, axis=2)
        return True, f

    def release(self):
        self._open = False
