// respmon_amd/csrc/rm_window.hip -- rm_window_*: the calibration on a sliding window.  A ring of per-frame pyramid rows takes the
// place of the resident [T,H,W] buffer of base.py:409-513: every camera frame goes through the frame-buffer kernel once, and the ROI
// is taken from the ring at any moment -- no refill after a reset.
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_internal.h"

using namespace rm;

// The ring holds what front_pyramid writes for a frame (G_S, or the Laplacian levels S .. L-2: PyrGeom::NP doubles), float64 whatever
// the frames were.  Frame j of the stream (counted from the last reset) sits in row j mod T, so with `count` frames held the oldest
// one is row `head` (0 until the ring is full) and the next one goes to row (head + count) mod T.  The temporal kernels read the
// chronological window in place (rm_temporal_kernels.h ring_row); nothing behind them knows about the ring.
struct rm_window {
    int device = 0;
    int T = 0, H = 0, W = 0, levels = 0, skip = 0;
    unsigned flags = 0;
    PyrGeom pg;
    size_t NP = 0;            // 0: nothing is filtered (skip >= levels - 1), no ring
    double *ring = nullptr;   // [T, NP], its own allocation: it has to survive every other call on the context
    int count = 0, head = 0;
};

extern "C" int rm_window_create(rm_ctx *ctx, int T, int H, int W, int levels, int skip, unsigned flags, rm_window **out)
{
    if (out) *out = nullptr;
    if (!ctx || !out || T < 1 || H < 1 || W < 1 || levels < 1 || skip < 1)
        return fail(RM_E_BADARG, "rm_window_create: bad argument (a window needs skip_levels_at_top >= 1)");
    if (T > MAX_T) return fail(RM_E_UNSUPPORTED, "rm_window_create: T=%d > %d", T, MAX_T);
    HIP_TRY(hipSetDevice(ctx->device));
    rm_window *w = new rm_window;
    w->device = ctx->device;
    w->T = T; w->H = H; w->W = W; w->levels = levels; w->skip = skip; w->flags = flags;
    pyr_geom(H, W, levels, skip, flags, w->pg);
    w->NP = w->pg.all_zero ? 0 : w->pg.NP;
    if (w->NP) {
        hipError_t e = hipMalloc((void **)&w->ring, sizeof(double) * (size_t)T * w->NP);
        if (e != hipSuccess) {
            delete w;
            return fail(RM_E_HIP, "rm_window_create: %zu bytes for the ring: %s", sizeof(double) * (size_t)T * w->NP, hipGetErrorString(e));
        }
    }
    *out = w;
    return RM_OK;
}

extern "C" int rm_window_destroy(rm_window *w)
{
    if (!w) return RM_OK;
    (void)hipSetDevice(w->device);
    if (w->ring) (void)hipFree(w->ring);   // (synchronises with the work that still reads the ring)
    delete w;
    return RM_OK;
}

extern "C" int rm_window_reset(rm_ctx *ctx, rm_window *w)
{
    if (!ctx || !w) return fail(RM_E_BADARG, "rm_window_reset: bad argument");
    w->count = 0; w->head = 0;   // the rows stay where they are: each is written again before it is read
    return RM_OK;
}

extern "C" int rm_window_info(const rm_window *w, int *count, int *head, size_t *np, size_t *ring_bytes)
{
    if (!w) return fail(RM_E_BADARG, "rm_window_info: bad argument");
    if (count) *count = w->count;
    if (head) *head = w->head;
    if (np) *np = w->NP;
    if (ring_bytes) *ring_bytes = sizeof(double) * (size_t)w->T * w->NP;
    return RM_OK;
}

extern "C" int rm_window_push(rm_ctx *ctx, rm_window *w, const void *frames, int dtype, int n, void *stream)
{
    if (!ctx || !w || !frames || n < 1 || !valid_buffer_dtype(dtype)) return fail(RM_E_BADARG, "rm_window_push: bad argument");
    if (ctx->device != w->device) return fail(RM_E_BADARG, "rm_window_push: the window belongs to device %d", w->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    const int T = w->T;
    const int next = (w->head + w->count) % T;        // row of the first frame of this call (== head once the ring is full)
    const int drop = n > T ? n - T : 0;               // frames of the call the ring would not hold at its end: never reduced
    const int keep = n - drop;
    if (w->NP) {
        const size_t frame_bytes = (size_t)w->H * w->W * dtype_size(dtype);
        const uint8_t *src = (const uint8_t *)frames + (size_t)drop * frame_bytes;
        const int row0 = (int)(((long long)next + drop) % T);
        const int n0 = std::min(keep, T - row0);      // up to the ring's end, then from row 0: two launches of the frame-buffer kernel
        RM_TRY(front_pyramid(ctx, src, dtype, n0, w->H, w->W, w->pg, w->flags, w->ring + (size_t)row0 * w->NP, s));
        if (keep > n0)
            RM_TRY(front_pyramid(ctx, src + (size_t)n0 * frame_bytes, dtype, keep - n0, w->H, w->W, w->pg, w->flags, w->ring, s));
    }
    if ((long long)w->count + n >= T) { w->head = (int)(((long long)next + n) % T); w->count = T; }
    else w->count += n;
    return RM_OK;
}

// frames held -> heatmap, through the stages rm_shard_collapse / rm_shard_heat run with one rank (front_filter, collapse_eval on
// ctx->shard_plan, collapse_sum); the time average and the heatmap extrema ride the sum kernel, as in rm_calibrate
static int window_heat(rm_ctx *ctx, rm_window *w, double fps, double fmin, double fmax, double amp, double thr, double *heat, hipStream_t s,
                       const char *who)
{
    if (!w || !heat || !(fps > 0)) return fail(RM_E_BADARG, "%s: bad argument", who);
    if (w->count < 1) return fail(RM_E_BADARG, "%s: the window holds no frame", who);
    if (ctx->device != w->device) return fail(RM_E_BADARG, "%s: the window belongs to device %d", who, w->device);
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, (void *)s, who));
    const int m = w->count;   // < T: rows 0 .. m-1 in order (head == 0), the operator is the one of m frames
    CollapsePlan &cp = ctx->shard_plan;
    cp.valid = false;
    ctx->nkept_H = ctx->nkept_W = 0;
    if (ctx->prof_on) ctx->prof_calls++;
    if (!w->NP) return zero_result(ctx, (size_t)w->H * w->W, heat, nullptr, s);
    ctx->state_fresh = false;   // whatever ran on the context since the push may have reduced into d_state
    SmallLevels sl;
    RM_TRY(front_filter(ctx, w->ring, m, w->pg, fps, fmin, fmax, amp, sl, s, w->head));
    RM_TRY(collapse_eval(ctx, sl, m, 0, m, thr, w->flags, cp, s));
    return collapse_sum(ctx, cp, thr, heat, s, m);
}

extern "C" int rm_window_calibrate(rm_ctx *ctx, rm_window *w, double fps, double fmin, double fmax, double amp, double thr, double *heat,
                                   void *stream)
{
    if (!ctx) return fail(RM_E_BADARG, "rm_window_calibrate: bad argument");
    return window_heat(ctx, w, fps, fmin, fmax, amp, thr, heat, (hipStream_t)stream, "rm_window_calibrate");
}

extern "C" int rm_window_locate(rm_ctx *ctx, rm_window *w, double fps, double fmin, double fmax, double amp, double thr, int threshold,
                                int32_t *xywh, void *stream)
{
    if (!ctx || !w || !xywh) return fail(RM_E_BADARG, "rm_window_locate: bad argument");
    ctx->cur_slot = 0;
    double *heat = nullptr;
    RM_TRY(ws(ctx, "heat", (size_t)w->H * w->W, &heat));
    RM_TRY(window_heat(ctx, w, fps, fmin, fmax, amp, thr, heat, (hipStream_t)stream, "rm_window_locate"));
    const CollapsePlan &cp = ctx->shard_plan;
    ctx->clip_frame_once = (w->flags & RM_FLAG_CONTOUR_CLIP_FRAME) != 0;
    ctx->tiles_const_once = cp.valid && cp.S >= 1;
    return heatmap_to_roi_impl(ctx, heat, w->H, w->W, threshold, xywh, nullptr, nullptr, stream, true);
}

extern "C" int rm_window_locate_multi(rm_ctx *ctx, rm_window *w, double fps, double fmin, double fmax, double amp, double thr, int threshold,
                                      int max_rois, double min_area, int32_t *xywh, double *area, int *n_out, void *stream)
{
    if (n_out) *n_out = 0;
    if (!ctx || !w || !xywh || !n_out || max_rois < 1 || max_rois > RM_MAX_ROIS || !(min_area >= 0.0))
        return fail(RM_E_BADARG, "rm_window_locate_multi: bad argument (1 <= max_rois <= %d, min_area >= 0)", RM_MAX_ROIS);
    double *heat = nullptr;
    RM_TRY(ws(ctx, "heat", (size_t)w->H * w->W, &heat));
    RM_TRY(window_heat(ctx, w, fps, fmin, fmax, amp, thr, heat, (hipStream_t)stream, "rm_window_locate_multi"));
    return heatmap_to_rois_impl(ctx, heat, w->H, w->W, threshold, (w->flags & RM_FLAG_CONTOUR_CLIP_FRAME) != 0, max_rois, min_area, xywh, area,
                                n_out, stream, "rm_window_locate_multi");
}

// the rate map of the frames held (rm_rate.hip rate_peak), read from the ring in place: possible where a row IS G_skip of its frame
extern "C" int rm_window_rate_map(rm_ctx *ctx, rm_window *w, double fps, double fmin, double fmax, int nfreq, double *freq, double *power,
                                  double *total, int32_t *index, void *stream)
{
    if (!ctx || !w) return fail(RM_E_BADARG, "rm_window_rate_map: bad argument");
    if (ctx->device != w->device) return fail(RM_E_BADARG, "rm_window_rate_map: the window belongs to device %d", w->device);
    if (w->count < 2) return fail(RM_E_BADARG, "rm_window_rate_map: the window holds %d frame(s), a rate needs two", w->count);
    if (!w->NP || !(w->pg.filter_first || w->pg.ff_levels))
        return fail(RM_E_UNSUPPORTED, "rm_window_rate_map: the rows of this window are not the Gaussian level %d (Laplacian levels: flags, or its geometry)",
                    w->skip);
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    return rate_peak(ctx, w->ring, w->count, w->NP, w->head, fps, fmin, fmax, nfreq, freq, power, total, index, (hipStream_t)stream,
                     "rm_window_rate_map");
}

extern "C" int rm_debug_window_rows(rm_ctx *ctx, const rm_window *w, int row0, int nrows, double *out_host, void *stream)
{
    if (!ctx || !w || !out_host || row0 < 0 || nrows < 0 || row0 + nrows > w->T) return fail(RM_E_BADARG, "rm_debug_window_rows: bad argument");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    if (w->NP && nrows)
        HIP_TRY(hipMemcpyAsync(out_host, w->ring + (size_t)row0 * w->NP, sizeof(double) * (size_t)nrows * w->NP, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));
    return RM_OK;
}
