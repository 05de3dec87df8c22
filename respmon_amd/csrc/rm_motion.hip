// respmon_amd/csrc/rm_motion.hip -- ROI reductions and motion extraction (base.py:354-407), for one subject and for several
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_internal.h"
#include "rm_roi_kernels.h"
#include "rm_subjects.h"
#include "rm_flow_multi.h"

using namespace rm;

// ------------------------------------------------------------------------------------------
// ROI reductions (base.py:355-358, 364)
// ------------------------------------------------------------------------------------------
static bool roi_ok(int H, int W, int x, int y, int w, int h) { return x >= 0 && y >= 0 && w >= 1 && h >= 1 && x + w <= W && y + h <= H; }

extern "C" int rm_roi_mean(rm_ctx *ctx, const void *frame, int dtype, int H, int W, int x, int y, int w, int h, double *out,
                           void *stream)
{
    if (!ctx || !frame || !out || !valid_dtype(dtype) || !roi_ok(H, W, x, y, w, h)) return fail(RM_E_BADARG, "rm_roi_mean: bad argument");
    hipStream_t s = (hipStream_t)stream;
    double *d = nullptr;
    RM_TRY(ws(ctx, "roi_mean", 1, &d));
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_roi_mean<T>), dim3(1), dim3(256), 0, s, (const T *)frame, W, x, y, w, h, d);
    });
    LAUNCH_CHECK();
    HIP_TRY(hipMemcpyAsync(out, d, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));
    return RM_OK;
}

extern "C" int rm_roi_to_uint8(rm_ctx *ctx, const void *frame, int dtype, int H, int W, int x, int y, int w, int h, uint8_t *dst,
                               void *stream)
{
    if (!ctx || !frame || !dst || !valid_dtype(dtype) || !roi_ok(H, W, x, y, w, h)) return fail(RM_E_BADARG, "rm_roi_to_uint8: bad argument");
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(nblk((size_t)w * h, 256, 1024)), block(256);
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_roi_to_u8<T>), grid, block, 0, s, (const T *)frame, W, x, y, w, h, dst);
    });
    LAUNCH_CHECK();
    return RM_OK;
}

// ------------------------------------------------------------------------------------------
// optical-flow path (rm_flow.h)
// ------------------------------------------------------------------------------------------
extern "C" int rm_good_features_to_track(rm_ctx *ctx, const uint8_t *img, int h, int w, int max_corners, double quality,
                                         double min_distance, int block_size, float *pts, int *n, void *stream)
{
    if (!ctx || !img || !pts || !n || h < 1 || w < 1 || block_size < 1 || (block_size & 1) == 0)
        return fail(RM_E_BADARG, "rm_good_features_to_track: bad argument");
    // the local-maximum test excludes the 1-pixel frame, so an image under 3 pixels in either direction has no corners
    // (OpenCV: "no corners", base.py:367 then reports "No motion key points found.")
    if (h < 3 || w < 3) { *n = 0; return RM_OK; }
    std::string err;
    int rc = flow_good_features(ctx->flow, img, h, w, max_corners, quality, min_distance, block_size, pts, n, (hipStream_t)stream, err);
    if (rc < 0) return fail(rc, "%s", err.c_str());
    return rc;
}

extern "C" int rm_calc_optical_flow_pyr_lk(rm_ctx *ctx, const uint8_t *prev, const uint8_t *next, int h, int w, const float *pts_in,
                                           int npts, int win_w, int win_h, int max_level, int max_count, double epsilon,
                                           float *pts_out, uint8_t *status, void *stream)
{
    if (!ctx || !prev || !next || !pts_in || !pts_out || !status || h < 1 || w < 1 || npts < 0 || win_w < 3 || win_h < 3 || max_level < 0)
        return fail(RM_E_BADARG, "rm_calc_optical_flow_pyr_lk: bad argument");
    std::string err;
    int rc = flow_pyr_lk(ctx->flow, prev, next, h, w, pts_in, npts, win_w, win_h, max_level, max_count, epsilon, pts_out, status,
                         (hipStream_t)stream, err);
    if (rc < 0) return fail(rc, "%s", err.c_str());
    return rc;
}

extern "C" int rm_mean_flow(rm_ctx *ctx, const float *old_pts, const float *new_pts, const uint8_t *status, int npts, float *mean_xy,
                            int *n_good, void *stream)
{
    if (!ctx || !old_pts || !new_pts || !status || !mean_xy || !n_good || npts < 0) return fail(RM_E_BADARG, "rm_mean_flow: bad argument");
    std::string err;
    int rc = flow_mean(ctx->flow, old_pts, new_pts, status, npts, mean_xy, n_good, (hipStream_t)stream, err);
    if (rc < 0) return fail(rc, "%s", err.c_str());
    return rc;
}

extern "C" int rm_pca_reduce(rm_ctx *ctx, const float *motion, int n, double *out, void *stream)
{
    if (!ctx || !motion || !out || n < 0) return fail(RM_E_BADARG, "rm_pca_reduce: bad argument");
    std::string err;
    int rc = flow_pca(ctx->flow, motion, n, out, (hipStream_t)stream, err);
    if (rc < 0) return fail(rc, "%s", err.c_str());
    return rc;
}

// ---- one C-ABI call per frame of extract_motion('flow') (base.py:363-388); crops and points stay on the device ----------
static int flow_crop(rm_ctx *ctx, const void *frame, int dtype, int H, int W, int x, int y, int w, int h, uint8_t *dst, hipStream_t s)
{
    return rm_roi_to_uint8(ctx, frame, dtype, H, W, x, y, w, h, dst, (void *)s);
}

struct rm_flow_state {
    int device = 0;
    FlowState fs;
};

extern "C" int rm_flow_state_create(rm_ctx *ctx, rm_flow_state **out)
{
    if (!ctx || !out) return fail(RM_E_BADARG, "rm_flow_state_create: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    rm_flow_state *st = new rm_flow_state();
    st->device = ctx->device;
    *out = st;
    return RM_OK;
}

extern "C" int rm_flow_state_destroy(rm_flow_state *st)
{
    if (!st) return RM_OK;
    (void)hipSetDevice(st->device);
    delete st;   // (FlowState / FlowWorkspace release their device and pinned memory)
    return RM_OK;
}

// a named buffer of a flow workspace, or the workspace's error as the call's
template <typename T> static int flow_buf(FlowWorkspace &ws, const std::string &name, size_t bytes, T **out)
{
    std::string err;
    const int rc = ws.get(name, bytes, (void **)out, err);
    return rc < 0 ? fail(rc, "%s", err.c_str()) : RM_OK;
}

static int flow_state_pts(FlowState &fs, float **pts_a, float **pts_b)
{
    RM_TRY(flow_buf(fs.ws, "pts_a", sizeof(float) * 2 * (size_t)fs.cap, pts_a));
    return flow_buf(fs.ws, "pts_b", sizeof(float) * 2 * (size_t)fs.cap, pts_b);
}

// level `level` of the pyramid of one side of a state (level 0: the crop itself)
static int flow_state_pyr(FlowState &fs, int side, int level, size_t bytes, uint8_t **out)
{
    std::string err;
    const int rc = flow_side_buf(fs, side, "pyr", level, bytes, (void **)out, err);
    return rc < 0 ? fail(rc, "%s", err.c_str()) : RM_OK;
}
static int flow_state_crop(FlowState &fs, int side, uint8_t **crop) { return flow_state_pyr(fs, side, 0, (size_t)fs.w * fs.h, crop); }

extern "C" int rm_flow_begin(rm_ctx *ctx, rm_flow_state *state, const void *frame, int dtype, int H, int W, int x, int y, int w, int h, int max_corners,
                             double quality, double min_distance, int block_size, float *pts_host, int *n_host, void *stream)
{
    if (!ctx || !state || !frame || !pts_host || !n_host || !valid_dtype(dtype) || !roi_ok(H, W, x, y, w, h) || block_size < 1 ||
        (block_size & 1) == 0)
        return fail(RM_E_BADARG, "rm_flow_begin: bad argument");
    if (state->device != ctx->device) return fail(RM_E_BADARG, "rm_flow_begin: the flow state belongs to device %d, the context to %d", state->device, ctx->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    FlowState &fs = state->fs;
    // (max_corners <= 0: no limit, as in OpenCV -- at most one corner per pixel)
    fs.w = w; fs.h = h; fs.cap = max_corners > 0 ? max_corners : w * h; fs.flip = 0; fs.npts = 0; fs.begun = false;
    fs.pyr_levels[0] = fs.pyr_levels[1] = -1; fs.deriv_levels[0] = fs.deriv_levels[1] = -1;
    if (!fs.res) HIP_TRY(hipHostMalloc((void **)&fs.res, 4 * sizeof(float), hipHostMallocDefault));
    uint8_t *crop = nullptr; float *pa = nullptr, *pb = nullptr;
    RM_TRY(flow_state_crop(fs, 0, &crop));
    RM_TRY(flow_state_pts(fs, &pa, &pb));
    RM_TRY(flow_crop(ctx, frame, dtype, H, W, x, y, w, h, crop, s));
    fs.pyr_levels[0] = 0;
    *n_host = 0;
    if (h >= 3 && w >= 3) {   // (narrower crops have no corners: rm_good_features_to_track)
        std::string err;
        int rc = flow_good_features(fs.ws, crop, h, w, max_corners, quality, min_distance, block_size, pts_host, n_host, s, err);
        if (rc < 0) return fail(rc, "%s", err.c_str());
    }
    fs.npts = *n_host;
    if (*n_host > 0) {
        HIP_TRY(hipMemcpyAsync(pa, pts_host, sizeof(float) * 2 * (size_t)*n_host, hipMemcpyHostToDevice, s));
        HIP_TRY(stream_wait(s));   // pts_host is the caller's again
    }
    fs.begun = true;
    return RM_OK;
}

extern "C" int rm_flow_step(rm_ctx *ctx, rm_flow_state *state, const void *frame, int dtype, int H, int W, int x, int y, int w, int h, int win_w,
                            int win_h, int max_level, int max_count, double epsilon, float *mean_xy_host, int *n_good_host, void *stream)
{
    if (!ctx || !state || !frame || !mean_xy_host || !n_good_host || !valid_dtype(dtype) || !roi_ok(H, W, x, y, w, h) || win_w < 3 || win_h < 3 ||
        max_level < 0)
        return fail(RM_E_BADARG, "rm_flow_step: bad argument");
    FlowState &fs = state->fs;
    if (!fs.begun || w != fs.w || h != fs.h) return fail(RM_E_BADARG, "rm_flow_step: rm_flow_begin has not been called on this state for this ROI size");
    if (state->device != ctx->device) return fail(RM_E_BADARG, "rm_flow_step: the flow state belongs to another device");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    const int prev_side = fs.flip, cur_side = fs.flip ^ 1;
    uint8_t *cur = nullptr; float *pa = nullptr, *pb = nullptr;
    RM_TRY(flow_state_crop(fs, cur_side, &cur));
    RM_TRY(flow_state_pts(fs, &pa, &pb));
    float *pts = fs.flip ? pb : pa, *pts_next = fs.flip ? pa : pb;
    RM_TRY(flow_crop(ctx, frame, dtype, H, W, x, y, w, h, cur, s));
    fs.pyr_levels[cur_side] = 0; fs.deriv_levels[cur_side] = -1;   // a new image on this side: its old pyramid and derivatives are void
    const int npts = fs.npts;
    mean_xy_host[0] = mean_xy_host[1] = 0.f; *n_good_host = 0;
    if (npts > 0) {
        std::string err;
        float *d_out = nullptr; uint8_t *d_st = nullptr; float *dev_res = nullptr;
        RM_TRY(flow_buf(fs.ws, "lk_pts_out", sizeof(float) * 2 * (size_t)npts, &d_out));
        RM_TRY(flow_buf(fs.ws, "lk_status", (size_t)npts, &d_st));
        const int rc = flow_track_resident(fs, prev_side, cur_side, pts, npts, win_w, win_h, max_level, max_count, epsilon, d_out, d_st, s, err);
        if (rc < 0) return fail(rc, "%s", err.c_str());
        HIP_TRY(hipHostGetDevicePointer((void **)&dev_res, fs.res, 0));
        if (npts <= FLOW_FINISH_MAX) hipLaunchKernelGGL(k_flow_finish<>, dim3(1), dim3(64), 2 * sizeof(float) * (size_t)flow_finish_pitch(npts), s, pts, d_out, d_st, npts, dev_res, pts_next);
        else hipLaunchKernelGGL(k_flow_finish_seq<>, dim3(1), dim3(1), 0, s, pts, d_out, d_st, npts, dev_res, pts_next);
        LAUNCH_CHECK();
        HIP_TRY(stream_wait(s));
        mean_xy_host[0] = fs.res[0]; mean_xy_host[1] = fs.res[1]; *n_good_host = (int)fs.res[2];
        fs.npts = *n_good_host;
    }
    fs.flip ^= 1;   // the crop just made is the next call's previous image, the packed points its input (base.py:381-382)
    return RM_OK;
}

extern "C" int rm_flow_points(rm_ctx *ctx, rm_flow_state *state, float *pts_host, int cap, int *n_host, void *stream)
{
    if (!ctx || !state || !n_host || cap < 0 || (cap > 0 && !pts_host)) return fail(RM_E_BADARG, "rm_flow_points: bad argument");
    FlowState &fs = state->fs;
    *n_host = fs.npts;
    if (fs.npts == 0 || cap == 0) return RM_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    float *pa = nullptr, *pb = nullptr;
    RM_TRY(flow_state_pts(fs, &pa, &pb));
    const int n = std::min(cap, fs.npts);
    HIP_TRY(hipMemcpyAsync(pts_host, fs.flip ? pb : pa, sizeof(float) * 2 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));
    return RM_OK;
}

// ------------------------------------------------------------------------------------------
// a whole resident clip per call: one host synchronisation, launches that do not grow with the number of frames
// ------------------------------------------------------------------------------------------
extern "C" int rm_roi_mean_clip(rm_ctx *ctx, const void *frames, int dtype, int N, int H, int W, int x, int y, int w, int h, double *out,
                                void *stream)
{
    if (!ctx || !frames || !out || N < 1 || !valid_dtype(dtype) || !roi_ok(H, W, x, y, w, h)) return fail(RM_E_BADARG, "rm_roi_mean_clip: bad argument");
    hipStream_t s = (hipStream_t)stream;
    double *d = nullptr;
    RM_TRY(ws(ctx, "roi_mean_clip", (size_t)N, &d));
    const size_t px = (size_t)H * W;
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_roi_mean_clip<T>), dim3(N), dim3(256), 0, s, (const T *)frames, px, W, x, y, w, h, d);
    });
    LAUNCH_CHECK();
    HIP_TRY(hipMemcpyAsync(out, d, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));
    return RM_OK;
}

// ... for K rectangles at once (several subjects in one frame): one launch over the (frame, rectangle) pairs, one result copy, one wait
extern "C" int rm_roi_mean_multi_clip(rm_ctx *ctx, const void *frames, int dtype, int N, int H, int W, const int32_t *rois, int K, double *out,
                                      void *stream)
{
    if (!ctx || !frames || !rois || !out || N < 1 || H < 1 || W < 1 || K < 1 || K > RM_MAX_ROIS || !valid_dtype(dtype) ||
        (long long)N * K > 0x7fffffffll)
        return fail(RM_E_BADARG, "rm_roi_mean_multi_clip: bad argument (1 <= K <= %d)", RM_MAX_ROIS);
    for (int k = 0; k < K; ++k)   // the whole call is refused before anything is enqueued
        if (!roi_ok(H, W, rois[4 * k], rois[4 * k + 1], rois[4 * k + 2], rois[4 * k + 3]))
            return fail(RM_E_BADARG, "rm_roi_mean_multi_clip: rectangle %d (%d, %d, %d, %d) does not lie inside the %d x %d frame", k, rois[4 * k],
                        rois[4 * k + 1], rois[4 * k + 2], rois[4 * k + 3], W, H);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    double *d = nullptr;
    int *d_rois = nullptr;
    RM_TRY(ws(ctx, "roi_mean_multi", (size_t)N * K, &d));
    RM_TRY(ws(ctx, "roi_mean_multi_rois", (size_t)4 * RM_MAX_ROIS, &d_rois));
    HIP_TRY(hipMemcpyAsync(d_rois, rois, sizeof(int32_t) * 4 * (size_t)K, hipMemcpyHostToDevice, s));
    const size_t px = (size_t)H * W;
    const dim3 grid((unsigned)(N * K)), block(256);
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_roi_mean_multi_clip<T>), grid, block, 0, s, (const T *)frames, px, W, (const int *)d_rois, K, d);
    });
    LAUNCH_CHECK();
    HIP_TRY(hipMemcpyAsync(out, d, sizeof(double) * (size_t)N * K, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));   // (the rectangles' host memory is the caller's again as well)
    return RM_OK;
}

// ------------------------------------------------------------------------------------------
// optical flow and windowed PCA over a clip (rm_flow_multi.h): one path for K subjects, the one-subject entry points are its K == 1
// ------------------------------------------------------------------------------------------
constexpr long long FLOW_CLIP_BYTES = 256ll << 20;   // workspace cap of one chunk's crops, pyramids and derivatives (rm_debug_set flow_clip_bytes)
constexpr int FLOW_CLIP_MAX_CHUNK = 32768;           // frames per chunk at most: the image index is a grid's y dimension

static int flow_multi_crop(const void *frames, int dtype, int n, int H, int W, const FlowSubject *tab, int nsub, size_t max_px, hipStream_t s)
{
    const size_t px = (size_t)H * W;
    const dim3 grid(nblk(max_px, 256, 1024), (unsigned)n, (unsigned)nsub);
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_flow_multi_crop<T>), grid, dim3(256), 0, s, (const T *)frames, px, W, tab);
    });
    LAUNCH_CHECK();
    return RM_OK;
}

// N successive rm_flow_step calls per subject as one call, subject k on states[k] with rectangle k.  The entry point has checked the
// arguments; `who` is its name for the UNSUPPORTED texts, which then name the subject as well, or NULL for the one-subject entry,
// whose texts are rm_flow_step's and name neither.  The clip is worked through in chunks of C frames.  The subjects that still have
// points ("live") share the chunks of one clip walk: one chunk length C for all, their images (the chunk's frames behind image 0, the
// crop the chunk tracks from) and derivatives in two arenas of the context, their points side by side under one global index (pt0 =
// prefix sum); a point keeps its index through all chunks, its position and life going from one chunk's tracker to the next through
// carry buffers of the whole call.  A subject without points only gets the crop of the clip's last frame (one extra launch for all
// of them).  Launches per chunk: 1 crop + (levels - 1) pyrDown + levels Scharr + 1 tracker + 1 or 2 finish (+ 1 carry).
static int flow_clips(rm_ctx *ctx, const char *who, rm_flow_state *const *states, const void *frames, int dtype, int N, int H, int W, const int32_t *rois,
                      int K, int win_w, int win_h, int max_level, int max_count, double epsilon, float *mean_xy_host, int32_t *n_good_host, hipStream_t s)
{
    // the limits rm_flow_step meets in its tracking stage, which a state without points never reaches: still nothing is enqueued
    for (int k = 0; k < K; ++k) {
        if (states[k]->fs.npts == 0) continue;
        const char *what = win_w * win_h > LK_MAX_WIN ? "winSize too large"
                         : lk_max_level(rois[4 * k + 3], rois[4 * k + 2], win_w, win_h, max_level) + 1 > LK_MAX_LEVELS ? "too many pyramid levels" : nullptr;
        if (what) return who ? fail(RM_E_UNSUPPORTED, "%s: %s (subject %d)", who, what, k) : fail(RM_E_UNSUPPORTED, "%s", what);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t frame_bytes = (size_t)H * W * dtype_size(dtype);
    lk_clamp_criteria(max_count, epsilon);

    // table rows: the live subjects first (row j = subject live[j]), then the others
    std::vector<int> live, dead;
    for (int k = 0; k < K; ++k) (states[k]->fs.npts > 0 ? live : dead).push_back(k);
    const int KL = (int)live.size(), KD = (int)dead.size();
    std::vector<FlowSubject> tab((size_t)K);
    std::memset(tab.data(), 0, sizeof(FlowSubject) * (size_t)K);
    size_t slot_bytes = 0, max_px[LK_MAX_LEVELS] = {0}, dead_px = 0;
    int P = 0, top_levels = 0, max_staged = 0;
    bool any_seq = false;
    for (int j = 0; j < KL; ++j) {
        const int k = live[j];
        FlowSubject &S = tab[j];
        S.x = rois[4 * k]; S.y = rois[4 * k + 1]; S.w = rois[4 * k + 2]; S.h = rois[4 * k + 3];
        S.npts = states[k]->fs.npts; S.pt0 = P;
        P += S.npts;
        S.L.n = lk_max_level(S.h, S.w, win_w, win_h, max_level) + 1;
        for (int l = 0, sh = S.h, sw = S.w; l < S.L.n; ++l, sh = (sh + 1) / 2, sw = (sw + 1) / 2) {
            S.L.h[l] = sh; S.L.w[l] = sw; S.L.stride[l] = (size_t)sh * sw;
            slot_bytes += S.L.stride[l] * (1 + 2 * sizeof(short));
            max_px[l] = std::max(max_px[l], S.L.stride[l]);
        }
        top_levels = std::max(top_levels, S.L.n);
        if (S.npts <= FLOW_FINISH_MAX) max_staged = std::max(max_staged, S.npts); else any_seq = true;
    }
    for (int j = 0; j < KD; ++j) {
        const int k = dead[j];
        FlowSubject &S = tab[KL + j];
        S.x = rois[4 * k]; S.y = rois[4 * k + 1]; S.w = rois[4 * k + 2]; S.h = rois[4 * k + 3];
        dead_px = std::max(dead_px, (size_t)S.w * S.h);
    }
    const long long cap = ctx->dbg.flow_clip_bytes > 0 ? ctx->dbg.flow_clip_bytes : FLOW_CLIP_BYTES;
    const int C = KL ? (int)std::max<long long>(1, std::min<long long>(std::min(N, FLOW_CLIP_MAX_CHUNK), cap / (long long)slot_bytes - 1)) : 1;

    // every buffer the call needs, of the context (arenas, point arrays, table) and of the states, before anything is enqueued
    uint8_t *img_arena = nullptr, *d_st = nullptr, *carry_a[2] = {nullptr, nullptr}, *d_tab_bytes = nullptr;
    short *der_arena = nullptr;
    float *d_pos = nullptr, *d_res = nullptr, *carry_p[2] = {nullptr, nullptr};
    const size_t tab_bytes = sizeof(FlowSubject) * (size_t)K, up_bytes = tab_bytes + sizeof(int) * (size_t)P;
    RM_TRY(flow_buf(ctx->flow, "fm_table", up_bytes, &d_tab_bytes));
    const FlowSubject *d_tab = (const FlowSubject *)d_tab_bytes;
    const int *d_pt_subject = (const int *)(d_tab_bytes + tab_bytes);
    if (KL) {
        size_t img_px = 0;   // pixels of one image of every level of every live subject
        for (int j = 0; j < KL; ++j) for (int l = 0; l < tab[j].L.n; ++l) img_px += tab[j].L.stride[l];
        RM_TRY(flow_buf(ctx->flow, "fm_img", img_px * (size_t)(C + 1), &img_arena));
        RM_TRY(flow_buf(ctx->flow, "fm_deriv", img_px * 2 * sizeof(short) * (size_t)C, &der_arena));
        RM_TRY(flow_buf(ctx->flow, "fm_pos", sizeof(float) * 2 * (size_t)P * C, &d_pos));
        RM_TRY(flow_buf(ctx->flow, "fm_status", (size_t)P * C, &d_st));
        RM_TRY(flow_buf(ctx->flow, "fm_res", sizeof(float) * 4 * (size_t)N * KL, &d_res));
        for (int i = 0; i < 2; ++i) {
            RM_TRY(flow_buf(ctx->flow, i ? "fm_carry_pts_b" : "fm_carry_pts_a", sizeof(float) * 2 * (size_t)P, &carry_p[i]));
            RM_TRY(flow_buf(ctx->flow, i ? "fm_carry_alive_b" : "fm_carry_alive_a", (size_t)P, &carry_a[i]));
        }
    }
    std::vector<uint8_t *> st_prev((size_t)K, nullptr);                  // [k]: the crop the subject tracks from
    std::vector<float *> st_pts((size_t)K, nullptr);                     // [k]: its points
    std::vector<uint8_t *> st_cur((size_t)K * LK_MAX_LEVELS, nullptr);   // [k][l]: level l of the "current" side
    size_t img_off = 0, der_off = 0;
    for (int j = 0; j < K; ++j) {
        const int k = j < KL ? live[j] : dead[j - KL];
        FlowState &fs = states[k]->fs;
        FlowSubject &S = tab[j];
        const int cur_side = fs.flip ^ 1;
        RM_TRY(flow_state_crop(fs, cur_side, &st_cur[(size_t)k * LK_MAX_LEVELS]));
        if (j >= KL) { S.crop_dst = st_cur[(size_t)k * LK_MAX_LEVELS]; continue; }
        float *pa = nullptr, *pb = nullptr;
        RM_TRY(flow_state_crop(fs, fs.flip, &st_prev[k]));
        RM_TRY(flow_state_pts(fs, &pa, &pb));
        st_pts[k] = fs.flip ? pb : pa;
        S.next_pts = fs.flip ? pa : pb;
        for (int l = 0; l < S.L.n; ++l) {
            if (l > 0) RM_TRY(flow_state_pyr(fs, cur_side, l, S.L.stride[l], &st_cur[(size_t)k * LK_MAX_LEVELS + l]));
            S.L.prev[l] = img_arena + img_off; S.L.next[l] = S.L.prev[l] + S.L.stride[l]; S.L.deriv[l] = der_arena + der_off;
            img_off += S.L.stride[l] * (size_t)(C + 1); der_off += S.L.stride[l] * 2 * (size_t)C;
        }
        S.crop_dst = const_cast<uint8_t *>(S.L.next[0]);
    }
    std::vector<uint8_t> up(up_bytes);
    std::memcpy(up.data(), tab.data(), tab_bytes);
    int *pt_subject = (int *)(up.data() + tab_bytes);
    for (int j = 0; j < KL; ++j) for (int i = 0; i < tab[j].npts; ++i) pt_subject[tab[j].pt0 + i] = j;

    for (size_t i = 0; i < (size_t)N * K; ++i) { mean_xy_host[2 * i] = mean_xy_host[2 * i + 1] = 0.f; n_good_host[i] = 0; }
    HIP_TRY(hipMemcpyAsync(d_tab_bytes, up.data(), up_bytes, hipMemcpyHostToDevice, s));
    if (KD)   // nothing to track: the previous image advances to the clip's last frame (base.py:381)
        RM_TRY(flow_multi_crop((const char *)frames + (size_t)(N - 1) * frame_bytes, dtype, 1, H, W, d_tab + KL, KD, dead_px, s));
    std::vector<float> res;
    if (KL) {
        for (int j = 0; j < KL; ++j) {
            const int k = live[j];
            HIP_TRY(hipMemcpyAsync(carry_p[0] + 2 * (size_t)tab[j].pt0, st_pts[k], sizeof(float) * 2 * (size_t)tab[j].npts, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(const_cast<uint8_t *>(tab[j].L.prev[0]), st_prev[k], tab[j].L.stride[0], hipMemcpyDeviceToDevice, s));
        }
        HIP_TRY(hipMemsetAsync(carry_a[0], 1, (size_t)P, s));
        const size_t finish_lds = 2 * sizeof(float) * (size_t)flow_finish_pitch(max_staged);
        int last = 0;   // the image of the chunk just done that holds its last frame
        for (int c0 = 0, c = 0; c0 < N; c0 += C, ++c) {
            const int n = std::min(C, N - c0);
            const bool final_chunk = c0 + n == N;
            // frame-parallel front: crops into images 1 .. n, the pyramids of images 0 .. n, the derivatives of images 0 .. n - 1
            RM_TRY(flow_multi_crop((const char *)frames + (size_t)c0 * frame_bytes, dtype, n, H, W, d_tab, KL, max_px[0], s));
            for (int l = 1; l < top_levels; ++l)
                hipLaunchKernelGGL(k_flow_multi_pyr_down<>, dim3((unsigned)((max_px[l] + 255) / 256), n + 1, KL), dim3(256), 0, s, d_tab, l);
            for (int l = 0; l < top_levels; ++l)
                hipLaunchKernelGGL(k_flow_multi_scharr<>, dim3((unsigned)((max_px[l] + 255) / 256), n, KL), dim3(256), 0, s, d_tab, l);
            // one wave per (subject, point), one workgroup per (frame, subject)
            const float *start = carry_p[c & 1]; const uint8_t *start_alive = carry_a[c & 1];
            if (win_w * win_h <= 256)
                hipLaunchKernelGGL(k_lk_track_multi_clip<4>, dim3(P), dim3(64), 0, s, d_tab, d_pt_subject, n, start, start_alive, P, win_w, win_h, max_count,
                                   epsilon, d_pos, d_st, carry_p[(c + 1) & 1], carry_a[(c + 1) & 1]);
            else
                hipLaunchKernelGGL(k_lk_track_multi_clip<16>, dim3(P), dim3(64), 0, s, d_tab, d_pt_subject, n, start, start_alive, P, win_w, win_h, max_count,
                                   epsilon, d_pos, d_st, carry_p[(c + 1) & 1], carry_a[(c + 1) & 1]);
            float *res_c = d_res + 4 * (size_t)c0 * KL;
            if (max_staged > 0)
                hipLaunchKernelGGL(k_flow_finish_multi<>, dim3(n, KL), dim3(64), finish_lds, s, d_tab, start, d_pos, d_st, P, n, res_c, final_chunk ? 1 : 0);
            if (any_seq)
                hipLaunchKernelGGL(k_flow_finish_multi_seq<>, dim3(n, KL), dim3(1), 0, s, d_tab, start, d_pos, d_st, P, n, res_c, final_chunk ? 1 : 0);
            LAUNCH_CHECK();
            last = n;
            if (!final_chunk) {
                hipLaunchKernelGGL(k_flow_multi_carry<>, dim3(nblk(max_px[0], 256, 1024), KL), dim3(256), 0, s, d_tab, n);
                LAUNCH_CHECK();
            }
        }
        // the state the next call starts from: the last crop with its pyramid (derivatives are built by the call that tracks from it)
        for (int j = 0; j < KL; ++j)
            for (int l = 0; l < tab[j].L.n; ++l)
                HIP_TRY(hipMemcpyAsync(st_cur[(size_t)live[j] * LK_MAX_LEVELS + l], tab[j].L.prev[l] + (size_t)last * tab[j].L.stride[l], tab[j].L.stride[l],
                                       hipMemcpyDeviceToDevice, s));
        res.resize(4 * (size_t)N * KL);
        HIP_TRY(hipMemcpyAsync(res.data(), d_res, sizeof(float) * 4 * (size_t)N * KL, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(stream_wait(s));   // (the table's host memory may go now as well)
    for (int j = 0; j < KL; ++j) {
        const int k = live[j];
        for (int i = 0; i < N; ++i) {
            const float *r = &res[4 * ((size_t)i * KL + j)];
            mean_xy_host[2 * ((size_t)i * K + k)] = r[0]; mean_xy_host[2 * ((size_t)i * K + k) + 1] = r[1]; n_good_host[(size_t)i * K + k] = (int)r[2];
        }
    }
    for (int j = 0; j < K; ++j) {
        const int k = j < KL ? live[j] : dead[j - KL];
        FlowState &fs = states[k]->fs;
        const int cur_side = fs.flip ^ 1;
        fs.pyr_levels[cur_side] = j < KL ? tab[j].L.n - 1 : 0; fs.deriv_levels[cur_side] = -1;
        if (j < KL) fs.npts = n_good_host[(size_t)(N - 1) * K + k];
        fs.flip ^= 1;
    }
    return RM_OK;
}

// the one-subject entry: its own argument check, then the driver with K = 1 (its outputs [N][1][2] and [N][1] are this call's layout)
extern "C" int rm_flow_clip(rm_ctx *ctx, rm_flow_state *state, const void *frames, int dtype, int N, int H, int W, int x, int y, int w, int h,
                            int win_w, int win_h, int max_level, int max_count, double epsilon, float *mean_xy_host, int *n_good_host, void *stream)
{
    if (!ctx || !state || !frames || !mean_xy_host || !n_good_host || N < 1 || !valid_dtype(dtype) || !roi_ok(H, W, x, y, w, h) || win_w < 3 ||
        win_h < 3 || max_level < 0)
        return fail(RM_E_BADARG, "rm_flow_clip: bad argument");
    const FlowState &fs = state->fs;
    if (!fs.begun || w != fs.w || h != fs.h) return fail(RM_E_BADARG, "rm_flow_clip: rm_flow_begin has not been called on this state for this ROI size");
    if (state->device != ctx->device) return fail(RM_E_BADARG, "rm_flow_clip: the flow state belongs to another device");
    const int32_t roi[4] = {x, y, w, h};
    return flow_clips(ctx, nullptr, &state, frames, dtype, N, H, W, roi, 1, win_w, win_h, max_level, max_count, epsilon, mean_xy_host, n_good_host,
                      (hipStream_t)stream);
}

extern "C" int rm_flow_multi_clip(rm_ctx *ctx, rm_flow_state *const *states, const void *frames, int dtype, int N, int H, int W, const int32_t *rois,
                                  int K, int win_w, int win_h, int max_level, int max_count, double epsilon, float *mean_xy_host,
                                  int32_t *n_good_host, void *stream)
{
    if (!ctx || !states || !frames || !rois || !mean_xy_host || !n_good_host || N < 1 || H < 1 || W < 1 || K < 1 || K > RM_MAX_ROIS ||
        !valid_dtype(dtype) || win_w < 3 || win_h < 3 || max_level < 0 || (long long)N * K > 0x7fffffffll)
        return fail(RM_E_BADARG, "rm_flow_multi_clip: bad argument (1 <= K <= %d)", RM_MAX_ROIS);
    // the whole call is refused before anything is enqueued or any state is touched: the argument errors of every subject come first
    for (int k = 0; k < K; ++k) {
        const int32_t *r = rois + 4 * k;
        if (!states[k]) return fail(RM_E_BADARG, "rm_flow_multi_clip: subject %d has no flow state (NULL)", k);
        if (!roi_ok(H, W, r[0], r[1], r[2], r[3]))
            return fail(RM_E_BADARG, "rm_flow_multi_clip: rectangle %d (%d, %d, %d, %d) does not lie inside the %d x %d frame", k, r[0], r[1], r[2], r[3], W, H);
        const FlowState &fs = states[k]->fs;
        if (!fs.begun || r[2] != fs.w || r[3] != fs.h)
            return fail(RM_E_BADARG, "rm_flow_multi_clip: rm_flow_begin has not been called on the state of subject %d for this ROI size", k);
        if (states[k]->device != ctx->device) return fail(RM_E_BADARG, "rm_flow_multi_clip: the flow state of subject %d belongs to another device", k);
        for (int j = 0; j < k; ++j)
            if (states[j] == states[k]) return fail(RM_E_BADARG, "rm_flow_multi_clip: subject %d uses the flow state of subject %d", k, j);
    }
    return flow_clips(ctx, "rm_flow_multi_clip", states, frames, dtype, N, H, W, rois, K, win_w, win_h, max_level, max_count, epsilon, mean_xy_host,
                      n_good_host, (hipStream_t)stream);
}

// The windows of K motion lists in one upload, one launch, one download and one wait (the entry points have checked the segments):
// `rows` rows of motion are in use, `nout` > 0 values come back.
static int pca_windows(rm_ctx *ctx, const float *motion, const int32_t *seg, int K, int window, long long rows, long long nout, double *out, hipStream_t s)
{
    HIP_TRY(hipSetDevice(ctx->device));
    // one upload: the rows, behind them the (first row of the list, row inside the list) pair of every output
    const size_t rows_bytes = (sizeof(float) * 2 * (size_t)rows + 7) / 8 * 8, map_bytes = sizeof(int) * 2 * (size_t)nout;
    std::vector<uint8_t> up(rows_bytes + map_bytes);
    std::memcpy(up.data(), motion, sizeof(float) * 2 * (size_t)rows);
    int *map = (int *)(up.data() + rows_bytes);
    for (int k = 0; k < K; ++k)
        for (int j = seg[3 * k + 2]; j < seg[3 * k + 1]; ++j) { *map++ = seg[3 * k]; *map++ = j; }
    uint8_t *d_in = nullptr;
    double *d_o = nullptr;
    RM_TRY(flow_buf(ctx->flow, "pcawm_in", up.size(), &d_in));
    RM_TRY(flow_buf(ctx->flow, "pcawm_out", sizeof(double) * (size_t)nout, &d_o));
    HIP_TRY(hipMemcpyAsync(d_in, up.data(), up.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pca_reduce_windows_multi<>, dim3((unsigned)nout), dim3(64), 0, s, (const float *)d_in, (const int *)(d_in + rows_bytes), window, d_o);
    LAUNCH_CHECK();
    HIP_TRY(hipMemcpyAsync(out, d_o, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));
    return RM_OK;
}

extern "C" int rm_pca_reduce_windows(rm_ctx *ctx, const float *motion, int n, int first, int window, double *out, void *stream)
{
    if (!ctx || !motion || !out || n < 0 || first < 0 || first > n || window < 1) return fail(RM_E_BADARG, "rm_pca_reduce_windows: bad argument");
    if (first == n) return RM_OK;
    const int32_t seg[3] = {0, n, first};
    return pca_windows(ctx, motion, seg, 1, window, n, n - first, out, (hipStream_t)stream);
}

// seg[k] = {first row of list k inside motion, its number of rows n_k, first_k}: list k's outputs are rm_pca_reduce_windows(its rows,
// n_k, first_k, window), one list after the other in out.  The lists may leave gaps between them but may not overlap.
extern "C" int rm_pca_reduce_windows_multi(rm_ctx *ctx, const float *motion, const int32_t *seg, int K, int window, double *out, void *stream)
{
    if (!ctx || !seg || K < 1 || K > RM_MAX_ROIS || window < 1) return fail(RM_E_BADARG, "rm_pca_reduce_windows_multi: bad argument (1 <= K <= %d)", RM_MAX_ROIS);
    long long rows = 0, nout = 0;
    for (int k = 0; k < K; ++k) {
        const long long row0 = seg[3 * k], n = seg[3 * k + 1], first = seg[3 * k + 2];
        if (row0 < 0 || n < 0 || first < 0 || first > n || row0 + n > 0x7fffffffll)
            return fail(RM_E_BADARG, "rm_pca_reduce_windows_multi: bad segment %d (first row %lld, %lld rows, first %lld)", k, row0, n, first);
        for (int j = 0; j < k; ++j)
            if (n > 0 && seg[3 * j + 1] > 0 && row0 < (long long)seg[3 * j] + seg[3 * j + 1] && seg[3 * j] < row0 + n)
                return fail(RM_E_BADARG, "rm_pca_reduce_windows_multi: segments %d and %d overlap", j, k);
        rows = std::max(rows, n > 0 ? row0 + n : 0);
        nout += n - first;
    }
    if (nout > 0x7fffffffll || (rows > 0 && !motion) || (nout > 0 && !out)) return fail(RM_E_BADARG, "rm_pca_reduce_windows_multi: bad argument");
    if (nout == 0) return RM_OK;
    return pca_windows(ctx, motion, seg, K, window, rows, nout, out, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// developer build only (-DRM_TRACE, librespmon_hip_trace.so; tools/trace_tail.py): workgroup timelines
// ------------------------------------------------------------------------------------------

