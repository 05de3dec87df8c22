// respmon_amd/csrc/rm_phase_motion.hip -- rm_phase_motion_*: the 'phase' motion signal of extract_motion.  Per frame and rectangle the
// amplitude-weighted sums of the quaternionic phase difference of ONE Riesz-pyramid level between consecutive frames (the quantity
// rm_phase_* shifts a level by), for K subjects and a whole clip in one call (rm_phase_motion_kernels.h; the rule: include/respmon_hip.h).
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_internal.h"
#include "rm_phase_motion_kernels.h"

using namespace rm;

// The session of one subject: the level of the previous frame, I alone (the kernel recomputes R1p, R2p, Ap from it), in two planes
// the chunks alternate between.  Its own allocation: it survives every other call on the context.
struct rm_phase_motion {
    int device = 0;
    int w = 0, h = 0, level = 0;
    int lh[PM_LEVELS] = {0}, lw[PM_LEVELS] = {0};   // G_0 .. G_level+1
    size_t px = 0;                                   // doubles of G_0 .. G_level+1 of one frame
    double *state = nullptr;                         // [2][lh * lw]
    int parity = 0;                                  // the plane that holds the previous frame
    long long seen = 0;                              // frames since creation or the last reset
};

constexpr long long PM_CHUNK_BYTES = 256ll << 20;   // workspace cap of one chunk, summed over the subjects
constexpr int PM_MAX_CHUNK = 32768;                 // frames per chunk at most: the frame index is a grid's y dimension

static bool pm_roi_ok(int H, int W, int x, int y, int w, int h) { return x >= 0 && y >= 0 && w >= 1 && h >= 1 && x <= W - w && y <= H - h; }

extern "C" int rm_phase_motion_create(rm_ctx *ctx, int w, int h, int level, rm_phase_motion **out)
{
    if (out) *out = nullptr;
    if (!ctx || !out || w < 1 || h < 1 || level < 0) return fail(RM_E_BADARG, "rm_phase_motion_create: bad argument (w, h >= 1, level >= 0)");
    if (level > PM_MAX_LEVEL) return fail(RM_E_UNSUPPORTED, "rm_phase_motion_create: level %d > %d", level, PM_MAX_LEVEL);
    HIP_TRY(hipSetDevice(ctx->device));
    rm_phase_motion *st = new rm_phase_motion;
    st->device = ctx->device;
    st->w = w; st->h = h; st->level = level;
    for (int j = 0, sh = h, sw = w; j <= level + 1; ++j, sh = (sh + 1) / 2, sw = (sw + 1) / 2) {
        st->lh[j] = sh; st->lw[j] = sw;
        st->px += (size_t)sh * sw;
    }
    const size_t bytes = sizeof(double) * 2 * (size_t)st->lh[level] * st->lw[level];
    hipError_t e = hipMalloc((void **)&st->state, bytes);
    if (e != hipSuccess) {
        delete st;
        return fail(RM_E_HIP, "rm_phase_motion_create: %zu bytes for the state: %s", bytes, hipGetErrorString(e));
    }
    *out = st;
    return RM_OK;
}

extern "C" int rm_phase_motion_destroy(rm_phase_motion *st)
{
    if (!st) return RM_OK;
    (void)hipSetDevice(st->device);
    if (st->state) (void)hipFree(st->state);   // (synchronises with the work that still uses the state)
    delete st;
    return RM_OK;
}

extern "C" int rm_phase_motion_reset(rm_ctx *ctx, rm_phase_motion *st)
{
    if (!ctx || !st) return fail(RM_E_BADARG, "rm_phase_motion_reset: bad argument");
    st->seen = 0;   // the next frame returns zeros and becomes the state, in stream order
    return RM_OK;
}

extern "C" int rm_phase_motion_info(const rm_phase_motion *st, long long *frames_seen, int *lh, int *lw, size_t *state_bytes)
{
    if (!st) return fail(RM_E_BADARG, "rm_phase_motion_info: bad argument");
    if (frames_seen) *frames_seen = st->seen;
    if (lh) *lh = st->lh[st->level];
    if (lw) *lw = st->lw[st->level];
    if (state_bytes) *state_bytes = sizeof(double) * 2 * (size_t)st->lh[st->level] * st->lw[st->level];
    return RM_OK;
}

// The entry points have checked the arguments.  Launches per chunk: 1 crop + (top level + 1) pyrDown + 1 level + 1 reduce + 1 finish,
// whatever N and K; one table upload, one result copy and one stream wait per call.
static int phase_motion_clips(rm_ctx *ctx, rm_phase_motion *const *states, const void *frames, int dtype, int N, int H, int W, const int32_t *rois,
                              int K, double *sums_host, hipStream_t s)
{
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<PmSubject> tab((size_t)K);
    std::memset(tab.data(), 0, sizeof(PmSubject) * (size_t)K);
    size_t frame_px = 0, max_px0 = 0, max_pxl = 0;
    unsigned max_down[PM_LEVELS] = {0};
    unsigned long long TT = 0;
    int top = 0, max_tiles = 0;
    for (int k = 0; k < K; ++k) frame_px += states[k]->px;
    const long long per_frame = (long long)sizeof(double) * (long long)frame_px;
    long long C = std::max<long long>(1, std::min<long long>(std::min(N, PM_MAX_CHUNK), PM_CHUNK_BYTES / per_frame));
    if (ctx->dbg.phase_motion_frames > 0) C = std::min<long long>(C, ctx->dbg.phase_motion_frames);
    size_t at = 0;
    for (int k = 0; k < K; ++k) {
        const rm_phase_motion *st = states[k];
        PmSubject &S = tab[k];
        S.x = rois[4 * k]; S.y = rois[4 * k + 1]; S.level = st->level;
        for (int j = 0; j <= st->level + 1; ++j) {
            S.h[j] = st->lh[j]; S.w[j] = st->lw[j]; S.off[j] = at;
            at += (size_t)C * st->lh[j] * st->lw[j];
            if (j > 0) max_down[j] = std::max(max_down[j], (unsigned)((S.w[j] + PD_TX - 1) / PD_TX) * (unsigned)((S.h[j] + PD_TY - 1) / PD_TY));
        }
        const int lh = S.h[S.level], lw = S.w[S.level];
        S.ntx = (lw + PM_TW - 1) / PM_TW;
        S.ntiles = S.ntx * ((lh + PM_TH - 1) / PM_TH);
        S.tile0 = (unsigned)TT;
        TT += (unsigned long long)S.ntiles;
        S.first = st->seen == 0; S.parity = st->parity; S.state = st->state;
        top = std::max(top, S.level);
        max_tiles = std::max(max_tiles, S.ntiles);
        max_px0 = std::max(max_px0, (size_t)S.h[0] * S.w[0]);
        max_pxl = std::max(max_pxl, (size_t)lh * lw);
    }
    if (TT >= (1ull << 31)) return fail(RM_E_UNSUPPORTED, "rm_phase_motion_multi_clip: the rectangles are too large");

    // every buffer the call needs before anything is enqueued
    double *wsp = nullptr, *part = nullptr, *res = nullptr;
    PmSubject *d_tab = nullptr;
    RM_TRY(ws(ctx, "pm_table", (size_t)K, &d_tab));
    RM_TRY(ws(ctx, "pm_levels", at, &wsp));
    RM_TRY(ws(ctx, "pm_part", (size_t)C * TT * 3, &part));
    RM_TRY(ws(ctx, "pm_res", (size_t)N * K * 3, &res));
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(PmSubject) * (size_t)K, hipMemcpyHostToDevice, s));
    const size_t frame_bytes = (size_t)H * W * dtype_size(dtype);
    int chunks = 0;
    for (int c0 = 0; c0 < N; c0 += (int)C, ++chunks) {
        const int n = (int)std::min<long long>(C, N - c0);
        const void *f = (const uint8_t *)frames + (size_t)c0 * frame_bytes;
        dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((k_pm_crop<T>), dim3(nblk(max_px0, 256, 1024), (unsigned)n, (unsigned)K), dim3(256), 0, s, (const T *)f, (size_t)H * W, W,
                               (const PmSubject *)d_tab, wsp);
        });
        for (int j = 1; j <= top + 1; ++j)
            hipLaunchKernelGGL(k_pm_down, dim3(max_down[j], (unsigned)n, (unsigned)K), dim3(256), 0, s, (const PmSubject *)d_tab, wsp, j);
        hipLaunchKernelGGL(k_pm_level, dim3(nblk(max_pxl, 256, 1024), (unsigned)n, (unsigned)K), dim3(256), 0, s, (const PmSubject *)d_tab, wsp);
        hipLaunchKernelGGL(k_pm_reduce, dim3((unsigned)max_tiles, (unsigned)K), dim3(256), 0, s, (const PmSubject *)d_tab, (const double *)wsp, n, chunks,
                           (unsigned)TT, part);
        hipLaunchKernelGGL(k_pm_finish, dim3((unsigned)((n * K * 3 + 63) / 64)), dim3(64), 0, s, (const PmSubject *)d_tab, (const double *)part, n, K,
                           (unsigned)TT, c0, res);
        LAUNCH_CHECK();
    }
    HIP_TRY(hipMemcpyAsync(sums_host, res, sizeof(double) * (size_t)N * K * 3, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));   // (the table's host memory may go now as well)
    for (int k = 0; k < K; ++k) {
        states[k]->parity = (states[k]->parity + chunks) & 1;
        states[k]->seen += N;
    }
    return RM_OK;
}

// the checks both entry points share, subject by subject; `who` names the entry point, the texts name the first offending subject
static int phase_motion_check(rm_ctx *ctx, const char *who, rm_phase_motion *const *states, const void *frames, int dtype, int N, int H, int W,
                              const int32_t *rois, int K, const double *sums_host)
{
    if (!ctx || !states || !frames || !rois || !sums_host || N < 1 || H < 1 || W < 1 || K < 1 || K > RM_MAX_ROIS || (long long)N * K * 3 > 0x7fffffffll)
        return fail(RM_E_BADARG, "%s: bad argument (1 <= K <= %d, N >= 1)", who, RM_MAX_ROIS);
    if (dtype == RM_BGR8) return fail(RM_E_UNSUPPORTED, "%s: RM_BGR8 frames (colour is not supported: convert with rm_bgr_to_gray)", who);
    if (!valid_dtype(dtype)) return fail(RM_E_BADARG, "%s: dtype %d is no gray frame dtype", who, dtype);
    for (int k = 0; k < K; ++k) {
        const int32_t *r = rois + 4 * k;
        if (!states[k]) return fail(RM_E_BADARG, "%s: subject %d has no state (NULL)", who, k);
        if (!pm_roi_ok(H, W, r[0], r[1], r[2], r[3]))
            return fail(RM_E_BADARG, "%s: rectangle %d (%d, %d, %d, %d) does not lie inside the %d x %d frame", who, k, r[0], r[1], r[2], r[3], W, H);
        if (r[2] != states[k]->w || r[3] != states[k]->h)
            return fail(RM_E_BADARG, "%s: the state of subject %d was created for %d x %d rectangles, not %d x %d", who, k, states[k]->w, states[k]->h, r[2], r[3]);
        if (states[k]->device != ctx->device) return fail(RM_E_BADARG, "%s: the state of subject %d belongs to device %d", who, k, states[k]->device);
        for (int j = 0; j < k; ++j)
            if (states[j] == states[k]) return fail(RM_E_BADARG, "%s: subject %d uses the state of subject %d", who, k, j);
    }
    return RM_OK;
}

extern "C" int rm_phase_motion_multi_clip(rm_ctx *ctx, rm_phase_motion *const *states, const void *frames, int dtype, int N, int H, int W,
                                          const int32_t *rois, int K, double *sums_host, void *stream)
{
    RM_TRY(phase_motion_check(ctx, "rm_phase_motion_multi_clip", states, frames, dtype, N, H, W, rois, K, sums_host));
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    return phase_motion_clips(ctx, states, frames, dtype, N, H, W, rois, K, sums_host, (hipStream_t)stream);
}

// the one-subject entry: the driver with K = 1 (its output [N][1][3] is this call's layout)
extern "C" int rm_phase_motion_clip(rm_ctx *ctx, rm_phase_motion *st, const void *frames, int dtype, int N, int H, int W, int x, int y,
                                    double *sums_host, void *stream)
{
    if (!st) return fail(RM_E_BADARG, "rm_phase_motion_clip: bad argument (no state)");
    const int32_t roi[4] = {x, y, st->w, st->h};
    RM_TRY(phase_motion_check(ctx, "rm_phase_motion_clip", &st, frames, dtype, N, H, W, roi, 1, sums_host));
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    return phase_motion_clips(ctx, &st, frames, dtype, N, H, W, roi, 1, sums_host, (hipStream_t)stream);
}
