// respmon_amd/csrc/rm_stabilize.hip -- rm_stab_*, rm_warp_shift: a shaky camera taken out of the frames before anything else looks at
// them.  Per frame the global shift against a fixed reference frame (translation-only Gauss-Newton, coarse to fine on the library's own
// Gaussian pyramid, every sum and the 2 x 2 update on the device) and the bilinear warp by it (rm_stabilize_kernels.h; the rule:
// include/respmon_hip.h).
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_internal.h"
#include "rm_stabilize_kernels.h"

using namespace rm;

// The session: the reference's levels level_fine .. level_coarse and their (a, bb, c, det).  Its own allocation: it survives every
// other call on the context.
struct rm_stab {
    int device = 0;
    int H = 0, W = 0, iters = 0;
    double max_shift = 0;
    StabGeom g{};                       // off[] is filled per call (it depends on the chunk capacity)
    int nt[STAB_LEVELS] = {0};          // reduction tiles of level l
    int b[STAB_LEVELS] = {0};           // border of the region at level l
    bool empty[STAB_LEVELS] = {false};  // the region of level l is empty
    size_t px = 0;                      // doubles of G_0 .. G_lc of one frame
    int max_nt = 1;
    double *state = nullptr;
    size_t state_doubles = 0;
    bool has_ref = false;
    long long seen = 0;                 // frames since creation or the last reset
};

constexpr long long STAB_CHUNK_BYTES = 256ll << 20;   // workspace cap of one chunk
constexpr int STAB_MAX_CHUNK = 32768;                 // frames per chunk at most: the frame index is a grid's y dimension

static bool stab_ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}
static bool stab_out_dtype_ok(int dtype, int out_dtype)
{
    if (dtype == RM_BGR8) return out_dtype == RM_BGR8;
    return out_dtype == RM_U8 || out_dtype == RM_U16 || out_dtype == RM_F32 || out_dtype == RM_F64;
}

extern "C" int rm_stab_create(rm_ctx *ctx, int H, int W, int level_coarse, int level_fine, int iterations, double max_shift, rm_stab **out)
{
    if (out) *out = nullptr;
    if (!ctx || !out || H < 1 || W < 1 || level_fine < 0 || level_coarse < level_fine || iterations < 1 || !(max_shift > 0.0) || !std::isfinite(max_shift))
        return fail(RM_E_BADARG, "rm_stab_create: bad argument (H, W >= 1, level_coarse >= level_fine >= 0, iterations >= 1, max_shift finite and > 0)");
    if (level_coarse > STAB_MAX_LEVEL) return fail(RM_E_UNSUPPORTED, "rm_stab_create: level %d > %d", level_coarse, STAB_MAX_LEVEL);
    if (max_shift > 64.0) return fail(RM_E_UNSUPPORTED, "rm_stab_create: max_shift %g > 64", max_shift);
    HIP_TRY(hipSetDevice(ctx->device));
    rm_stab *st = new rm_stab;
    st->device = ctx->device;
    st->H = H; st->W = W; st->iters = iterations; st->max_shift = max_shift;
    st->g.lc = level_coarse; st->g.lf = level_fine;
    size_t at = 4 * STAB_LEVELS;
    for (int l = 0, h = H, w = W; l <= level_coarse; ++l, h = (h + 1) / 2, w = (w + 1) / 2) {
        st->g.h[l] = h; st->g.w[l] = w;
        st->px += (size_t)h * w;
        st->nt[l] = ((w + STAB_TW - 1) / STAB_TW) * ((h + STAB_TH - 1) / STAB_TH);
        st->b[l] = (int)std::ceil(max_shift / (double)(1 << l)) + 2;
        st->empty[l] = w < 2 * st->b[l] + 1 || h < 2 * st->b[l] + 1;
        if (l >= level_fine) {
            st->g.roff[l] = at;
            at += (size_t)h * w;
            st->max_nt = std::max(st->max_nt, st->nt[l]);
        }
    }
    st->state_doubles = at;
    hipError_t e = hipMalloc((void **)&st->state, sizeof(double) * at);
    if (e != hipSuccess) {
        delete st;
        return fail(RM_E_HIP, "rm_stab_create: %zu bytes for the state: %s", sizeof(double) * at, hipGetErrorString(e));
    }
    *out = st;
    return RM_OK;
}

extern "C" int rm_stab_destroy(rm_stab *st)
{
    if (!st) return RM_OK;
    (void)hipSetDevice(st->device);
    if (st->state) (void)hipFree(st->state);   // (synchronises with the work that still uses the state)
    delete st;
    return RM_OK;
}

extern "C" int rm_stab_reset(rm_ctx *ctx, rm_stab *st)
{
    if (!ctx || !st) return fail(RM_E_BADARG, "rm_stab_reset: bad argument");
    st->seen = 0;
    st->has_ref = false;   // the next frame becomes the reference, in stream order
    return RM_OK;
}

extern "C" int rm_stab_info(const rm_stab *st, long long *frames_seen, int *has_reference, size_t *state_bytes)
{
    if (!st) return fail(RM_E_BADARG, "rm_stab_info: bad argument");
    if (frames_seen) *frames_seen = st->seen;
    if (has_reference) *has_reference = st->has_ref ? 1 : 0;
    if (state_bytes) *state_bytes = sizeof(double) * st->state_doubles;
    return RM_OK;
}

// G_0 .. G_lc of n frames into the chunk workspace
static int stab_pyramid(const rm_stab *st, const StabGeom &g, const void *frames, int dtype, int n, double *wsp, hipStream_t s)
{
    const size_t px = (size_t)st->H * st->W;
    if (dtype == RM_BGR8)
        hipLaunchKernelGGL((k_stab_gray<bgr8_t>), dim3(nblk(px, 256, 2048), (unsigned)n), dim3(256), 0, s, (const bgr8_t *)frames, px, wsp + g.off[0]);
    else
        dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((k_stab_gray<T>), dim3(nblk(px, 256, 2048), (unsigned)n), dim3(256), 0, s, (const T *)frames, px, wsp + g.off[0]);
        });
    for (int j = 1; j <= g.lc; ++j) {
        const unsigned tiles = (unsigned)((g.w[j] + PD_TX - 1) / PD_TX) * (unsigned)((g.h[j] + PD_TY - 1) / PD_TY);
        hipLaunchKernelGGL(k_stab_down, dim3(tiles, (unsigned)n), dim3(256), 0, s, g, wsp, j);
    }
    LAUNCH_CHECK();
    return RM_OK;
}

// the first frame of the chunk workspace becomes the reference: its levels into the session, then a, bb, c, det of each
static int stab_take_reference(rm_stab *st, const StabGeom &g, const double *wsp, double *part, hipStream_t s)
{
    for (int l = g.lf; l <= g.lc; ++l) {
        double *R = st->state + g.roff[l];
        HIP_TRY(hipMemcpyAsync(R, wsp + g.off[l], sizeof(double) * (size_t)g.h[l] * g.w[l], hipMemcpyDeviceToDevice, s));
        if (st->empty[l]) continue;
        hipLaunchKernelGGL(k_stab_hsums, dim3((unsigned)st->nt[l]), dim3(256), 0, s, (const double *)R, g.h[l], g.w[l], st->b[l], part);
        hipLaunchKernelGGL(k_stab_hfold, dim3(1), dim3(64), 0, s, (const double *)part, st->nt[l], st->state + 4 * l);
    }
    LAUNCH_CHECK();
    return RM_OK;
}

static void stab_offsets(const rm_stab *st, long long C, StabGeom &g, size_t &total)
{
    g = st->g;
    size_t at = 0;
    for (int j = 0; j <= g.lc; ++j) {
        g.off[j] = at;
        at += (size_t)C * g.h[j] * g.w[j];
    }
    total = at;
}

static int stab_warp(const void *frames, int dtype, int n, int H, int W, const double *d, void *out, int out_dtype, hipStream_t s)
{
    const unsigned rows = (unsigned)std::min(H, 65535);
    if (dtype == RM_BGR8) {
        hipLaunchKernelGGL(k_stab_warp_bgr, dim3(nblk(3 * (size_t)W, 256, 1u << 30), rows, (unsigned)n), dim3(256), 0, s, (const uint8_t *)frames, H, W, d,
                           (uint8_t *)out);
    } else {
        dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            const dim3 grid(nblk((size_t)W, 256, 1u << 30), rows, (unsigned)n);
            switch (out_dtype) {
            case RM_U8: hipLaunchKernelGGL((k_stab_warp<T, uint8_t>), grid, dim3(256), 0, s, (const T *)frames, H, W, d, (uint8_t *)out); break;
            case RM_U16: hipLaunchKernelGGL((k_stab_warp<T, uint16_t>), grid, dim3(256), 0, s, (const T *)frames, H, W, d, (uint16_t *)out); break;
            case RM_F32: hipLaunchKernelGGL((k_stab_warp<T, float>), grid, dim3(256), 0, s, (const T *)frames, H, W, d, (float *)out); break;
            default: hipLaunchKernelGGL((k_stab_warp<T, double>), grid, dim3(256), 0, s, (const T *)frames, H, W, d, (double *)out); break;
            }
        });
    }
    LAUNCH_CHECK();
    return RM_OK;
}

extern "C" int rm_stab_set_reference(rm_ctx *ctx, rm_stab *st, const void *frame, int dtype, void *stream)
{
    if (!ctx || !st || !frame) return fail(RM_E_BADARG, "rm_stab_set_reference: bad argument");
    if (!valid_buffer_dtype(dtype)) return fail(RM_E_BADARG, "rm_stab_set_reference: dtype %d is no frame dtype", dtype);
    if (st->device != ctx->device) return fail(RM_E_BADARG, "rm_stab_set_reference: the state belongs to device %d", st->device);
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    hipStream_t s = (hipStream_t)stream;
    StabGeom g;
    size_t total = 0;
    stab_offsets(st, 1, g, total);
    double *wsp = nullptr, *part = nullptr;
    RM_TRY(ws(ctx, "stab_levels", total, &wsp));
    RM_TRY(ws(ctx, "stab_part", (size_t)st->max_nt * 3, &part));
    RM_TRY(stab_pyramid(st, g, frame, dtype, 1, wsp, s));
    RM_TRY(stab_take_reference(st, g, wsp, part, s));
    st->has_ref = true;
    return RM_OK;
}

// Launches per chunk: 1 gray + level_coarse pyrDown + 1 init + 2 per level and iteration + 1 warp, whatever N (the call that takes its
// reference adds a copy and two launches per level); one result copy and one stream wait per call.
extern "C" int rm_stab_push(rm_ctx *ctx, rm_stab *st, const void *frames, int dtype, int N, void *out, int out_dtype, double *shifts_host,
                            int32_t *flags_host, void *stream)
{
    if (!ctx || !st || !frames || !shifts_host || !flags_host || N < 1) return fail(RM_E_BADARG, "rm_stab_push: bad argument (N >= 1, no NULL but out_dev)");
    if (!valid_buffer_dtype(dtype)) return fail(RM_E_BADARG, "rm_stab_push: dtype %d is no frame dtype", dtype);
    if (st->device != ctx->device) return fail(RM_E_BADARG, "rm_stab_push: the state belongs to device %d", st->device);
    const int H = st->H, W = st->W;
    const size_t npix = (size_t)H * W, in_fb = npix * dtype_size(dtype);
    if (out) {
        if (!stab_out_dtype_ok(dtype, out_dtype))
            return fail(RM_E_BADARG, "rm_stab_push: out_dtype %d (RM_U8, RM_U16, RM_F32 or RM_F64 for gray frames, RM_BGR8 for RM_BGR8 frames)", out_dtype);
        if (stab_ranges_overlap(frames, (size_t)N * in_fb, out, (size_t)N * npix * dtype_size(out_dtype)))
            return fail(RM_E_BADARG, "rm_stab_push: out_dev overlaps the frames");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    hipStream_t s = (hipStream_t)stream;

    const long long per_frame = (long long)sizeof(double) * (long long)(st->px + (size_t)st->max_nt * 3);
    long long C = std::max<long long>(1, std::min<long long>(std::min(N, STAB_MAX_CHUNK), STAB_CHUNK_BYTES / per_frame));
    if (ctx->dbg.stab_frames > 0) C = std::min<long long>(C, ctx->dbg.stab_frames);
    StabGeom g;
    size_t total = 0;
    stab_offsets(st, C, g, total);
    // every buffer the call needs before anything is enqueued
    double *wsp = nullptr, *part = nullptr, *res = nullptr;
    RM_TRY(ws(ctx, "stab_levels", total, &wsp));
    RM_TRY(ws(ctx, "stab_part", (size_t)C * st->max_nt * 3, &part));
    RM_TRY(ws(ctx, "stab_res", (size_t)N * 2 + ((size_t)N + 1) / 2, &res));   // [N][2] shifts, then [N] int32 flags
    int32_t *flg = (int32_t *)(res + (size_t)N * 2);
    const size_t res_bytes = sizeof(double) * 2 * (size_t)N + sizeof(int32_t) * (size_t)N;
    std::vector<uint8_t> host(res_bytes);

    int base_flags = 0;
    for (int l = g.lf; l <= g.lc; ++l)
        if (st->empty[l]) base_flags |= STAB_FLAG_LEVEL_SKIPPED;
    const size_t out_fb = out ? npix * dtype_size(out_dtype) : 0;
    for (int c0 = 0; c0 < N; c0 += (int)C) {
        const int n = (int)std::min<long long>(C, N - c0);
        const void *f = (const uint8_t *)frames + (size_t)c0 * in_fb;
        double *d = res + 2 * (size_t)c0;
        RM_TRY(stab_pyramid(st, g, f, dtype, n, wsp, s));
        if (!st->has_ref) {
            RM_TRY(stab_take_reference(st, g, wsp, part, s));
            st->has_ref = true;
        }
        hipLaunchKernelGGL(k_stab_init, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d, flg + c0, n, base_flags);
        for (int l = g.lc; l >= g.lf; --l) {
            if (st->empty[l]) continue;
            const double scale = (double)(1 << l), inv = 1.0 / scale;
            for (int it = 0; it < st->iters; ++it) {
                hipLaunchKernelGGL(k_stab_resid, dim3((unsigned)st->nt[l], (unsigned)n), dim3(256), 0, s, g, (const double *)wsp, (const double *)st->state, l,
                                   st->b[l], inv, (const double *)d, part);
                hipLaunchKernelGGL(k_stab_update, dim3((unsigned)n), dim3(64), 0, s, (const double *)part, st->nt[l], (const double *)(st->state + 4 * l),
                                   st->max_shift / scale, scale, inv, (l == g.lf && it == st->iters - 1) ? 1 : 0, d, flg + c0);
            }
        }
        LAUNCH_CHECK();
        if (out) RM_TRY(stab_warp(f, dtype, n, H, W, d, (uint8_t *)out + (size_t)c0 * out_fb, out_dtype, s));
    }
    HIP_TRY(hipMemcpyAsync(host.data(), res, res_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));
    std::memcpy(shifts_host, host.data(), sizeof(double) * 2 * (size_t)N);
    std::memcpy(flags_host, host.data() + sizeof(double) * 2 * (size_t)N, sizeof(int32_t) * (size_t)N);
    st->seen += N;
    return RM_OK;
}

extern "C" int rm_warp_shift(rm_ctx *ctx, const void *frames, int dtype, int N, int H, int W, const double *shifts_host, void *out, int out_dtype,
                             void *stream)
{
    if (!ctx || !frames || !shifts_host || !out || N < 1 || H < 1 || W < 1) return fail(RM_E_BADARG, "rm_warp_shift: bad argument");
    if (!valid_buffer_dtype(dtype)) return fail(RM_E_BADARG, "rm_warp_shift: dtype %d is no frame dtype", dtype);
    if (!stab_out_dtype_ok(dtype, out_dtype))
        return fail(RM_E_BADARG, "rm_warp_shift: out_dtype %d (RM_U8, RM_U16, RM_F32 or RM_F64 for gray frames, RM_BGR8 for RM_BGR8 frames)", out_dtype);
    for (size_t i = 0; i < 2 * (size_t)N; ++i)
        if (!(std::fabs(shifts_host[i]) <= 1048576.0)) return fail(RM_E_BADARG, "rm_warp_shift: shift %zu of frame %zu is not finite or beyond 2^20", i & 1, i / 2);
    const size_t npix = (size_t)H * W, in_fb = npix * dtype_size(dtype), out_fb = npix * dtype_size(out_dtype);
    if (stab_ranges_overlap(frames, (size_t)N * in_fb, out, (size_t)N * out_fb)) return fail(RM_E_BADARG, "rm_warp_shift: out_dev overlaps the frames");
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    hipStream_t s = (hipStream_t)stream;
    double *d = nullptr;
    RM_TRY(ws(ctx, "stab_shifts", (size_t)N * 2, &d));
    HIP_TRY(hipMemcpyAsync(d, shifts_host, sizeof(double) * 2 * (size_t)N, hipMemcpyHostToDevice, s));
    for (int c0 = 0; c0 < N; c0 += STAB_MAX_CHUNK) {
        const int n = std::min(STAB_MAX_CHUNK, N - c0);
        RM_TRY(stab_warp((const uint8_t *)frames + (size_t)c0 * in_fb, dtype, n, H, W, d + 2 * (size_t)c0, (uint8_t *)out + (size_t)c0 * out_fb, out_dtype, s));
    }
    return RM_OK;
}

// ---- rm_stab_sim_*, rm_warp_similarity: the similarity model.  The session is rm_stab's with a header of STAB_SIM_HDR doubles per
// level: the levels above level_linear keep (a, bb, c, det) there and run the shift model's kernels as they are, the others keep the
// L D L^T factors of their 4 x 4 system.
struct rm_stab_sim {
    rm_stab t;                          // H, W, levels, iterations, max_shift, geometry, tiles, borders, state, reference, frames seen
    int ll = -1;                        // level_linear
    double max_linear = 0;
    double cx = 0, cy = 0;              // the centre of the frame in level-0 pixels
};

extern "C" int rm_stab_sim_create(rm_ctx *ctx, int H, int W, int level_coarse, int level_fine, int level_linear, int iterations, double max_shift,
                                  double max_linear, rm_stab_sim **out)
{
    if (out) *out = nullptr;
    if (!ctx || !out || H < 1 || W < 1 || level_fine < 0 || level_coarse < level_fine || iterations < 1 || !(max_shift > 0.0) || !std::isfinite(max_shift) ||
        level_linear < -1 || level_linear > level_coarse || !(max_linear > 0.0) || !std::isfinite(max_linear))
        return fail(RM_E_BADARG, "rm_stab_sim_create: bad argument (H, W >= 1, level_coarse >= level_fine >= 0, -1 <= level_linear <= level_coarse, "
                                 "iterations >= 1, max_shift and max_linear finite and > 0)");
    if (level_coarse > STAB_MAX_LEVEL) return fail(RM_E_UNSUPPORTED, "rm_stab_sim_create: level %d > %d", level_coarse, STAB_MAX_LEVEL);
    if (max_shift > 64.0) return fail(RM_E_UNSUPPORTED, "rm_stab_sim_create: max_shift %g > 64", max_shift);
    if (max_linear > 0.25) return fail(RM_E_UNSUPPORTED, "rm_stab_sim_create: max_linear %g > 0.25", max_linear);
    HIP_TRY(hipSetDevice(ctx->device));
    rm_stab_sim *ss = new rm_stab_sim;
    rm_stab *st = &ss->t;
    ss->ll = level_linear; ss->max_linear = max_linear;
    ss->cx = (double)(W - 1) * 0.5; ss->cy = (double)(H - 1) * 0.5;
    st->device = ctx->device;
    st->H = H; st->W = W; st->iters = iterations; st->max_shift = max_shift;
    st->g.lc = level_coarse; st->g.lf = level_fine;
    size_t at = (size_t)STAB_SIM_HDR * STAB_LEVELS;
    for (int l = 0, h = H, w = W; l <= level_coarse; ++l, h = (h + 1) / 2, w = (w + 1) / 2) {
        const double inv = 1.0 / (double)(1 << l);
        st->g.h[l] = h; st->g.w[l] = w;
        st->px += (size_t)h * w;
        st->nt[l] = ((w + STAB_TW - 1) / STAB_TW) * ((h + STAB_TH - 1) / STAB_TH);
        st->b[l] = l > level_linear ? (int)std::ceil(max_shift / (double)(1 << l)) + 2 : (int)std::ceil((max_shift + max_linear * (ss->cx + ss->cy)) * inv) + 2;
        st->empty[l] = w < 2 * st->b[l] + 1 || h < 2 * st->b[l] + 1;
        if (l >= level_fine) {
            st->g.roff[l] = at;
            at += (size_t)h * w;
            st->max_nt = std::max(st->max_nt, st->nt[l]);
        }
    }
    st->state_doubles = at;
    hipError_t e = hipMalloc((void **)&st->state, sizeof(double) * at);
    if (e != hipSuccess) {
        delete ss;
        return fail(RM_E_HIP, "rm_stab_sim_create: %zu bytes for the state: %s", sizeof(double) * at, hipGetErrorString(e));
    }
    *out = ss;
    return RM_OK;
}

extern "C" int rm_stab_sim_destroy(rm_stab_sim *ss)
{
    if (!ss) return RM_OK;
    (void)hipSetDevice(ss->t.device);
    if (ss->t.state) (void)hipFree(ss->t.state);   // (synchronises with the work that still uses the state)
    delete ss;
    return RM_OK;
}

extern "C" int rm_stab_sim_reset(rm_ctx *ctx, rm_stab_sim *ss)
{
    if (!ctx || !ss) return fail(RM_E_BADARG, "rm_stab_sim_reset: bad argument");
    ss->t.seen = 0;
    ss->t.has_ref = false;   // the next frame becomes the reference, in stream order
    return RM_OK;
}

extern "C" int rm_stab_sim_info(const rm_stab_sim *ss, long long *frames_seen, int *has_reference, size_t *state_bytes)
{
    if (!ss) return fail(RM_E_BADARG, "rm_stab_sim_info: bad argument");
    return rm_stab_info(&ss->t, frames_seen, has_reference, state_bytes);
}

// the first frame of the chunk workspace becomes the reference: its levels into the session, then the level's sums -- (a, bb, c, det)
// above level_linear, the ten H_ij and their factorisation at and below it.  part: max_nt * 10 doubles at least
static int stab_sim_take_reference(rm_stab_sim *ss, const StabGeom &g, const double *wsp, double *part, hipStream_t s)
{
    rm_stab *st = &ss->t;
    for (int l = g.lf; l <= g.lc; ++l) {
        double *R = st->state + g.roff[l], *hs = st->state + (size_t)STAB_SIM_HDR * l;
        HIP_TRY(hipMemcpyAsync(R, wsp + g.off[l], sizeof(double) * (size_t)g.h[l] * g.w[l], hipMemcpyDeviceToDevice, s));
        if (st->empty[l]) continue;
        if (l > ss->ll) {
            hipLaunchKernelGGL(k_stab_hsums, dim3((unsigned)st->nt[l]), dim3(256), 0, s, (const double *)R, g.h[l], g.w[l], st->b[l], part);
            hipLaunchKernelGGL(k_stab_hfold, dim3(1), dim3(64), 0, s, (const double *)part, st->nt[l], hs);
        } else {
            const double inv = 1.0 / (double)(1 << l);
            hipLaunchKernelGGL(k_stab_hsums_sim, dim3((unsigned)st->nt[l]), dim3(256), 0, s, (const double *)R, g.h[l], g.w[l], st->b[l], ss->cx * inv,
                               ss->cy * inv, part);
            hipLaunchKernelGGL(k_stab_hfold_sim, dim3(1), dim3(64), 0, s, (const double *)part, st->nt[l], hs);
        }
    }
    LAUNCH_CHECK();
    return RM_OK;
}

static int stab_sim_warp(const void *frames, int dtype, int n, int H, int W, const double *params, void *out, int out_dtype, hipStream_t s)
{
    const unsigned rows = (unsigned)std::min(H, 65535);
    if (dtype == RM_BGR8) {
        hipLaunchKernelGGL(k_stab_warp_sim_bgr, dim3(nblk(3 * (size_t)W, 256, 1u << 30), rows, (unsigned)n), dim3(256), 0, s, (const uint8_t *)frames, H, W, params,
                           (uint8_t *)out);
    } else {
        dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            const dim3 grid(nblk((size_t)W, 256, 1u << 30), rows, (unsigned)n);
            switch (out_dtype) {
            case RM_U8: hipLaunchKernelGGL((k_stab_warp_sim<T, uint8_t>), grid, dim3(256), 0, s, (const T *)frames, H, W, params, (uint8_t *)out); break;
            case RM_U16: hipLaunchKernelGGL((k_stab_warp_sim<T, uint16_t>), grid, dim3(256), 0, s, (const T *)frames, H, W, params, (uint16_t *)out); break;
            case RM_F32: hipLaunchKernelGGL((k_stab_warp_sim<T, float>), grid, dim3(256), 0, s, (const T *)frames, H, W, params, (float *)out); break;
            default: hipLaunchKernelGGL((k_stab_warp_sim<T, double>), grid, dim3(256), 0, s, (const T *)frames, H, W, params, (double *)out); break;
            }
        });
    }
    LAUNCH_CHECK();
    return RM_OK;
}

extern "C" int rm_stab_sim_set_reference(rm_ctx *ctx, rm_stab_sim *ss, const void *frame, int dtype, void *stream)
{
    if (!ctx || !ss || !frame) return fail(RM_E_BADARG, "rm_stab_sim_set_reference: bad argument");
    if (!valid_buffer_dtype(dtype)) return fail(RM_E_BADARG, "rm_stab_sim_set_reference: dtype %d is no frame dtype", dtype);
    rm_stab *st = &ss->t;
    if (st->device != ctx->device) return fail(RM_E_BADARG, "rm_stab_sim_set_reference: the state belongs to device %d", st->device);
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    hipStream_t s = (hipStream_t)stream;
    StabGeom g;
    size_t total = 0;
    stab_offsets(st, 1, g, total);
    double *wsp = nullptr, *part = nullptr;
    RM_TRY(ws(ctx, "stab_levels", total, &wsp));
    RM_TRY(ws(ctx, "stab_part", (size_t)st->max_nt * 10, &part));
    RM_TRY(stab_pyramid(st, g, frame, dtype, 1, wsp, s));
    RM_TRY(stab_sim_take_reference(ss, g, wsp, part, s));
    st->has_ref = true;
    return RM_OK;
}

// Launches per chunk: 1 gray + level_coarse pyrDown + 2 init + 2 per level and iteration + 1 pack + 1 warp, whatever N (the call that
// takes its reference adds a copy and two launches per level); one result copy and one stream wait per call.
extern "C" int rm_stab_sim_push(rm_ctx *ctx, rm_stab_sim *ss, const void *frames, int dtype, int N, void *out, int out_dtype, double *params_host,
                                int32_t *flags_host, void *stream)
{
    if (!ctx || !ss || !frames || !params_host || !flags_host || N < 1)
        return fail(RM_E_BADARG, "rm_stab_sim_push: bad argument (N >= 1, no NULL but out_dev)");
    if (!valid_buffer_dtype(dtype)) return fail(RM_E_BADARG, "rm_stab_sim_push: dtype %d is no frame dtype", dtype);
    rm_stab *st = &ss->t;
    if (st->device != ctx->device) return fail(RM_E_BADARG, "rm_stab_sim_push: the state belongs to device %d", st->device);
    const int H = st->H, W = st->W;
    const size_t npix = (size_t)H * W, in_fb = npix * dtype_size(dtype);
    if (out) {
        if (!stab_out_dtype_ok(dtype, out_dtype))
            return fail(RM_E_BADARG, "rm_stab_sim_push: out_dtype %d (RM_U8, RM_U16, RM_F32 or RM_F64 for gray frames, RM_BGR8 for RM_BGR8 frames)", out_dtype);
        if (stab_ranges_overlap(frames, (size_t)N * in_fb, out, (size_t)N * npix * dtype_size(out_dtype)))
            return fail(RM_E_BADARG, "rm_stab_sim_push: out_dev overlaps the frames");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    hipStream_t s = (hipStream_t)stream;

    const long long per_frame = (long long)sizeof(double) * (long long)(st->px + (size_t)st->max_nt * 4);
    long long C = std::max<long long>(1, std::min<long long>(std::min(N, STAB_MAX_CHUNK), STAB_CHUNK_BYTES / per_frame));
    if (ctx->dbg.stab_frames > 0) C = std::min<long long>(C, ctx->dbg.stab_frames);
    StabGeom g;
    size_t total = 0;
    stab_offsets(st, C, g, total);
    // every buffer the call needs before anything is enqueued
    double *wsp = nullptr, *part = nullptr, *res = nullptr, *dq = nullptr;
    RM_TRY(ws(ctx, "stab_levels", total, &wsp));
    RM_TRY(ws(ctx, "stab_part", std::max((size_t)C * st->max_nt * 4, (size_t)st->max_nt * 10), &part));
    RM_TRY(ws(ctx, "stab_res", (size_t)N * 4 + ((size_t)N + 1) / 2, &res));   // [N][4] parameters, then [N] int32 flags
    RM_TRY(ws(ctx, "stab_dq", (size_t)C * 4, &dq));                           // the chunk's shifts [C][2], then its linear parts [C][2]
    double *d = dq, *q = dq + 2 * (size_t)C;
    int32_t *flg = (int32_t *)(res + (size_t)N * 4);
    const size_t res_bytes = sizeof(double) * 4 * (size_t)N + sizeof(int32_t) * (size_t)N;
    std::vector<uint8_t> host(res_bytes);

    int base_flags = 0;
    for (int l = g.lf; l <= g.lc; ++l)
        if (st->empty[l]) base_flags |= STAB_FLAG_LEVEL_SKIPPED;
    const size_t out_fb = out ? npix * dtype_size(out_dtype) : 0;
    for (int c0 = 0; c0 < N; c0 += (int)C) {
        const int n = (int)std::min<long long>(C, N - c0);
        const void *f = (const uint8_t *)frames + (size_t)c0 * in_fb;
        double *params = res + 4 * (size_t)c0;
        RM_TRY(stab_pyramid(st, g, f, dtype, n, wsp, s));
        if (!st->has_ref) {
            RM_TRY(stab_sim_take_reference(ss, g, wsp, part, s));
            st->has_ref = true;
        }
        hipLaunchKernelGGL(k_stab_init, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d, flg + c0, n, base_flags);
        hipLaunchKernelGGL(k_stab_init, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, q, flg + c0, n, base_flags);
        for (int l = g.lc; l >= g.lf; --l) {
            if (st->empty[l]) continue;
            const double scale = (double)(1 << l), inv = 1.0 / scale;
            const double *hs = st->state + (size_t)STAB_SIM_HDR * l;
            for (int it = 0; it < st->iters; ++it) {
                const int last = (l == g.lf && it == st->iters - 1) ? 1 : 0;
                if (l > ss->ll) {
                    hipLaunchKernelGGL(k_stab_resid, dim3((unsigned)st->nt[l], (unsigned)n), dim3(256), 0, s, g, (const double *)wsp, (const double *)st->state, l,
                                       st->b[l], inv, (const double *)d, part);
                    hipLaunchKernelGGL(k_stab_update, dim3((unsigned)n), dim3(64), 0, s, (const double *)part, st->nt[l], hs, st->max_shift / scale, scale, inv, last,
                                       d, flg + c0);
                } else {
                    hipLaunchKernelGGL(k_stab_resid_sim, dim3((unsigned)st->nt[l], (unsigned)n), dim3(256), 0, s, g, (const double *)wsp, (const double *)st->state,
                                       l, st->b[l], inv, ss->cx * inv, ss->cy * inv, (const double *)d, (const double *)q, part);
                    hipLaunchKernelGGL(k_stab_update_sim, dim3((unsigned)n), dim3(64), 0, s, (const double *)part, st->nt[l], hs, st->max_shift / scale,
                                       ss->max_linear, scale, inv, last, d, q, flg + c0);
                }
            }
        }
        hipLaunchKernelGGL(k_stab_pack_sim, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const double *)d, (const double *)q, params, n);
        LAUNCH_CHECK();
        if (out) RM_TRY(stab_sim_warp(f, dtype, n, H, W, params, (uint8_t *)out + (size_t)c0 * out_fb, out_dtype, s));
    }
    HIP_TRY(hipMemcpyAsync(host.data(), res, res_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));
    std::memcpy(params_host, host.data(), sizeof(double) * 4 * (size_t)N);
    std::memcpy(flags_host, host.data() + sizeof(double) * 4 * (size_t)N, sizeof(int32_t) * (size_t)N);
    st->seen += N;
    return RM_OK;
}

extern "C" int rm_warp_similarity(rm_ctx *ctx, const void *frames, int dtype, int N, int H, int W, const double *params_host, void *out, int out_dtype,
                                  void *stream)
{
    if (!ctx || !frames || !params_host || !out || N < 1 || H < 1 || W < 1) return fail(RM_E_BADARG, "rm_warp_similarity: bad argument");
    if (!valid_buffer_dtype(dtype)) return fail(RM_E_BADARG, "rm_warp_similarity: dtype %d is no frame dtype", dtype);
    if (!stab_out_dtype_ok(dtype, out_dtype))
        return fail(RM_E_BADARG, "rm_warp_similarity: out_dtype %d (RM_U8, RM_U16, RM_F32 or RM_F64 for gray frames, RM_BGR8 for RM_BGR8 frames)", out_dtype);
    for (size_t i = 0; i < 4 * (size_t)N; ++i)
        if (!(std::fabs(params_host[i]) <= ((i & 3) < 2 ? 1.0 : 1048576.0)))
            return fail(RM_E_BADARG, "rm_warp_similarity: parameter %zu of frame %zu is not finite or beyond its range (|p0|, |p1| <= 1, |t| <= 2^20)", i & 3, i / 4);
    const size_t npix = (size_t)H * W, in_fb = npix * dtype_size(dtype), out_fb = npix * dtype_size(out_dtype);
    if (stab_ranges_overlap(frames, (size_t)N * in_fb, out, (size_t)N * out_fb)) return fail(RM_E_BADARG, "rm_warp_similarity: out_dev overlaps the frames");
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    hipStream_t s = (hipStream_t)stream;
    double *p = nullptr;
    RM_TRY(ws(ctx, "stab_params", (size_t)N * 4, &p));
    HIP_TRY(hipMemcpyAsync(p, params_host, sizeof(double) * 4 * (size_t)N, hipMemcpyHostToDevice, s));
    for (int c0 = 0; c0 < N; c0 += STAB_MAX_CHUNK) {
        const int n = std::min(STAB_MAX_CHUNK, N - c0);
        RM_TRY(stab_sim_warp((const uint8_t *)frames + (size_t)c0 * in_fb, dtype, n, H, W, p + 4 * (size_t)c0, (uint8_t *)out + (size_t)c0 * out_fb, out_dtype, s));
    }
    return RM_OK;
}
