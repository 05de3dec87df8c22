// respmon_amd/csrc/rm_pulse.hip -- the pulse beside the breath: per-channel block and rectangle sums of a BGR buffer, the POS
// projection of those sums, and the pulse map (rm_bgr_block_sums, rm_bgr_roi_sums, rm_pulse_pos, rm_pulse_map)
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_internal.h"
#include "rm_pulse_kernels.h"

using namespace rm;

static bool pulse_block_ok(int block) { return block == 4 || block == 8 || block == 16 || block == 32 || block == 64; }

template <int BLOCK>
static void launch_block_sums(bool fast, const uint8_t *frames, int H, int W, int Hb, int Wb, unsigned rows, uint32_t *sums, hipStream_t s)
{
    const int G = (W + 15) / 16, lanes = Wb * (BLOCK >= 16 ? BLOCK / 16 : 1);   // groups that hold pixels; lanes of a block row (whole blocks)
    const dim3 grid((rows + 3) / 4, (unsigned)((lanes + 63) / 64)), block(64, 4);
    if (fast) hipLaunchKernelGGL((k_bgr_block_sums<BLOCK, true>), grid, block, 0, s, frames, H, W, Hb, Wb, G, rows, sums);
    else hipLaunchKernelGGL((k_bgr_block_sums<BLOCK, false>), grid, block, 0, s, frames, H, W, Hb, Wb, G, rows, sums);
}

// the arguments have been checked (N, H, W >= 1, a block of the list)
static int block_sums(const uint8_t *frames, int N, int H, int W, int block, uint32_t *sums, hipStream_t s, const char *who)
{
    const int Hb = (H + block - 1) / block, Wb = (W + block - 1) / block;
    const size_t rows = (size_t)N * Hb;
    if (rows > 0x7fffffffull || ((size_t)Wb * (block >= 16 ? block / 16 : 1) + 63) / 64 > 65535)
        return fail(RM_E_UNSUPPORTED, "%s: %d frames of %d x %d in blocks of %d exceed the launch grid", who, N, W, H, block);
    const bool fast = W % 16 == 0 && ((uintptr_t)frames & 15) == 0;   // every 16-pixel group of every row is three aligned 16-byte loads
    switch (block) {
    case 4: launch_block_sums<4>(fast, frames, H, W, Hb, Wb, (unsigned)rows, sums, s); break;
    case 8: launch_block_sums<8>(fast, frames, H, W, Hb, Wb, (unsigned)rows, sums, s); break;
    case 16: launch_block_sums<16>(fast, frames, H, W, Hb, Wb, (unsigned)rows, sums, s); break;
    case 32: launch_block_sums<32>(fast, frames, H, W, Hb, Wb, (unsigned)rows, sums, s); break;
    default: launch_block_sums<64>(fast, frames, H, W, Hb, Wb, (unsigned)rows, sums, s); break;
    }
    LAUNCH_CHECK();
    return RM_OK;
}

extern "C" int rm_bgr_block_sums(rm_ctx *ctx, const uint8_t *frames_dev, int N, int H, int W, int block, uint32_t *sums_dev, void *stream)
{
    if (!ctx || !frames_dev || !sums_dev || N < 1 || H < 1 || W < 1 || !pulse_block_ok(block))
        return fail(RM_E_BADARG, "rm_bgr_block_sums: bad argument (N, H, W >= 1, block one of 4, 8, 16, 32, 64)");
    HIP_TRY(hipSetDevice(ctx->device));
    return block_sums(frames_dev, N, H, W, block, sums_dev, (hipStream_t)stream, "rm_bgr_block_sums");
}

extern "C" int rm_bgr_roi_sums(rm_ctx *ctx, const uint8_t *frames_dev, int N, int H, int W, const int32_t *rois_host, int K, uint32_t *sums_dev,
                               void *stream)
{
    if (!ctx || !frames_dev || !rois_host || !sums_dev || N < 1 || H < 1 || W < 1 || K < 1 || K > RM_MAX_ROIS)
        return fail(RM_E_BADARG, "rm_bgr_roi_sums: bad argument (N >= 1, 1 <= K <= %d)", RM_MAX_ROIS);
    PulseRois r;
    memset(&r, 0, sizeof r);
    for (int k = 0; k < K; ++k) {   // the whole call is refused before anything is enqueued
        const int x = rois_host[4 * k], y = rois_host[4 * k + 1], w = rois_host[4 * k + 2], h = rois_host[4 * k + 3];
        if (!(x >= 0 && y >= 0 && w >= 1 && h >= 1 && w <= W - x && h <= H - y))
            return fail(RM_E_BADARG, "rm_bgr_roi_sums: rectangle %d (%d, %d, %d, %d) does not lie inside the %d x %d frame", k, x, y, w, h, W, H);
        if ((unsigned long long)w * h * 255ull >= (1ull << 32))
            return fail(RM_E_UNSUPPORTED, "rm_bgr_roi_sums: rectangle %d (%d x %d) can overflow a 32-bit sum", k, w, h);
        r.v[4 * k] = x; r.v[4 * k + 1] = y; r.v[4 * k + 2] = w; r.v[4 * k + 3] = h;
    }
    if ((long long)N * K > 0x7fffffffll) return fail(RM_E_UNSUPPORTED, "rm_bgr_roi_sums: %d frames x %d rectangles exceed the launch grid", N, K);
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_bgr_roi_sums<>, dim3((unsigned)(N * K)), dim3(256), 0, (hipStream_t)stream, frames_dev, (size_t)H * W * 3, W, r, K, sums_dev);
    LAUNCH_CHECK();
    return RM_OK;
}

static int pulse_pos_args(const char *who, int N, int window)
{
    if (N < 2 || window < 2 || window > N) return fail(RM_E_BADARG, "%s: bad argument (2 <= window <= N)", who);
    if (N > MAX_T) return fail(RM_E_UNSUPPORTED, "%s: N=%d > %d", who, N, MAX_T);
    return RM_OK;
}

// the arguments have been checked; the per-window sums and ratios live in the context's workspace
static int pulse_pos(rm_ctx *ctx, const uint32_t *sums, int N, size_t NP, int window, double *h, hipStream_t s, const char *who)
{
    if (NP == 0) return RM_OK;
    if ((NP + 255) / 256 > 0x7fffffffull) return fail(RM_E_UNSUPPORTED, "%s: %zu columns", who, NP);
    const int NW = N - window + 1;
    double *Sw = nullptr, *alpha = nullptr;
    RM_TRY(ws(ctx, "pulse_Sw", (size_t)NW * NP * 3, &Sw));
    RM_TRY(ws(ctx, "pulse_alpha", (size_t)NW * NP, &alpha));
    const unsigned gx = (unsigned)((NP + 255) / 256);
    hipLaunchKernelGGL(k_pos_windows<>, dim3(gx, (unsigned)NW), dim3(256), 0, s, sums, NP, window, Sw, alpha);
    hipLaunchKernelGGL(k_pos_overlap_add<>, dim3(gx, (unsigned)N), dim3(256), 0, s, sums, N, NP, window, (const double *)Sw, (const double *)alpha, h);
    LAUNCH_CHECK();
    return RM_OK;
}

extern "C" int rm_pulse_pos(rm_ctx *ctx, const uint32_t *sums_dev, int N, size_t NP, int window, double *h_dev, void *stream)
{
    if (!ctx || !sums_dev || !h_dev) return fail(RM_E_BADARG, "rm_pulse_pos: NULL argument");
    RM_TRY(pulse_pos_args("rm_pulse_pos", N, window));
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    return pulse_pos(ctx, sums_dev, N, NP, window, h_dev, (hipStream_t)stream, "rm_pulse_pos");
}

extern "C" int rm_pulse_map(rm_ctx *ctx, const uint8_t *frames_dev, int N, int H, int W, int block, int window, double fps, double fmin, double fmax,
                            int nfreq, double *freq_dev, double *power_dev, double *total_dev, int32_t *index_dev, void *stream)
{
    // (the band's conditions are rate_peak's, written so that a NaN anywhere fails them)
    if (!ctx || !frames_dev || N < 2 || H < 1 || W < 1 || !pulse_block_ok(block) || window < 2 || window > N || nfreq < 3 || nfreq > 64 ||
        !(fmin > 0.0 && fmin < fmax && fmax <= fps / 2) || (!freq_dev && !power_dev && !total_dev && !index_dev))
        return fail(RM_E_BADARG, "rm_pulse_map: bad argument (N >= 2, block one of 4, 8, 16, 32, 64, 2 <= window <= N, 3 <= nfreq <= 64, "
                                 "0 < freq_min < freq_max <= fps / 2, at least one output)");
    if (N > MAX_T) return fail(RM_E_UNSUPPORTED, "rm_pulse_map: N=%d > %d", N, MAX_T);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    const size_t NP = (size_t)((H + block - 1) / block) * (size_t)((W + block - 1) / block);
    uint32_t *sums = nullptr;
    double *h = nullptr;
    RM_TRY(ws(ctx, "pulse_sums", (size_t)N * NP * 3, &sums));
    RM_TRY(ws(ctx, "pulse_h", (size_t)N * NP, &h));
    RM_TRY(block_sums(frames_dev, N, H, W, block, sums, s, "rm_pulse_map"));
    RM_TRY(pulse_pos(ctx, sums, N, NP, window, h, s, "rm_pulse_map"));
    return rate_peak(ctx, h, N, NP, 0, fps, fmin, fmax, nfreq, freq_dev, power_dev, total_dev, index_dev, s, "rm_pulse_map");
}
