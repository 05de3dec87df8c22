// respmon_amd/csrc/rm_magnify.hip -- rm_magnify, rm_magnify_bgr: the magnified video, frames + band-passed motion, in one fused pass (rm_magnify.h;
// transforms.py:170 adds the band-passed levels into the video pyramid, transforms.py:181 is the commented-out collapse of it)
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_internal.h"
#include "rm_magnify.h"

using namespace rm;

namespace {

struct MagCall {
    const void *frames; void *out;
    int T, H, W;
    hipStream_t s;
};

// SYM = 1: rm_magnify / rm_magnify_bgr (cS / raw hold the unique frames of a signal even in time); SYM = 0: a row per frame (magnify_rows)
template <int S, typename Tin, typename Tout, int SYM>
int launch_fused(const MagCall &c, const double *cS, const ChainGeom &g)
{
    using G = MagGeom<Tin, Tout>;
    const int ntiles = g.tiles_x * g.tiles_y, nchunks = ((SYM ? sym_frames(c.T) : c.T) + MAG_FC - 1) / MAG_FC;
    const int vec = ((((uintptr_t)c.frames | (uintptr_t)c.out) & 15) == 0 && c.W % G::V == 0) ? 1 : 0;
    hipLaunchKernelGGL((k_magnify<S, Tin, Tout, SYM>), dim3((unsigned)(ntiles * nchunks)), dim3(64), sizeof(double) * MAG_LDS_DOUBLES, c.s, cS, g, c.T, ntiles,
                       (const Tin *)c.frames, (Tout *)c.out, vec);
    LAUNCH_CHECK();
    return RM_OK;
}

template <typename Tin, typename Tout, int SYM = 1>
int launch_any(const MagCall &c, const double *cS, const ChainGeom *g, const double *raw)
{
    if (g) {
        switch (g->S) {
        case 1: return launch_fused<1, Tin, Tout, SYM>(c, cS, *g);
        case 2: return launch_fused<2, Tin, Tout, SYM>(c, cS, *g);
        case 3: return launch_fused<3, Tin, Tout, SYM>(c, cS, *g);
        default: return launch_fused<4, Tin, Tout, SYM>(c, cS, *g);
        }
    }
    const size_t npix = (size_t)c.H * c.W;
    hipLaunchKernelGGL((k_magnify_plain<Tin, Tout, SYM>), dim3(nblk(npix, 256, 4096), (unsigned)c.T), dim3(256), 0, c.s, (const Tin *)c.frames, raw, c.T, npix,
                       (Tout *)c.out);
    LAUNCH_CHECK();
    return RM_OK;
}

template <typename Tin, int SYM = 1>
int launch_out(const MagCall &c, int out_dtype, const double *cS, const ChainGeom *g, const double *raw)
{
    switch (out_dtype) {
    case RM_U8: return launch_any<Tin, uint8_t, SYM>(c, cS, g, raw);
    case RM_U16: return launch_any<Tin, uint16_t, SYM>(c, cS, g, raw);
    case RM_F32: return launch_any<Tin, float, SYM>(c, cS, g, raw);
    default: return launch_any<Tin, double, SYM>(c, cS, g, raw);
    }
}

template <int SYM = 1>
int launch_in(const MagCall &c, int dtype, int out_dtype, const double *cS, const ChainGeom *g, const double *raw)
{
    switch (dtype) {
    case RM_U8: return launch_out<uint8_t, SYM>(c, out_dtype, cS, g, raw);
    case RM_U16: return launch_out<uint16_t, SYM>(c, out_dtype, cS, g, raw);
    case RM_F16: return launch_out<__half, SYM>(c, out_dtype, cS, g, raw);
    case RM_F32: return launch_out<float, SYM>(c, out_dtype, cS, g, raw);
    case RM_F64: return launch_out<double, SYM>(c, out_dtype, cS, g, raw);
    default: return launch_out<bgr8_t, SYM>(c, out_dtype, cS, g, raw);
    }
}

// behind the collapse to level S, `rows` frames of C_S (the unique frames of rm_magnify, every frame of a stream chunk): launch(cS,
// geometry, raw) with nothing filtered (all null: raw == 0), the level-S signal and the geometry of the fused kernel (1 <= S <= 4 where
// TileEval applies), or the materialised rows of raw
template <typename Launch>
int magnify_tail(rm_ctx *ctx, const MagCall &c, const SmallLevels &sl, int rows, Launch launch)
{
    if (sl.all_zero) return launch(nullptr, nullptr, nullptr);   // nothing is filtered: raw == 0
    const int Th = rows;
    if (sl.S >= 1 && sl.S <= 4) {
        ChainGeom g;
        RM_TRY(make_geom(sl, g));
        if (tile_eval_ok(g) && (long long)g.tiles_x * g.tiles_y * ((Th + MAG_FC - 1) / MAG_FC) < (1ll << 31))
            return launch(sl.cS, &g, nullptr);
    }
    // every other shape: the materialised collapse of the unique frames (as rm_eulerian_magnification_bandpass forms raw), then the sum
    const double *cur = sl.cS;
    for (int l = sl.S - 1; l >= 0; --l) {
        double *dst = nullptr;
        RM_TRY(ws(ctx, l == 0 ? "magnify_raw" : ((l & 1) ? "collapse_a" : "collapse_b"), (size_t)Th * sl.h[l] * sl.w[l], &dst));
        RM_TRY(launch_pyr_up(cur, Th, sl.h[l + 1], sl.w[l + 1], dst, sl.h[l], sl.w[l], 0, nullptr, c.s));
        cur = dst;
    }
    return launch(nullptr, nullptr, cur);
}

template <typename Launch>
int magnify_dispatch(rm_ctx *ctx, const MagCall &c, int dtype, double fps, double fmin, double fmax, double amp, int levels, int skip, Launch launch)
{
    SmallLevels sl;
    RM_TRY(front_half(ctx, c.frames, dtype, c.T, c.H, c.W, fps, fmin, fmax, amp, levels, skip, 0, sl, c.s));
    return magnify_tail(ctx, c, sl, sym_frames(c.T), launch);
}

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

}  // namespace

// out[t] = convert(f[t] + pyrUp^S(C_S[t])) for the n frames of a stream chunk, C_S[t] = sl.cS + t * h_S * w_S (rm_stream.hip): the
// dispatch of magnify_dispatch with a row of C_S per frame.  out_dtype RM_BGR8: the colour rule of rm_magnify_bgr (dtype RM_BGR8 only).
int magnify_rows(rm_ctx *ctx, const void *frames, int dtype, int n, int H, int W, const SmallLevels &sl, void *out, int out_dtype, hipStream_t s)
{
    const MagCall c{frames, out, n, H, W, s};
    if (out_dtype == RM_BGR8)
        return magnify_tail(ctx, c, sl, n, [&](const double *cS, const ChainGeom *g, const double *raw) { return launch_any<bgr8_t, bgr8_t, 0>(c, cS, g, raw); });
    return magnify_tail(ctx, c, sl, n, [&](const double *cS, const ChainGeom *g, const double *raw) { return launch_in<0>(c, dtype, out_dtype, cS, g, raw); });
}

extern "C" int rm_magnify(rm_ctx *ctx, const void *frames, int dtype, int T, int H, int W, double fps, double fmin, double fmax, double amp,
                          int levels, int skip, void *out, int out_dtype, void *stream)
{
    if (!ctx || !frames || !out || T < 1 || H < 1 || W < 1 || levels < 1 || skip < 0 || !(fps > 0) || !valid_buffer_dtype(dtype))
        return fail(RM_E_BADARG, "rm_magnify: bad argument");
    if (out_dtype != RM_U8 && out_dtype != RM_U16 && out_dtype != RM_F32 && out_dtype != RM_F64)
        return fail(RM_E_BADARG, "rm_magnify: out_dtype %d (RM_U8, RM_U16, RM_F32 or RM_F64)", out_dtype);
    if (T > MAX_T) return fail(RM_E_UNSUPPORTED, "rm_magnify: T=%d > %d", T, MAX_T);
    const size_t n = (size_t)T * H * W;
    if (ranges_overlap(frames, n * dtype_size(dtype), out, n * dtype_size(out_dtype))) return fail(RM_E_BADARG, "rm_magnify: out_dev overlaps the frame buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    const MagCall c{frames, out, T, H, W, (hipStream_t)stream};
    return magnify_dispatch(ctx, c, dtype, fps, fmin, fmax, amp, levels, skip,
                            [&](const double *cS, const ChainGeom *g, const double *raw) { return launch_in<1>(c, dtype, out_dtype, cS, g, raw); });
}

// the colour form: BGR frames in, BGR video out, the same raw onto the three channels (rm_magnify.h)
extern "C" int rm_magnify_bgr(rm_ctx *ctx, const uint8_t *frames, int T, int H, int W, double fps, double fmin, double fmax, double amp, int levels,
                              int skip, uint8_t *out, void *stream)
{
    if (!ctx || !frames || !out || T < 1 || H < 1 || W < 1 || levels < 1 || skip < 0 || !(fps > 0)) return fail(RM_E_BADARG, "rm_magnify_bgr: bad argument");
    if (T > MAX_T) return fail(RM_E_UNSUPPORTED, "rm_magnify_bgr: T=%d > %d", T, MAX_T);
    const size_t n = (size_t)T * H * W * sizeof(bgr8_t);
    if (ranges_overlap(frames, n, out, n)) return fail(RM_E_BADARG, "rm_magnify_bgr: out_dev overlaps the frame buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    const MagCall c{frames, out, T, H, W, (hipStream_t)stream};
    return magnify_dispatch(ctx, c, RM_BGR8, fps, fmin, fmax, amp, levels, skip,
                            [&](const double *cS, const ChainGeom *g, const double *raw) { return launch_any<bgr8_t, bgr8_t>(c, cS, g, raw); });
}
