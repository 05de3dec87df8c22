// respmon_amd/csrc/rm_stream.hip -- rm_sosfilt, rm_stream_*: the causal band-pass as a cascade of second-order sections with carried
// state (rm_stream_kernels.h), and a live stream magnified chunk by chunk on it: O(1) per frame, no [T,H,W] buffer, the result
// independent of how the stream was cut into calls.
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_internal.h"
#include "rm_stream_kernels.h"

using namespace rm;

// sos_host[nsec][6] = (b0, b1, b2, a0, a1, a2) as scipy.signal.butter(..., output='sos') lays them out; zi_host[nsec][2] or null
static int sos_coef(const char *who, const double *sos_host, int nsec, const double *zi_host, SosCoef &c)
{
    if (!sos_host || nsec < 1) return fail(RM_E_BADARG, "%s: bad argument (nsec >= 1 sections)", who);
    if (nsec > SOS_MAX) return fail(RM_E_UNSUPPORTED, "%s: %d sections > %d", who, nsec, SOS_MAX);
    for (int s = 0; s < SOS_MAX; ++s) {
        const bool on = s < nsec;
        const double *q = sos_host + 6 * (on ? s : 0);
        if (on && q[3] != 1.0) return fail(RM_E_BADARG, "%s: a0 of section %d is %g (sections must be normalised: a0 == 1)", who, s, q[3]);
        c.b0[s] = on ? q[0] : 0.0; c.b1[s] = on ? q[1] : 0.0; c.b2[s] = on ? q[2] : 0.0;
        c.a1[s] = on ? q[4] : 0.0; c.a2[s] = on ? q[5] : 0.0;
        c.zi[s][0] = (on && zi_host) ? zi_host[2 * s] : 0.0;
        c.zi[s][1] = (on && zi_host) ? zi_host[2 * s + 1] : 0.0;
    }
    c.n = nsec;
    return RM_OK;
}

extern "C" int rm_sosfilt(rm_ctx *ctx, const double *data, int T, size_t npix, const double *sos_host, int nsec, const double *zi_host,
                          double scale, double *out, void *stream)
{
    if (!ctx || !data || !out || T < 1) return fail(RM_E_BADARG, "rm_sosfilt: bad argument");
    SosCoef c;
    RM_TRY(sos_coef("rm_sosfilt", sos_host, nsec, zi_host, c));
    if (npix == 0) return RM_OK;
    if (data == out) return fail(RM_E_BADARG, "rm_sosfilt: in-place filtering is not supported");
    HIP_TRY(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((npix + 63) / 64)), block(64);
    if (zi_host) hipLaunchKernelGGL((k_sosfilt<0, 1>), grid, block, 0, (hipStream_t)stream, data, T, npix, c, scale, out, (double *)nullptr);
    else hipLaunchKernelGGL((k_sosfilt<0, 0>), grid, block, 0, (hipStream_t)stream, data, T, npix, c, scale, out, (double *)nullptr);
    LAUNCH_CHECK();
    return RM_OK;
}

// The state of a stream: z[nsec][2][NP] float64, NP the Laplacian levels S .. L-2 of a frame side by side (what front_pyramid writes
// under RM_FLAG_FILTER_LAPLACIANS).  Its own allocation: it has to survive every other call on the context, like the window's ring.
struct rm_stream {
    int device = 0;
    int H = 0, W = 0, levels = 0, skip = 0;
    unsigned flags = RM_FLAG_FILTER_LAPLACIANS;   // the reference's operation order: Laplacians first, then the filter (transforms.py:148-170)
    PyrGeom pg;
    size_t NP = 0;            // 0: nothing is filtered (skip >= levels - 1), no state
    SosCoef coef;
    bool steady = false;      // zi given: the first frame of the stream sets z = zi * x[0]
    double amp = 0;
    double *z = nullptr;
    long long seen = 0;       // frames pushed since creation or the last reset
};

constexpr long long STREAM_CHUNK_BYTES = 256ll << 20;   // workspace cap of one internal chunk of rm_stream_push
constexpr int STREAM_CHUNK_FRAMES = 256;

extern "C" int rm_stream_create(rm_ctx *ctx, int H, int W, int levels, int skip, const double *sos_host, int nsec, const double *zi_host,
                                double amp, rm_stream **out)
{
    if (out) *out = nullptr;
    if (!ctx || !out || H < 1 || W < 1 || levels < 1 || skip < 0) return fail(RM_E_BADARG, "rm_stream_create: bad argument");
    SosCoef c;
    RM_TRY(sos_coef("rm_stream_create", sos_host, nsec, zi_host, c));
    HIP_TRY(hipSetDevice(ctx->device));
    rm_stream *st = new rm_stream;
    st->device = ctx->device;
    st->H = H; st->W = W; st->levels = levels; st->skip = skip;
    st->coef = c; st->steady = zi_host != nullptr; st->amp = amp;
    pyr_geom(H, W, levels, skip, st->flags, st->pg);
    st->NP = st->pg.all_zero ? 0 : st->pg.NP;
    if (st->NP) {
        const size_t bytes = sizeof(double) * 2 * (size_t)nsec * st->NP;
        hipError_t e = hipMalloc((void **)&st->z, bytes);
        if (e != hipSuccess) {
            delete st;
            return fail(RM_E_HIP, "rm_stream_create: %zu bytes for the filter state: %s", bytes, hipGetErrorString(e));
        }
    }
    *out = st;
    return RM_OK;
}

extern "C" int rm_stream_destroy(rm_stream *st)
{
    if (!st) return RM_OK;
    (void)hipSetDevice(st->device);
    if (st->z) (void)hipFree(st->z);   // (synchronises with the work that still uses the state)
    delete st;
    return RM_OK;
}

extern "C" int rm_stream_reset(rm_ctx *ctx, rm_stream *st)
{
    if (!ctx || !st) return fail(RM_E_BADARG, "rm_stream_reset: bad argument");
    st->seen = 0;   // the next push starts the state again, in stream order
    return RM_OK;
}

extern "C" int rm_stream_info(const rm_stream *st, long long *frames_seen, size_t *np, size_t *state_bytes)
{
    if (!st) return fail(RM_E_BADARG, "rm_stream_info: bad argument");
    if (frames_seen) *frames_seen = st->seen;
    if (np) *np = st->NP;
    if (state_bytes) *state_bytes = sizeof(double) * 2 * (size_t)st->coef.n * st->NP;
    return RM_OK;
}

static bool stream_ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

// one internal chunk: m frames -> Laplacian rows -> band-passed rows (the state moves on) -> C_S[m] -> the sum kernel
static int stream_chunk(rm_ctx *ctx, rm_stream *st, const void *frames, int dtype, int m, void *out, int out_dtype, hipStream_t s)
{
    SmallLevels sl;
    sl.h = st->pg.h; sl.w = st->pg.w;
    if (!st->NP) {   // nothing is filtered: the conversion alone
        sl.all_zero = true;
        return magnify_rows(ctx, frames, dtype, m, st->H, st->W, sl, out, out_dtype, s);
    }
    const size_t NP = st->NP;
    double *lap = nullptr, *bp = nullptr;
    RM_TRY(ws(ctx, "stream_lap", (size_t)m * NP, &lap));
    RM_TRY(ws(ctx, "stream_bp", (size_t)m * NP, &bp));
    RM_TRY(front_pyramid(ctx, frames, dtype, m, st->H, st->W, st->pg, st->flags, lap, s));
    const bool state_fresh = ctx->state_fresh;
    ctx->state_fresh = false;   // the collapse below reduces into d_state
    const dim3 grid((unsigned)((NP + 63) / 64)), block(64);
    if (st->seen == 0 && st->steady) {
        hipLaunchKernelGGL((k_sosfilt<1, 1>), grid, block, 0, s, (const double *)lap, m, NP, st->coef, st->amp, bp, st->z);
    } else {
        if (st->seen == 0) HIP_TRY(hipMemsetAsync(st->z, 0, sizeof(double) * 2 * (size_t)st->coef.n * NP, s));   // from rest
        hipLaunchKernelGGL((k_sosfilt<1, 0>), grid, block, 0, s, (const double *)lap, m, NP, st->coef, st->amp, bp, st->z);
    }
    LAUNCH_CHECK();
    RM_TRY(collapse_levels(ctx, bp, m, st->pg, state_fresh, false, sl, s));
    return magnify_rows(ctx, frames, dtype, m, st->H, st->W, sl, out, out_dtype, s);
}

extern "C" int rm_stream_push(rm_ctx *ctx, rm_stream *st, const void *frames, int dtype, int n, void *out, int out_dtype, void *stream)
{
    if (!ctx || !st || !frames || !out || n < 1 || !valid_buffer_dtype(dtype)) return fail(RM_E_BADARG, "rm_stream_push: bad argument");
    if (out_dtype != RM_U8 && out_dtype != RM_U16 && out_dtype != RM_F32 && out_dtype != RM_F64 && out_dtype != RM_BGR8)
        return fail(RM_E_BADARG, "rm_stream_push: out_dtype %d (RM_U8, RM_U16, RM_F32, RM_F64 or RM_BGR8)", out_dtype);
    if (out_dtype == RM_BGR8 && dtype != RM_BGR8) return fail(RM_E_BADARG, "rm_stream_push: RM_BGR8 output needs RM_BGR8 frames");
    if (ctx->device != st->device) return fail(RM_E_BADARG, "rm_stream_push: the stream belongs to device %d", st->device);
    const size_t npix = (size_t)st->H * st->W, in_fb = npix * dtype_size(dtype), out_fb = npix * dtype_size(out_dtype);
    if (stream_ranges_overlap(frames, (size_t)n * in_fb, out, (size_t)n * out_fb)) return fail(RM_E_BADARG, "rm_stream_push: out_dev overlaps the frames");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    // n is unbounded for the caller: internal chunks sized by the workspace they need (Laplacian and band-passed rows, C_S, and the
    // materialised raw where the fused sum kernel does not apply)
    const PyrGeom &pg = st->pg;
    const bool fused = st->NP && pg.S >= 1 && pg.S <= 4;
    const long long per_frame = st->NP ? 8ll * (long long)(2 * st->NP + (size_t)pg.h[pg.S] * pg.w[pg.S] + (fused ? 0 : 2 * npix)) : 1;
    long long cap = std::max(1ll, std::min((long long)STREAM_CHUNK_FRAMES, STREAM_CHUNK_BYTES / per_frame));
    if (ctx->dbg.stream_frames > 0) cap = ctx->dbg.stream_frames;
    for (int done = 0; done < n;) {
        const int m = (int)std::min<long long>(cap, n - done);
        RM_TRY(stream_chunk(ctx, st, (const uint8_t *)frames + (size_t)done * in_fb, dtype, m, (uint8_t *)out + (size_t)done * out_fb, out_dtype, s));
        st->seen += m;
        done += m;
    }
    return RM_OK;
}
