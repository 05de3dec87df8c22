// respmon_amd/csrc/rm_phase.hip -- rm_phase_*: phase-based motion magnification on the Riesz pyramid (Wadhwa, Rubinstein, Durand, Freeman,
// "Riesz Pyramids for Fast Phase-Based Video Magnification", ICCP 2014), a stream object like rm_stream: frame-to-frame phase
// differences, a running sum, the causal band-pass of rm_sosfilt on it, an amplitude-weighted blur and a phase shift of every
// processed Laplacian level (rm_phase_kernels.h; the rule: include/respmon_hip.h).
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_internal.h"
#include "rm_phase_kernels.h"

using namespace rm;

// The state of a phase stream: [5 + 4 nsec][NP] float64 -- Ip, R1p, R2p, Pc, Ps, then z[nsec][2] of the cosine and of the sine channel --,
// NP the processed levels S .. L-2 of a frame side by side.  Its own allocation: it survives every other call on the context.
struct rm_phase {
    int device = 0;
    int H = 0, W = 0, levels = 0, skip = 0;
    unsigned flags = 0;
    std::vector<int> h, w;    // every pyramid level
    size_t NA = 0;            // pixels of all levels of a frame
    size_t NP = 0;            // pixels of the processed levels; 0: nothing is processed (skip >= levels - 1)
    PhaseGeom g;
    SosCoef coef;
    double amp = 0;
    double *state = nullptr;
    long long seen = 0;       // frames pushed since creation or the last reset
};

constexpr long long PHASE_CHUNK_BYTES = 2048ll << 20;   // workspace cap of one internal chunk of rm_phase_push
constexpr int PHASE_CHUNK_FRAMES = 256;

// rm_sosfilt's argument checks (rm_stream.hip sos_coef) for a filter that always starts from rest
static int phase_sos_coef(const double *sos_host, int nsec, SosCoef &c)
{
    if (!sos_host || nsec < 1) return fail(RM_E_BADARG, "rm_phase_create: bad argument (nsec >= 1 sections)");
    if (nsec > SOS_MAX) return fail(RM_E_UNSUPPORTED, "rm_phase_create: %d sections > %d", nsec, SOS_MAX);
    for (int s = 0; s < SOS_MAX; ++s) {
        const bool on = s < nsec;
        const double *q = sos_host + 6 * (on ? s : 0);
        if (on && q[3] != 1.0) return fail(RM_E_BADARG, "rm_phase_create: a0 of section %d is %g (sections must be normalised: a0 == 1)", s, q[3]);
        c.b0[s] = on ? q[0] : 0.0; c.b1[s] = on ? q[1] : 0.0; c.b2[s] = on ? q[2] : 0.0;
        c.a1[s] = on ? q[4] : 0.0; c.a2[s] = on ? q[5] : 0.0;
        c.zi[s][0] = 0.0; c.zi[s][1] = 0.0;
    }
    c.n = nsec;
    return RM_OK;
}

static size_t phase_state_doubles(const rm_phase *ph) { return (size_t)(5 + 4 * ph->coef.n) * ph->NP; }

extern "C" int rm_phase_create(rm_ctx *ctx, int H, int W, int levels, int skip, const double *sos_host, int nsec, double amp, unsigned flags,
                               rm_phase **out)
{
    if (out) *out = nullptr;
    if (!ctx || !out || H < 1 || W < 1 || levels < 1 || skip < 0) return fail(RM_E_BADARG, "rm_phase_create: bad argument");
    if (flags & ~RM_PHASE_NO_BLUR) return fail(RM_E_BADARG, "rm_phase_create: unknown flags 0x%x", flags);
    SosCoef c;
    RM_TRY(phase_sos_coef(sos_host, nsec, c));
    const int nl = std::max(0, levels - 1 - skip);
    if (nl > PHASE_MAX_LEVELS) return fail(RM_E_UNSUPPORTED, "rm_phase_create: %d processed levels > %d", nl, PHASE_MAX_LEVELS);
    HIP_TRY(hipSetDevice(ctx->device));
    rm_phase *ph = new rm_phase;
    ph->device = ctx->device;
    ph->H = H; ph->W = W; ph->levels = levels; ph->skip = skip; ph->flags = flags;
    ph->coef = c; ph->amp = amp;
    level_sizes(H, W, levels, ph->h, ph->w);
    for (int l = 0; l < levels; ++l) ph->NA += (size_t)ph->h[l] * ph->w[l];
    PhaseGeom &g = ph->g;
    memset(&g, 0, sizeof(g));
    g.nl = nl;
    unsigned long long tb = 0, sb = 0;
    for (int i = 0; i < nl; ++i) {
        const int h = ph->h[skip + i], w = ph->w[skip + i];
        g.h[i] = h; g.w[i] = w; g.off[i] = ph->NP;
        g.tb0[i] = (unsigned)tb; g.sb0[i] = (unsigned)sb;
        tb += (unsigned long long)h * ((w + 63) / 64);
        sb += (unsigned long long)((h + PH_TH - 1) / PH_TH) * ((w + PH_TW - 1) / PH_TW);
        ph->NP += (size_t)h * w;
    }
    if (tb >= (1ull << 31)) { delete ph; return fail(RM_E_UNSUPPORTED, "rm_phase_create: %d x %d frames are too large", H, W); }
    for (int i = nl; i <= PHASE_MAX_LEVELS; ++i) { g.tb0[i] = (unsigned)tb; g.sb0[i] = (unsigned)sb; }
    if (ph->NP) {
        const size_t bytes = sizeof(double) * phase_state_doubles(ph);
        hipError_t e = hipMalloc((void **)&ph->state, bytes);
        if (e != hipSuccess) {
            delete ph;
            return fail(RM_E_HIP, "rm_phase_create: %zu bytes for the state: %s", bytes, hipGetErrorString(e));
        }
    }
    *out = ph;
    return RM_OK;
}

extern "C" int rm_phase_destroy(rm_phase *ph)
{
    if (!ph) return RM_OK;
    (void)hipSetDevice(ph->device);
    if (ph->state) (void)hipFree(ph->state);   // (synchronises with the work that still uses the state)
    delete ph;
    return RM_OK;
}

extern "C" int rm_phase_reset(rm_ctx *ctx, rm_phase *ph)
{
    if (!ctx || !ph) return fail(RM_E_BADARG, "rm_phase_reset: bad argument");
    ph->seen = 0;   // the next push starts the state again, in stream order
    return RM_OK;
}

extern "C" int rm_phase_info(const rm_phase *ph, long long *frames_seen, size_t *np, size_t *state_bytes)
{
    if (!ph) return fail(RM_E_BADARG, "rm_phase_info: bad argument");
    if (frames_seen) *frames_seen = ph->seen;
    if (np) *np = ph->NP;
    if (state_bytes) *state_bytes = sizeof(double) * phase_state_doubles(ph);
    return RM_OK;
}

template <bool BLUR>
static int phase_launch_time(const rm_phase *ph, const double *lap, int m, bool first, double *pa, double *pb, double *pc, hipStream_t s)
{
    const PhaseGeom &g = ph->g;
    const dim3 grid(g.tb0[g.nl]), block(64);
    const int f = first ? 1 : 0;
    switch (ph->coef.n) {
    case 1: hipLaunchKernelGGL((k_phase_time<1, BLUR>), grid, block, 0, s, lap, m, g, ph->NP, ph->coef, f, pa, pb, pc, ph->state); break;
    case 2: hipLaunchKernelGGL((k_phase_time<2, BLUR>), grid, block, 0, s, lap, m, g, ph->NP, ph->coef, f, pa, pb, pc, ph->state); break;
    case 3: hipLaunchKernelGGL((k_phase_time<3, BLUR>), grid, block, 0, s, lap, m, g, ph->NP, ph->coef, f, pa, pb, pc, ph->state); break;
    case 4: hipLaunchKernelGGL((k_phase_time<4, BLUR>), grid, block, 0, s, lap, m, g, ph->NP, ph->coef, f, pa, pb, pc, ph->state); break;
    default: hipLaunchKernelGGL((k_phase_time<8, BLUR>), grid, block, 0, s, lap, m, g, ph->NP, ph->coef, f, pa, pb, pc, ph->state); break;
    }
    LAUNCH_CHECK();
    return RM_OK;
}

template <typename Tout>
static int phase_launch_convert(const double *v, size_t count, void *out, hipStream_t s)
{
    hipLaunchKernelGGL((k_phase_convert<Tout>), dim3(nblk(count, 256, 16384)), dim3(256), 0, s, v, count, (Tout *)out);
    LAUNCH_CHECK();
    return RM_OK;
}

// one internal chunk: m frames -> Laplacian pyramid -> time kernel (the state moves on) -> space kernel -> collapse -> conversion.
// The number of launches depends on the pyramid alone, not on m.
static int phase_chunk(rm_ctx *ctx, rm_phase *ph, const void *frames, int dtype, int m, void *out, int out_dtype, hipStream_t s)
{
    const int L = ph->levels, S = ph->skip;
    const std::vector<int> &h = ph->h, &w = ph->w;
    double *pyr = nullptr;
    RM_TRY(ws(ctx, "phase_pyr", (size_t)m * ph->NA, &pyr));
    std::vector<double *> lv(L);
    {
        size_t o = 0;
        for (int l = 0; l < L; ++l) { lv[l] = pyr + (size_t)m * o; o += (size_t)h[l] * w[l]; }
    }
    // rm_create_laplacian_video_pyramid's launches (rm_pyramid.hip): the Gaussian chain into the level arrays, then L_l = G_l - pyrUp(G_l+1) in place
    RM_TRY(launch_to_f64(frames, dtype, (size_t)m * h[0] * w[0], lv[0], s));
    for (int l = 1; l < L; ++l) RM_TRY(launch_pyr_down(lv[l - 1], RM_F64, m, h[l - 1], w[l - 1], lv[l], s));
    for (int l = 0; l + 1 < L; ++l) RM_TRY(launch_pyr_up(lv[l + 1], m, h[l + 1], w[l + 1], lv[l], h[l], w[l], 1, lv[l], s));
    double *lp = nullptr;
    if (ph->NP) {
        const bool blur = !(ph->flags & RM_PHASE_NO_BLUR);
        double *pa = nullptr, *pb = nullptr, *pc = nullptr;
        if (blur) RM_TRY(ws(ctx, "phase_a", (size_t)m * ph->NP, &pa));
        RM_TRY(ws(ctx, "phase_c", (size_t)m * ph->NP, &pb));
        RM_TRY(ws(ctx, "phase_s", (size_t)m * ph->NP, &pc));
        RM_TRY(ws(ctx, "phase_out", (size_t)m * ph->NP, &lp));
        const double *lap = lv[S];   // the processed levels are contiguous in phase_pyr: level S + i at m * g.off[i] behind lv[S]
        const dim3 grid(ph->g.sb0[ph->g.nl], (unsigned)m), block(PH_THREADS);
        if (blur) {
            HIP_TRY(hipFuncSetAttribute((const void *)k_phase_space<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * PH_LDS_DOUBLES)));   // 76.5 KB: beyond the 64 KB a launch gets unasked
            RM_TRY(phase_launch_time<true>(ph, lap, m, ph->seen == 0, pa, pb, pc, s));
            hipLaunchKernelGGL((k_phase_space<true>), grid, block, sizeof(double) * PH_LDS_DOUBLES, s, lap, m, ph->g, ph->amp, (const double *)pa,
                               (const double *)pb, (const double *)pc, lp);
        } else {
            RM_TRY(phase_launch_time<false>(ph, lap, m, ph->seen == 0, pa, pb, pc, s));
            hipLaunchKernelGGL((k_phase_space<false>), grid, block, 0, s, lap, m, ph->g, ph->amp, (const double *)pa, (const double *)pb,
                               (const double *)pc, lp);
        }
        LAUNCH_CHECK();
    }
    // rm_collapse_laplacian_video_pyramid's rule on L': cur = pyrUp(cur) + L'_l from the coarsest level down, each level summed in place
    double *cur = lv[L - 1];
    for (int l = L - 2; l >= 0; --l) {
        double *dst = (lp && l >= S) ? lp + (size_t)m * ph->g.off[l - S] : lv[l];
        RM_TRY(launch_pyr_up(cur, m, h[l + 1], w[l + 1], dst, h[l], w[l], 2, dst, s));
        cur = dst;
    }
    const size_t count = (size_t)m * ph->H * ph->W;
    switch (out_dtype) {
    case RM_U8: return phase_launch_convert<uint8_t>(cur, count, out, s);
    case RM_U16: return phase_launch_convert<uint16_t>(cur, count, out, s);
    case RM_F32: return phase_launch_convert<float>(cur, count, out, s);
    default: return phase_launch_convert<double>(cur, count, out, s);
    }
}

static bool phase_ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

extern "C" int rm_phase_push(rm_ctx *ctx, rm_phase *ph, const void *frames, int dtype, int n, void *out, int out_dtype, void *stream)
{
    if (!ctx || !ph || !frames || !out || n < 1) return fail(RM_E_BADARG, "rm_phase_push: bad argument");
    if (dtype == RM_BGR8) return fail(RM_E_UNSUPPORTED, "rm_phase_push: RM_BGR8 frames (colour is not supported: convert with rm_bgr_to_gray)");
    if (!valid_dtype(dtype)) return fail(RM_E_BADARG, "rm_phase_push: dtype %d", dtype);
    if (out_dtype != RM_U8 && out_dtype != RM_U16 && out_dtype != RM_F32 && out_dtype != RM_F64)
        return fail(RM_E_BADARG, "rm_phase_push: out_dtype %d (RM_U8, RM_U16, RM_F32 or RM_F64)", out_dtype);
    if (ctx->device != ph->device) return fail(RM_E_BADARG, "rm_phase_push: the object belongs to device %d", ph->device);
    const size_t npix = (size_t)ph->H * ph->W, in_fb = npix * dtype_size(dtype), out_fb = npix * dtype_size(out_dtype);
    if (phase_ranges_overlap(frames, (size_t)n * in_fb, out, (size_t)n * out_fb)) return fail(RM_E_BADARG, "rm_phase_push: out_dev overlaps the frames");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    // n is unbounded for the caller: internal chunks sized by the workspace they need (the pyramid and four planes of the processed levels)
    const long long per_frame = 8ll * (long long)(ph->NA + 4 * ph->NP);
    long long cap = std::max(1ll, std::min((long long)PHASE_CHUNK_FRAMES, PHASE_CHUNK_BYTES / per_frame));
    if (ctx->dbg.stream_frames > 0) cap = ctx->dbg.stream_frames;
    for (int done = 0; done < n;) {
        const int m = (int)std::min<long long>(cap, n - done);
        RM_TRY(phase_chunk(ctx, ph, (const uint8_t *)frames + (size_t)done * in_fb, dtype, m, (uint8_t *)out + (size_t)done * out_fb, out_dtype, s));
        ph->seen += m;
        done += m;
    }
    return RM_OK;
}
