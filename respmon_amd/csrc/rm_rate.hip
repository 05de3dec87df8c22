// respmon_amd/csrc/rm_rate.hip -- the rate map: dominant in-band frequency and its share of the band's power for every pixel column
// (rm_spectral_operator, rm_spectral_peak, rm_rate_map; rm_window_rate_map in rm_window.hip calls rate_peak)
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_internal.h"
#include "rm_rate_kernels.h"

using namespace rm;

static bool rate_band_ok(double fps, double fmin, double fmax)
{
    return fmin > 0.0 && fmin < fmax && fmax <= fps / 2;   // (false for a NaN anywhere)
}

// The estimator of the reference's prototypes/temporal_analysis.py on a fine frequency grid instead of the FFT bins:
//   E[2j, t] = w[t] cos(2 pi f_j t / fps),  E[2j+1, t] = -w[t] sin(2 pi f_j t / fps),  A[r, t] = E[r, t] - mean_u E[r, u]
// with scipy.signal.blackmanharris(T) (symmetric) for w and f_j = fmin + j * step: sig - sig.mean() is folded into the operator.
// Built in long double, rounded once.  A [2F][T] row major, freqs [F].
static void spectral_operator(int T, double fps, double fmin, double fmax, int F, double *A, double *freqs)
{
    const long double two_pi = 6.283185307179586476925286766559L;
    const double step = (fmax - fmin) / (double)(F - 1);
    std::vector<long double> w(T), e(T);
    for (int t = 0; t < T; ++t) {
        // a0 - a1 cos x + a2 cos 2x - a3 cos 3x with 1 - cos k x = 2 sin^2(k x / 2): at the window's ends the four terms of the textbook form
        // cancel from 0.5 down to 6e-5 and leave the absolute error of the large ones behind (4 u relative to w there)
        const long double hx = two_pi * (long double)(2 * t < T ? t : T - 1 - t) / (long double)(T - 1) / 2.0L;   // (the window is symmetric)
        const long double s1 = sinl(hx), s2 = sinl(2.0L * hx), s3 = sinl(3.0L * hx);
        w[t] = 0.00006L + 2.0L * ((0.48829L * s1 * s1 - 0.14128L * s2 * s2) + 0.01168L * s3 * s3);
    }
    for (int j = 0; j < F; ++j) {
        const double f = fmin + (double)j * step;
        if (freqs) freqs[j] = f;
        if (!A) continue;
        for (int part = 0; part < 2; ++part) {
            // The mean decides the entries at the window's ends (w = 6e-5 there): whole turns leave the angle EXACTLY (f t has at most
            // 65 bits, fmodl is exact, so the angle errs by one rounding of a value below one turn), and the sum is compensated
            long double sum = 0.0L, comp = 0.0L;
            for (int t = 0; t < T; ++t) {
                const long double ang = two_pi * (fmodl((long double)f * (long double)t, (long double)fps) / (long double)fps);
                e[t] = part == 0 ? w[t] * cosl(ang) : -(w[t] * sinl(ang));
                const long double s2 = sum + e[t];   // (Neumaier)
                comp += fabsl(sum) >= fabsl(e[t]) ? (sum - s2) + e[t] : (e[t] - s2) + sum;
                sum = s2;
            }
            const long double mean = (sum + comp) / (long double)T;
            double *row = A + (size_t)(2 * j + part) * T;
            for (int t = 0; t < T; ++t) row[t] = (double)(e[t] - mean);
        }
    }
}

extern "C" int rm_spectral_operator(int T, double fps, double fmin, double fmax, int nfreq, double *A_host, double *freqs_host)
{
    if (T < 2 || nfreq < 3 || nfreq > 64 || !rate_band_ok(fps, fmin, fmax))
        return fail(RM_E_BADARG, "rm_spectral_operator: bad argument (T >= 2, 3 <= nfreq <= 64, 0 < freq_min < freq_max <= fps / 2)");
    if (T > MAX_T) return fail(RM_E_UNSUPPORTED, "rm_spectral_operator: T=%d > %d", T, MAX_T);
    spectral_operator(T, fps, fmin, fmax, nfreq, A_host, freqs_host);
    return RM_OK;
}

// the operator in the fragment-major form of rm_rate_kernels.h, cached per (T, fps, fmin, fmax, F) in the context's workspace
static int rate_operator(rm_ctx *ctx, int T, double fps, double fmin, double fmax, int F, const double **Af_out, hipStream_t s)
{
    const int NH = (F + 15) / 16, NT = 2 * NH, nks = (T + 3) / 4;
    const size_t n = (size_t)nks * NT * 64;
    double *dAf = nullptr;
    if (!(ctx->rate_T == T && ctx->rate_F == F && ctx->rate_fps == fps && ctx->rate_fmin == fmin && ctx->rate_fmax == fmax)) {
        ctx->rate_T = 0;
        std::vector<double> A((size_t)2 * F * T), Af(n, 0.0);
        spectral_operator(T, fps, fmin, fmax, F, A.data(), nullptr);
        for (int ks = 0; ks < nks; ++ks)
            for (int q = 0; q < NT; ++q)
                for (int l = 0; l < 64; ++l) {
                    const int j = 16 * (q < NH ? q : q - NH) + (l & 15), t = 4 * ks + (l >> 4);
                    if (j < F && t < T) Af[((size_t)ks * NT + q) * 64 + l] = A[(size_t)(2 * j + (q < NH ? 0 : 1)) * T + t];
                }
        RM_TRY(ws(ctx, "rate_Af", n, &dAf));
        HIP_TRY(hipMemcpyAsync(dAf, Af.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
        HIP_TRY(stream_wait(s));  // the source is a stack-lifetime vector
        ctx->rate_T = T; ctx->rate_F = F; ctx->rate_fps = fps; ctx->rate_fmin = fmin; ctx->rate_fmax = fmax;
    }
    RM_TRY(ws(ctx, "rate_Af", n, &dAf));
    *Af_out = dAf;
    return RM_OK;
}

template <int NH, int RING>
static int launch_rate_forms(bool wide, const double *x, int T, size_t NP, const double *Af, const RatePeak &o, int head, hipStream_t s)
{
    if (!wide && rate_split_lds(NH) > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)k_rate_peak<NH, RING>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rate_split_lds(NH)));
    if (wide) hipLaunchKernelGGL((k_rate_peak_px<NH, RING>), dim3((unsigned)((NP + 16 * RT_W - 1) / (16 * RT_W))), dim3(64 * RT_W), 0, s, x, T, NP, Af, o, head);
    else hipLaunchKernelGGL((k_rate_peak<NH, RING>), dim3((unsigned)((NP + 15) / 16)), dim3(64 * RT_W), rate_split_lds(NH), s, x, T, NP, Af, o, head);
    return RM_OK;
}

int rate_peak(rm_ctx *ctx, const double *x, int T, size_t NP, int head, double fps, double fmin, double fmax, int F, double *freq, double *power,
              double *total, int32_t *index, hipStream_t s, const char *who)
{
    if (!x || T < 2 || F < 3 || F > 64 || !rate_band_ok(fps, fmin, fmax) || (!freq && !power && !total && !index))
        return fail(RM_E_BADARG, "%s: bad argument (T >= 2, 3 <= nfreq <= 64, 0 < freq_min < freq_max <= fps / 2, at least one output)", who);
    if (T > MAX_T) return fail(RM_E_UNSUPPORTED, "%s: T=%d > %d", who, T, MAX_T);
    if (head < 0 || head >= T) return fail(RM_E_BADARG, "%s: ring head %d outside [0, %d)", who, head, T);
    if (NP == 0) return RM_OK;
    if ((NP + 15) / 16 > 0x7fffffffull) return fail(RM_E_UNSUPPORTED, "%s: %zu pixel columns", who, NP);
    const double *Af = nullptr;
    RM_TRY(rate_operator(ctx, T, fps, fmin, fmax, F, &Af, s));
    RatePeak o;
    o.freq = freq; o.power = power; o.total = total; o.index = index;
    o.fmin = fmin; o.step = (fmax - fmin) / (double)(F - 1); o.F = F;
    // large levels: one wave per 16 pixel columns, no K-split (k_rate_peak_px); the choice depends on NP only
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    const bool wide = ctx->dbg.rate_wide >= 0 ? ctx->dbg.rate_wide != 0 : NP >= (size_t)64 * 4 * cus;
    const int NH = (F + 15) / 16;
#define RM_RATE_CASE(NN)                                                                    \
    case NN:                                                                                \
        if (head > 0) RM_TRY((launch_rate_forms<NN, 1>(wide, x, T, NP, Af, o, head, s)));   \
        else RM_TRY((launch_rate_forms<NN, 0>(wide, x, T, NP, Af, o, 0, s)));               \
        break;
    switch (NH) {
        RM_RATE_CASE(1)
        RM_RATE_CASE(2)
        RM_RATE_CASE(3)
        default: RM_RATE_CASE(4)
    }
#undef RM_RATE_CASE
    LAUNCH_CHECK();
    return RM_OK;
}

extern "C" int rm_spectral_peak(rm_ctx *ctx, const double *x_dev, int T, size_t NP, double fps, double fmin, double fmax, int nfreq, double *freq_dev,
                                double *power_dev, double *total_dev, int32_t *index_dev, void *stream)
{
    if (!ctx) return fail(RM_E_BADARG, "rm_spectral_peak: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    return rate_peak(ctx, x_dev, T, NP, 0, fps, fmin, fmax, nfreq, freq_dev, power_dev, total_dev, index_dev, (hipStream_t)stream, "rm_spectral_peak");
}

extern "C" int rm_rate_map(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W, int level, double fps, double fmin, double fmax, int nfreq,
                           double *freq_dev, double *power_dev, double *total_dev, int32_t *index_dev, void *stream)
{
    if (!ctx || !frames_dev || !valid_buffer_dtype(dtype) || T < 2 || H < 1 || W < 1 || level < 1 || nfreq < 3 || nfreq > 64 ||
        !rate_band_ok(fps, fmin, fmax) || (!freq_dev && !power_dev && !total_dev && !index_dev))
        return fail(RM_E_BADARG, "rm_rate_map: bad argument (T >= 2, level >= 1, 3 <= nfreq <= 64, 0 < freq_min < freq_max <= fps / 2, at least one output)");
    if (T > MAX_T) return fail(RM_E_UNSUPPORTED, "rm_rate_map: T=%d > %d", T, MAX_T);
    if (level >= MAX_CHAIN) return fail(RM_E_UNSUPPORTED, "rm_rate_map: level %d >= %d", level, MAX_CHAIN);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ctx->device));
    RM_TRY(ctx_stream_ok(ctx, stream, __func__));
    // G_level of every frame by the route front_pyramid takes for G_S: the frame-buffer kernel, one pass over the frames
    std::vector<int> h, w;
    level_sizes(H, W, level + 1, h, w);
    const size_t NP = (size_t)h[level] * w[level];
    double *g = nullptr;
    RM_TRY(ws(ctx, "rate_g", (size_t)T * NP, &g));
    RM_TRY(launch_frames_down(ctx, frames_dev, dtype, T, h, w, level, g, s, false));
    return rate_peak(ctx, g, T, NP, 0, fps, fmin, fmax, nfreq, freq_dev, power_dev, total_dev, index_dev, s, "rm_rate_map");
}
