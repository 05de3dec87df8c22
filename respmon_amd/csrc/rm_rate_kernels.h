// respmon_amd/csrc/rm_rate_kernels.h -- the rate map: per pixel column the dominant frequency of a band and its share of the band's
// power (include/respmon_hip.h rm_spectral_peak): the kernels of rm_rate.hip.
#pragma once
#include "rm_temporal_kernels.h"   // ring_row, v4f64

namespace rm {

// A windowed DTFT on a fine grid of F <= 64 frequencies is a dense contraction along T, P = |A y|^2 with A [2F x T] (rm_rate.hip
// spectral_operator: Blackman-Harris window, mean removal folded in) and y[t, p] = x[t, p] - x[0, p], followed by a per-column argmax
// and a three-point refinement on log P.  The contraction runs on v_mfma_f64_16x16x4_f64 as the temporal band-pass does
// (rm_temporal_kernels.h): a wave holds 16 pixel columns and NT = 2 NH accumulator tiles of 16 operator rows, NH = ceil(F / 16);
// tile q holds the COSINE rows of frequencies 16 q .. 16 q + 15 and tile q + NH the SINE rows of the same sixteen, so that in the D
// layout (row = (lane >> 4) + 4 reg, column = lane & 15) the two halves of P_j sit in the same lane and register:
//   P[16 q + (lane >> 4) + 4 r][lane & 15] = acc[q][r]^2 + acc[q + NH][r]^2.
// The operator arrives fragment major (built on the host), every A operand one coalesced 512-byte load:
//   Af[(ks * NT + q) * 64 + lane] = row(q, lane & 15)[4 ks + (lane >> 4)],  zero for rows past F and frames past T.
// y is formed in registers (x[0, p] is loaded once per lane); K-steps past T multiply zeros.
// Epilogue (rate_epilogue): the wave writes its P[F][16] to LDS (at most 8 KB) and sixteen lanes scan one column each in ascending j:
// the sequential total, the FIRST maximum and its two neighbours need no cross-lane tie rule.
// Two forms, for the reasons the band-pass has two: k_rate_peak splits K over the four waves of a workgroup (small levels
// are latency bound; the partial tiles meet in LDS and are added in wave order), k_rate_peak_px gives a wave its 16 columns for the
// whole contraction and fetches the operator chunks once per workgroup through LDS (large levels).  Which one a call takes depends on
// (T, NP, F) only; the two agree to rounding, not bit for bit (the K order differs).
struct RatePeak {
    double *freq, *power, *total;   // [NP] each, any may be null
    int *index;
    double fmin, step;              // f_j = fmin + j * step
    int F;
};

constexpr int RT_W = 4;   // waves per workgroup, both forms
constexpr size_t rate_split_lds(int NH) { return sizeof(double) * (size_t)(RT_W * 8 * NH * 64 + NH * 256); }   // dynamic LDS of k_rate_peak<NH>
__device__ __forceinline__ void rate_scan(const double *sp, int lane, size_t p0, size_t NP, const struct RatePeak &o);

// acc: the wave's finished tiles; sp: NH * 256 doubles of LDS that belong to this wave; p0: the wave's first pixel column
template <int NH>
__device__ __forceinline__ void rate_epilogue(const v4f64 (&acc)[2 * NH], double *sp, int lane, size_t p0, size_t NP, const RatePeak &o)
{
    const int lo = lane & 15, hi = lane >> 4;
#pragma unroll
    for (int q = 0; q < NH; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 16 * q + hi + 4 * r;
            const double c = acc[q][r], s = acc[q + NH][r];
            if (j < o.F) sp[j * 16 + lo] = c * c + s * s;
        }
    wave_sync();
    rate_scan(sp, lane, p0, NP, o);
}

// sixteen lanes scan one column of the finished P[F][16] each
__device__ __forceinline__ void rate_scan(const double *sp, int lane, size_t p0, size_t NP, const RatePeak &o)
{
    if (lane >= 16 || p0 + lane >= NP) return;
    const size_t p = p0 + lane;
    const int F = o.F;
    double total = 0.0, best = sp[lane];
    int idx = 0;
    for (int j = 0; j < F; ++j) {
        const double v = sp[j * 16 + lane];
        total = total + v;
        if (v > best) { best = v; idx = j; }
    }
    double freq;
    if (total == 0.0) {
        idx = -1; best = 0.0;
        freq = __longlong_as_double(0x7ff8000000000000ll);
    } else {
        double delta = 0.0;
        if (idx > 0 && idx < F - 1) {
            const double pa = sp[(idx - 1) * 16 + lane], pc = sp[(idx + 1) * 16 + lane];
            if (pa > 0.0 && best > 0.0 && pc > 0.0) {
                const double a = log(pa), b = log(best), c = log(pc);
                const double num = a - c, den = (a - 2.0 * b) + c;
                if (den < 0.0) {
                    delta = (0.5 * num) / den;
                    delta = delta < -0.5 ? -0.5 : delta > 0.5 ? 0.5 : delta;
                }
            }
        }
        freq = (o.fmin + (double)idx * o.step) + delta * o.step;
    }
    if (o.freq) o.freq[p] = freq;
    if (o.power) o.power[p] = best;
    if (o.total) o.total[p] = total;
    if (o.index) o.index[p] = idx;
}

// K-split form: a workgroup owns 16 pixel columns, wave w contracts K-steps w, w + 4, ... in increasing order (the x operands of a
// chunk are all requested up front, the operator fragments in batches, as in k_temporal_sym); the partial tiles meet in LDS, where wave
// w adds those of frequencies 16 w .. 16 w + 15 in wave order; wave 0 scans.
template <int NH, int RING = 0>
__global__ __launch_bounds__(64 * RT_W, 2) void k_rate_peak(const double *__restrict__ x, int T, size_t NP, const double *__restrict__ Af, RatePeak o,
                                                            int head)
{
    constexpr int NT = 2 * NH;
    constexpr int RT_U = NH == 1 ? 8 : NH == 2 ? 4 : 2;   // K-steps whose operator fragments travel together
    constexpr int RT_XPF = NH <= 2 ? 16 : 8;              // K-steps of a wave whose x operands travel together
    HIP_DYNAMIC_SHARED(double, s_part)            // [RT_W][4 NT][64] partial tiles, then P [NH * 16][16]: rate_split_lds(NH) bytes
    double *s_p = s_part + RT_W * 4 * NT * 64;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lo = lane & 15, hi = lane >> 4;
    const size_t p0 = (size_t)blockIdx.x * 16, p = p0 + lo;
    const size_t pc = p < NP ? p : NP - 1;     // columns past the end repeat the last one (never stored)
    const int nks = (T + 3) >> 2;
    const double x0 = x[(size_t)ring_row<RING>(0, head, T) * NP + pc];
    v4f64 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int kc = wave; kc < nks; kc += RT_W * RT_XPF) {
        double xa[RT_XPF];
#pragma unroll
        for (int i = 0; i < RT_XPF; ++i) {
            const int ks = kc + i * RT_W;
            if (ks < nks) {   // (wave-uniform)
                const int t = 4 * ks + hi, tc = t < T ? t : T - 1;
                xa[i] = x[(size_t)ring_row<RING>(tc, head, T) * NP + pc];
            }
        }
#pragma unroll
        for (int i0 = 0; i0 < RT_XPF; i0 += RT_U) {
            if (kc + i0 * RT_W >= nks) break;   // (wave-uniform)
            double rr[RT_U][NT];
#pragma unroll
            for (int u = 0; u < RT_U; ++u) {
                const int ks = kc + (i0 + u) * RT_W;
                if (ks < nks) {
                    const double *af = Af + (size_t)ks * NT * 64 + lane;
#pragma unroll
                    for (int q = 0; q < NT; ++q) rr[u][q] = af[q * 64];
                }
            }
#pragma unroll
            for (int u = 0; u < RT_U; ++u) {
                const int ks = kc + (i0 + u) * RT_W;
                if (ks < nks) {
                    const double y = 4 * ks + hi < T ? xa[i0 + u] - x0 : 0.0;
#pragma unroll
                    for (int q = 0; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rr[u][q], y, acc[q], 0, 0, 0);
                }
            }
        }
    }
    // every wave leaves its partial tiles in LDS; wave w < NH then owns the frequencies 16 w .. 16 w + 15: it adds the four partial sums of
    // their cosine and sine tiles in wave order and writes their powers; wave 0 scans the finished P[F][16]
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_part[(wave * 4 * NT + 4 * q + r) * 64 + lane] = acc[q][r];
    __syncthreads();
    if (wave < NH) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double c = s_part[(4 * wave + r) * 64 + lane], s = s_part[(4 * (wave + NH) + r) * 64 + lane];
#pragma unroll
            for (int w = 1; w < RT_W; ++w) {
                c = c + s_part[(w * 4 * NT + 4 * wave + r) * 64 + lane];
                s = s + s_part[(w * 4 * NT + 4 * (wave + NH) + r) * 64 + lane];
            }
            const int j = 16 * wave + hi + 4 * r;
            if (j < o.F) s_p[j * 16 + lo] = c * c + s * s;
        }
    }
    __syncthreads();
    if (wave == 0) rate_scan(s_p, lane, p0, NP, o);
}

// Wide form: a WAVE owns 16 pixel columns for the whole contraction, K runs straight through; x streams through two register buffers
// of RP_XC K-steps, the operator chunks through two LDS buffers the workgroup's 256 threads fill with 16-byte loads while the previous
// chunk is multiplied (one barrier per chunk, conflict-free ds_read_b64 of the A operands) -- the scheme of k_temporal_sym_px.  The
// barrier behind the last chunk frees both buffers: the four waves' P arrays take their place.
template <int NH, int RING = 0>
__global__ __launch_bounds__(64 * RT_W, 2) void k_rate_peak_px(const double *__restrict__ x, int T, size_t NP, const double *__restrict__ Af, RatePeak o,
                                                               int head)
{
    constexpr int NT = 2 * NH;
    constexpr int RP_XC = NH <= 2 ? 8 : 4;         // K-steps per chunk
    constexpr int RCH = RP_XC * NT * 64;           // doubles of one fragment chunk (8 / 16 / 12 / 16 KB)
    constexpr int RL = RCH / 512;                  // 16-byte loads per thread and chunk
    static_assert(RCH % 512 == 0 && 2 * RCH >= RT_W * NH * 256, "chunk buffers: whole loads, and room for the four P arrays");
    __shared__ double s_frag[2][RCH];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6)), lo = lane & 15, hi = lane >> 4;
    const size_t p0 = ((size_t)blockIdx.x * RT_W + wave) * 16, p = p0 + lo;   // (waves past NP multiply a clamped column and store nothing: they keep the barriers)
    const size_t pc = p < NP ? p : NP - 1;
    const int nks = (T + 3) >> 2;
    const int nchunks = (nks + RP_XC - 1) / RP_XC;
    const double x0 = x[(size_t)ring_row<RING>(0, head, T) * NP + pc];
    v4f64 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (v4f64){0.0, 0.0, 0.0, 0.0};
    double xa[2][RP_XC];
    auto load_x = [&](int buf, int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < RP_XC; ++i) {
            const int ks = k0 + i;
            const int t = 4 * (ks < nks ? ks : nks - 1) + hi, tc = t < T ? t : T - 1;
            xa[buf][i] = x[(size_t)ring_row<RING>(tc, head, T) * NP + pc];
        }
    };
    // this thread's share of a fragment chunk: global -> registers (in flight while the previous chunk is multiplied) -> LDS
    typedef RM_VEC(double, 2) v2f64;
    const size_t a_last = (size_t)nks * NT * 64 - 2;              // (chunks are whole RP_XC K-steps: the last one reads clamped, unused values)
    v2f64 gl[RL];
    auto fetch_a = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < RL; ++j) {
            size_t i = (size_t)c * RCH + 2 * tid + 512 * j;
            i = i < a_last ? i : a_last;
            gl[j] = *reinterpret_cast<const v2f64 *>(Af + i);
        }
    };
    auto stash_a = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < RL; ++j) *reinterpret_cast<v2f64 *>(&s_frag[buf][2 * tid + 512 * j]) = gl[j];
    };
    auto products = [&](int xbuf, int c) __attribute__((always_inline)) {
        const double *sr = &s_frag[c & 1][lane];
#pragma unroll
        for (int u = 0; u < RP_XC; ++u) {
            const int ks = c * RP_XC + u;
            if (ks < nks) {   // (uniform)
                double rr[NT];
#pragma unroll
                for (int q = 0; q < NT; ++q) rr[q] = sr[(u * NT + q) * 64];
                const double y = 4 * ks + hi < T ? xa[xbuf][u] - x0 : 0.0;
#pragma unroll
                for (int q = 0; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rr[q], y, acc[q], 0, 0, 0);
            }
        }
    };
    fetch_a(0);
    load_x(0, 0);
    stash_a(0);
    __syncthreads();
    for (int c0 = 0; c0 < nchunks; c0 += 2) {      // two chunks per trip: the x register buffers are static
        if (c0 + 1 < nchunks) fetch_a(c0 + 1);
        load_x(1, (c0 + 1) * RP_XC);
        products(0, c0);
        if (c0 + 1 < nchunks) stash_a(1);          // (every wave left buffer 1 before the barrier that ended the previous chunk)
        __syncthreads();
        if (c0 + 1 >= nchunks) break;              // (uniform)
        if (c0 + 2 < nchunks) fetch_a(c0 + 2);
        load_x(0, (c0 + 2) * RP_XC);
        products(1, c0 + 1);
        if (c0 + 2 < nchunks) stash_a(0);
        __syncthreads();
    }
    rate_epilogue<NH>(acc, &s_frag[0][0] + wave * (NH * 256), lane, p0, NP, o);
}

}  // namespace rm
