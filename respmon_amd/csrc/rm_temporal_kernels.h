// respmon_amd/csrc/rm_temporal_kernels.h -- the temporal filters along T (transforms.py:72-102): the FFT band-pass as a linear operator
// in its two-stage and MFMA forms, scipy's lfilter: the kernels of rm_temporal.hip.
#pragma once
#include "rm_kernels.h"

namespace rm {

// ----------------------------------------------------------------------------------------
// K5-K8  temporal band-pass (transforms.py:82-102): packed rfft -> index mask -> Re(ifft) -> *amp,
//        a fixed real linear operator along T, applied in its two-stage form.
// ----------------------------------------------------------------------------------------
// Two-stage form (the reference's own rfft -> mask -> ifft order; ~T/(2*nk) times cheaper than the dense
// T x T product M = C R that rm_temporal_operator() exports for inspection):
//   stage 1 (packed real FFT rows that survive the mask):  y[k,p]   = sum_t R[k,t] x[t,p]          k < nk
//   stage 2 (Re(ifft) of the packed array, then *amp):     out[s,p] = amp * sum_k C[s,k] y[k,p]    s < T
// One single-wave workgroup = 64 pixels x KC (resp. SC) outputs; coefficient chunks are staged in LDS and
// read as broadcasts; the pixel loads are issued U deep.  All levels of the small pyramid sit side by side
// in one [T, NP] buffer, so one launch per stage serves every filtered level.
constexpr int TF_KC = 4, TF_SC = 8, TF_U = 16;

// Measured and rejected (1080p x 256, both stages 0.064 ms as written): splitting T over 4 waves per workgroup with an
// LDS reduction (stage 1 48 us vs 42 us); splitting T over 2 / 4 workgroups with partial y buffers (+11 / +56 us);
// 8 / 12 / 16 rows of R per workgroup instead of 4, i.e. fewer re-reads of x through L2 but fewer waves (+10 / +25 /
// +34 us); 16 output rows per workgroup in stage 2 (no change);
// one fused kernel per 64 pixel columns that reads x once, keeps all y[k] in registers and takes the
// coefficients through the scalar cache (128 us vs 64 us for both stages: one workgroup per CU exposes every
// scalar-load and global-load latency, the two-stage form has 8-20 waves per CU to hide them).


// The input of the temporal kernels may be a RING of T rows (rm_window.hip): frame t of the chronological window is row t + head,
// minus T when that reaches T (0 <= head < T).  RING is a compile-time variant: with RING == 0 `head` is never read and the kernels are
// the ones every call on a contiguous [T, NP] buffer has always run.  The row index is integer arithmetic on values known before any
// load is issued, so the up-front batches of x loads stay independent of each other; the outputs are in chronological order.
template <int RING> __device__ __forceinline__ int ring_row(int t, int head, int T)
{
    if (RING) { const int r = t + head; return r >= T ? r - T : r; }
    return t;
}

// st_init (nullable): workgroup (0, 0) also resets the reduction state of the collapse passes that follow on the stream
template <int RING = 0>
__global__ __launch_bounds__(64) void k_temporal_fwd(const double *x, int T, size_t NP, const double *R, int nk, double *y, struct CollapseState *st_init,
                                                     int head)
{
    HIP_DYNAMIC_SHARED(double, s_r)  // [T][TF_KC]
    if (st_init && blockIdx.x == 0 && blockIdx.y == 0) state_init_lane(st_init, (int)threadIdx.x);
    const int k0 = blockIdx.y * TF_KC;
    for (int i = threadIdx.x; i < T * TF_KC; i += 64) {
        int t = i / TF_KC, k = i - t * TF_KC;
        s_r[i] = (k0 + k < nk) ? R[(size_t)(k0 + k) * T + t] : 0.0;
    }
    __syncthreads();
    size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= NP) return;
    double acc[TF_KC];
#pragma unroll
    for (int k = 0; k < TF_KC; ++k) acc[k] = 0.0;
    for (int t0 = 0; t0 < T; t0 += TF_U) {
        double v[TF_U];
#pragma unroll
        for (int u = 0; u < TF_U; ++u) v[u] = (t0 + u < T) ? x[(size_t)ring_row<RING>(t0 + u, head, T) * NP + p] : 0.0;
#pragma unroll
        for (int u = 0; u < TF_U; ++u) {
            if (t0 + u < T) {
                const double *r = &s_r[(t0 + u) * TF_KC];
#pragma unroll
                for (int k = 0; k < TF_KC; ++k) acc[k] = acc[k] + r[k] * v[u];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < TF_KC; ++k)
        if (k0 + k < nk) y[(size_t)(k0 + k) * NP + p] = acc[k];
}

// T = rows of C / frames written (the unique frames: sym_frames(n)); mirror_n > 0: also store row s as row mirror_n - s
// (0 < s, 2 s < mirror_n) -- the full [n, NP] array of the module-level filter call
RM_KERNEL __launch_bounds__(64) void k_temporal_inv(const double *y, int nk, size_t NP, const double *C, int T, double amp,
                                                     double *out, int mirror_n)
{
    HIP_DYNAMIC_SHARED(double, s_c)  // [nk][TF_SC]
    const int s0 = blockIdx.y * TF_SC;
    for (int i = threadIdx.x; i < nk * TF_SC; i += 64) {
        int k = i / TF_SC, j = i - k * TF_SC;
        s_c[i] = (s0 + j < T) ? C[(size_t)(s0 + j) * nk + k] : 0.0;
    }
    __syncthreads();
    size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= NP) return;
    double acc[TF_SC];
#pragma unroll
    for (int j = 0; j < TF_SC; ++j) acc[j] = 0.0;
    for (int k0 = 0; k0 < nk; k0 += TF_U) {
        double v[TF_U];
#pragma unroll
        for (int u = 0; u < TF_U; ++u) v[u] = (k0 + u < nk) ? y[(size_t)(k0 + u) * NP + p] : 0.0;
#pragma unroll
        for (int u = 0; u < TF_U; ++u) {
            if (k0 + u < nk) {
                const double *c = &s_c[(k0 + u) * TF_SC];
#pragma unroll
                for (int j = 0; j < TF_SC; ++j) acc[j] = acc[j] + c[j] * v[u];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TF_SC; ++j)
        if (s0 + j < T) {
            const int sr = s0 + j;
            const double v = acc[j] * amp;
            out[(size_t)sr * NP + p] = v;
            if (mirror_n > 0 && sr > 0 && 2 * sr < mirror_n) out[(size_t)(mirror_n - sr) * NP + p] = v;
        }
}

// Matrix-core form of the two stages (even n, at most 48 merged rows of either symmetry class).
// The band-pass IS a dense contraction along T -- z = Rz x, out = amp * Cz z -- and the only place on this path where MFMA fits.
// v_mfma_f64_16x16x4_f64 runs at the fp64 vector rate on gfx950, so what counts is the number of products and operand reuse:
//   * merged rows (host, get_operator): packed indices k and n - k multiply the same inverse column cos(2 pi k s / n), so their
//     forward rows are added once on the host: about half the rows of R and the columns of C;
//   * folded frames: a merged row is a cosine row (even in t) or a sine row (odd in t), never a mix (n even), so
//         z_even = sum_{t <= n/2} Rz[., t] e[t],   e[t] = x[t] + x[n - t]   (x[t] alone for t = 0 and t = n / 2)
//         z_odd  = sum_{t <  n/2} Rz[., t] o[t],   o[t] = x[t] - x[n - t]   (0 there)
//     -- half the K-steps; the tiles of 16 rows are class-pure (NH "even" tiles, then NH "odd" tiles, zero padded);
//   * unique output frames: only s <= n / 2 is produced (sym_frames): half the products of stage 2.
// 6 x fewer products than the plain two-stage form at n = 256 / 512.  A workgroup owns 16 pixel columns and reads its x[T, 16] tile
// ONCE, keeps z in 2 NH accumulator tiles and feeds them straight back as the B operands of the second product -- the D layout of
// the first product (row = (lane >> 4) + 4 * reg, col = lane & 15) is exactly the B layout the second one needs for K-step
// (tile, reg) -- so z never leaves registers.  The W wavefronts of a workgroup share the 16 columns: wave w contracts every W-th
// K-step of stage 1 (the partial z tiles meet in LDS, summed in wave order) and produces every W-th tile of 16 output frames.
// The operators arrive "fragment major" (built on the host), so that every A operand is one coalesced 512-byte load:
//   Rf[(ks * 2 NH + q) * 64 + lane] = Rz[row(q, lane & 15)][4 ks + (lane >> 4)]
//   Cf[(m * 8 NH + 4 q + r) * 64 + lane] = Cz[16 m + (lane & 15)][row(q, 4 r + (lane >> 4))]
// fused == materialised == per-level stays bit for bit: every path through the library uses this same kernel for a given n.
constexpr int TM_W = 4;            // waves per workgroup
constexpr int TM_MAX_HALF = 3;     // up to 48 merged rows per symmetry class (n = 1024 at 10 fps has 47 + 47)

typedef RM_VEC(double, 4) v4f64;

// mirror_n > 0: also store output frame s as frame mirror_n - s (the full [n, NP] array of the module-level filter call)
template <int NH, int RING = 0>
__global__ __launch_bounds__(64 * TM_W, NH == 1 ? 3 : 2) void k_temporal_sym(const double *__restrict__ x, int T, size_t NP, const double *__restrict__ Rf,
                                                             const double *__restrict__ Cf, double amp, double *__restrict__ out, int mirror_n,
                                                             struct CollapseState *st_init, int head)
{
    RM_TRACE_SCOPE(2);
    if (st_init && blockIdx.x == 0 && threadIdx.x < 64) state_init_lane(st_init, (int)threadIdx.x);
    constexpr int NT = 2 * NH;
    __shared__ double s_y[TM_W][4 * NT][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lo = lane & 15, hi = lane >> 4;
    const size_t p = (size_t)blockIdx.x * 16 + lo;
    const size_t pc = p < NP ? p : NP - 1;     // columns past the end repeat the last one (never stored)
    const int Th = sym_frames(T), nks = (Th + 3) >> 2;
    v4f64 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (v4f64){0.0, 0.0, 0.0, 0.0};
    RM_TRACE_MARK(2, 0);
    // x comes from HBM (one round trip ~2 us under load), the operator fragments from L2: a chunk of up to TM_XPF K-steps has ALL
    // its x operands requested up front (two doubles per K-step and lane), then the K-steps run in batches of TM_U whose operator
    // fragments are requested together.  A loop that loads one step's operands, waits and multiplies is a chain of round trips, and
    // at 2-3 waves per SIMD nothing hides them (4K x 512: 2.75 -> 1.16 ms with the symmetric operator, -> this).
    // The order of the products into each accumulator is fixed: K-steps wave, wave + W, ... in increasing order.
    constexpr int TM_U = NH == 1 ? 8 : 4;
    constexpr int TM_XPF = NH == 3 ? 8 : 16;
    for (int kc = wave; kc < nks; kc += TM_W * TM_XPF) {
        double xa[TM_XPF], xb[TM_XPF];
#pragma unroll
        for (int i = 0; i < TM_XPF; ++i) {
            const int ks = kc + i * TM_W;
            if (ks < nks) {   // (wave-uniform)
                const int t = 4 * ks + hi, tc = t < Th ? t : Th - 1, tp = tc == 0 ? 0 : T - tc;
                xa[i] = x[(size_t)ring_row<RING>(tc, head, T) * NP + pc];
                xb[i] = x[(size_t)ring_row<RING>(tp, head, T) * NP + pc];
            }
        }
#pragma unroll
        for (int i0 = 0; i0 < TM_XPF; i0 += TM_U) {
            if (kc + i0 * TM_W >= nks) break;   // (wave-uniform)
            double rr[TM_U][NT];
#pragma unroll
            for (int u = 0; u < TM_U; ++u) {
                const int ks = kc + (i0 + u) * TM_W;
                if (ks < nks) {
                    const double *rf = Rf + (size_t)ks * NT * 64 + lane;
#pragma unroll
                    for (int q = 0; q < NT; ++q) rr[u][q] = rf[q * 64];
                }
            }
#pragma unroll
            for (int u = 0; u < TM_U; ++u) {
                const int ks = kc + (i0 + u) * TM_W;
                if (ks < nks) {
                    const int t = 4 * ks + hi;
                    const bool self = t == 0 || 2 * t == T, valid = t < Th;
                    double e = self ? xa[i0 + u] : xa[i0 + u] + xb[i0 + u], o = self ? 0.0 : xa[i0 + u] - xb[i0 + u];
                    if (!valid) { e = 0.0; o = 0.0; }
#pragma unroll
                    for (int q = 0; q < NH; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rr[u][q], e, acc[q], 0, 0, 0);
#pragma unroll
                    for (int q = NH; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rr[u][q], o, acc[q], 0, 0, 0);
                }
            }
        }
        RM_TRACE_MARK(2, 8 + (kc - wave) / (TM_W * TM_XPF));
    }
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_y[wave][4 * q + r][lane] = acc[q][r];
    RM_TRACE_MARK(2, 1);
    const int mt = (Th + 15) >> 4;             // output tiles of 16 frames, dealt round-robin to the waves
    // the A operands of this wave's first output tile travel while the partial z tiles meet in LDS
    double cfv[4 * NT];
    if (wave < mt) {
        const double *cf = Cf + (size_t)wave * 4 * NT * 64 + lane;
#pragma unroll
        for (int q = 0; q < 4 * NT; ++q) cfv[q] = cf[q * 64];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = s_y[0][4 * q + r][lane];
#pragma unroll
            for (int w = 1; w < TM_W; ++w) v = v + s_y[w][4 * q + r][lane];
            acc[q][r] = v;
        }
    RM_TRACE_MARK(2, 2);
    for (int m = wave; m < mt; m += TM_W) {
        const int s0 = 16 * m;
        v4f64 o = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < NT; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) o = __builtin_amdgcn_mfma_f64_16x16x4f64(cfv[4 * q + r], acc[q][r], o, 0, 0, 0);
        }
        if (m + TM_W < mt) {   // the next tile's operands travel while this one is stored
            const double *cf = Cf + (size_t)(m + TM_W) * 4 * NT * 64 + lane;
#pragma unroll
            for (int q = 0; q < 4 * NT; ++q) cfv[q] = cf[q * 64];
        }
        if (p < NP) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int sr = s0 + hi + 4 * r;
                if (sr < Th) {
                    const double v = o[r] * amp;
                    out[(size_t)sr * NP + p] = v;
                    if (mirror_n > 0 && sr > 0 && 2 * sr < mirror_n) out[(size_t)(mirror_n - sr) * NP + p] = v;
                }
            }
        }
    }
    RM_TRACE_MARK(2, 3);
}

// The same products for LARGE levels (4K x 512, skip 2: 518 400 pixels per frame, 2.1 GB in, 1.07 GB out): throughput, not
// latency, is what counts there, and k_temporal_sym's K-split costs it an LDS exchange plus a barrier per 16 pixels and a
// frontier of only 128 contiguous bytes per frame and workgroup in DRAM.  Here a WAVE owns 16 pixel columns for the whole
// contraction (the four waves of a workgroup sit on adjacent columns: 512 contiguous bytes per frame) and x streams through two
// register buffers of TP_XC K-steps (the next chunk is requested before the current one is multiplied).
// Round 5: the operator fragments travel through LDS, fetched ONCE per workgroup.  Every wave needs all of Rf and Cf (272 KB at T = 512)
// for its 16 pixels; with each wave loading them itself the CU's vector memory path moved 3 KB per K-step and wave against 256 MFMA
// cycles per SIMD -- PMC at 4K x 512: TA busy 69 %, MFMA pipe 39 %, waves 70 % in issue stalls, 14 % in s_waitcnt.  Now the workgroup's 256
// threads copy a chunk of TP_XC K-steps (stage 2: one output tile) into one of two LDS buffers with 16-byte loads while the previous
// chunk is multiplied, one barrier per chunk, and the waves read their A operands with conflict-free ds_read_b64.
// The products into each accumulator happen in the same order as in k_temporal_sym?  No: there the partial sums of the four K-phases
// are added in wave order -- here K runs straight through.  The two kernels agree to rounding (~1e-16), and a given (T, level size)
// always takes the same one.
template <int NH, int RING = 0>
__global__ __launch_bounds__(256, 2) void k_temporal_sym_px(const double *__restrict__ x, int T, size_t NP, const double *__restrict__ Rf,
                                                            const double *__restrict__ Cf, double amp, double *__restrict__ out, int mirror_n,
                                                            struct CollapseState *st_init, int head)
{
    if (st_init && blockIdx.x == 0 && threadIdx.x < 64) state_init_lane(st_init, (int)threadIdx.x);
    constexpr int NT = 2 * NH;
    constexpr int TP_XC = 8;                       // K-steps per chunk (x registers and operator fragments alike)
    constexpr int RCH = TP_XC * NT * 64;           // doubles of one stage-1 fragment chunk (NH = 2: 16 KB)
    constexpr int CCH = 4 * NT * 64;               // doubles of one output tile's stage-2 fragments (NH = 2: 8 KB)
    constexpr int RL = RCH / 512, CL = CCH / 512;  // 16-byte loads per thread and chunk
    __shared__ double s_frag[2][RCH];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6)), lo = lane & 15, hi = lane >> 4;
    const size_t p = ((size_t)blockIdx.x * 4 + wave) * 16 + lo;   // (waves past NP multiply a clamped column and store nothing: they keep the barriers)
    const size_t pc = p < NP ? p : NP - 1;
    const int Th = sym_frames(T), nks = (Th + 3) >> 2;
    const int nchunks = (nks + TP_XC - 1) / TP_XC;
    v4f64 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = (v4f64){0.0, 0.0, 0.0, 0.0};
    double xa[2][TP_XC], xb[2][TP_XC];
    auto load_x = [&](int buf, int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TP_XC; ++i) {
            const int ks = k0 + i;
            const int t = 4 * (ks < nks ? ks : nks - 1) + hi, tc = t < Th ? t : Th - 1, tp = tc == 0 ? 0 : T - tc;
            xa[buf][i] = x[(size_t)ring_row<RING>(tc, head, T) * NP + pc];
            xb[buf][i] = x[(size_t)ring_row<RING>(tp, head, T) * NP + pc];
        }
    };
    // this thread's share of a fragment chunk: global -> registers (in flight while the previous chunk is multiplied) -> LDS
    typedef RM_VEC(double, 2) v2f64;
    const size_t r_last = (size_t)nks * NT * 64 - 2;              // (chunks are whole TP_XC K-steps: the last one reads clamped, unused values)
    v2f64 gl[RL];
    auto fetch_r = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < RL; ++j) {
            size_t i = (size_t)c * RCH + 2 * tid + 512 * j;
            i = i < r_last ? i : r_last;
            gl[j] = *reinterpret_cast<const v2f64 *>(Rf + i);
        }
    };
    auto stash_r = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < RL; ++j) *reinterpret_cast<v2f64 *>(&s_frag[buf][2 * tid + 512 * j]) = gl[j];
    };
    auto products = [&](int xbuf, int c) __attribute__((always_inline)) {
        const double *sr = &s_frag[c & 1][lane];
#pragma unroll
        for (int u = 0; u < TP_XC; ++u) {
            const int ks = c * TP_XC + u;
            if (ks < nks) {   // (uniform)
                double rr[NT];
#pragma unroll
                for (int q = 0; q < NT; ++q) rr[q] = sr[(u * NT + q) * 64];
                const int t = 4 * ks + hi;
                const bool self = t == 0 || 2 * t == T, valid = t < Th;
                double e = self ? xa[xbuf][u] : xa[xbuf][u] + xb[xbuf][u], o = self ? 0.0 : xa[xbuf][u] - xb[xbuf][u];
                if (!valid) { e = 0.0; o = 0.0; }
#pragma unroll
                for (int q = 0; q < NH; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rr[q], e, acc[q], 0, 0, 0);
#pragma unroll
                for (int q = NH; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rr[q], o, acc[q], 0, 0, 0);
            }
        }
    };
    fetch_r(0);
    load_x(0, 0);
    stash_r(0);
    __syncthreads();
    for (int c0 = 0; c0 < nchunks; c0 += 2) {      // two chunks per trip: the x register buffers are static
        if (c0 + 1 < nchunks) fetch_r(c0 + 1);
        load_x(1, (c0 + 1) * TP_XC);
        products(0, c0);
        if (c0 + 1 < nchunks) stash_r(1);          // (every wave left buffer 1 before the barrier that ended the previous chunk)
        __syncthreads();
        if (c0 + 1 >= nchunks) break;              // (uniform)
        if (c0 + 2 < nchunks) fetch_r(c0 + 2);
        load_x(0, (c0 + 2) * TP_XC);
        products(1, c0 + 1);
        if (c0 + 2 < nchunks) stash_r(0);
        __syncthreads();
    }
    // stage 2: out tile m (16 unique frames) = Cz[m] z, the A operands of a tile through the same two LDS buffers
    const int mt = (Th + 15) >> 4;
    v2f64 gc[CL];
    auto fetch_c = [&](int m) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < CL; ++j) gc[j] = *reinterpret_cast<const v2f64 *>(Cf + (size_t)m * CCH + 2 * tid + 512 * j);
    };
    auto stash_c = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < CL; ++j) *reinterpret_cast<v2f64 *>(&s_frag[buf][2 * tid + 512 * j]) = gc[j];
    };
    fetch_c(0);
    stash_c(0);                                    // (the barrier that ended the last chunk of stage 1 freed both buffers)
    __syncthreads();
    for (int m = 0; m < mt; ++m) {
        if (m + 1 < mt) fetch_c(m + 1);            // the next tile's operands travel while this one is multiplied and stored
        const double *sc = &s_frag[m & 1][lane];
        const int s0 = 16 * m;
        v4f64 o = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < NT; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) o = __builtin_amdgcn_mfma_f64_16x16x4f64(sc[(4 * q + r) * 64], acc[q][r], o, 0, 0, 0);
        }
        if (p < NP) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int sr = s0 + hi + 4 * r;
                if (sr < Th) {
                    const double v = o[r] * amp;
                    out[(size_t)sr * NP + p] = v;
                    if (mirror_n > 0 && sr > 0 && 2 * sr < mirror_n) out[(size_t)(mirror_n - sr) * NP + p] = v;
                }
            }
        }
        if (m + 1 < mt) stash_c((m + 1) & 1);
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------------
// transforms.py:72-79 temporal_bandpass_filter (the IIR alternative to the FFT filter, selectable through
// eulerian_magnification_bandpass(temporal_filter_function=...)): scipy.signal.lfilter(b, a, data, axis=0) * amp.
// One lane per pixel column, the recurrence runs sequentially in t in scipy's transposed direct form II
//   y = z[0] + b[0] x ;  z[i] = z[i+1] + b[i+1] x - a[i+1] y ;  z[n-2] = b[n-1] x - a[n-1] y
// (b, a already divided by a[0], as scipy does), so every value is the same sequence of float64 operations.
// Coefficients are wave-uniform (constant memory through the kernel argument), loads are coalesced across pixels.
// ----------------------------------------------------------------------------------------
constexpr int IIR_MAX = 16;  // coefficients per polynomial (a band-pass of order 6 has 13)
struct IirCoef { double b[IIR_MAX], a[IIR_MAX]; int n; };

RM_KERNEL __launch_bounds__(64) void k_lfilter(const double *x, int T, size_t NP, IirCoef c, double scale, double *y)
{
    const size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= NP) return;
    double z[IIR_MAX];
#pragma unroll
    for (int i = 0; i < IIR_MAX; ++i) z[i] = 0.0;
    double nxt = x[p];
    for (int t = 0; t < T; ++t) {
        const double v = nxt;
        if (t + 1 < T) nxt = x[(size_t)(t + 1) * NP + p];   // one sample ahead of the recurrence
        const double out = z[0] + c.b[0] * v;
#pragma unroll
        for (int i = 0; i < IIR_MAX - 2; ++i)
            if (i < c.n - 2) z[i] = (z[i + 1] + c.b[i + 1] * v) - c.a[i + 1] * out;
        if (c.n >= 2) {
#pragma unroll
            for (int i = 0; i < IIR_MAX - 1; ++i)
                if (i == c.n - 2) z[i] = c.b[i + 1] * v - c.a[i + 1] * out;
        }
        y[(size_t)t * NP + p] = out * scale;
    }
}

}  // namespace rm
