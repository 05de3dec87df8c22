// respmon_amd/csrc/rm_phase_kernels.h -- phase-based motion magnification on the Riesz pyramid (rm_phase_push): the per-pixel work
// between the Laplacian pyramid of a chunk and its collapse.  The rule, operation by operation, is the comment of rm_phase_* in
// include/respmon_hip.h; everything is float64 and every operation rounds once (the library is built with -ffp-contract=off).
//
// The processed levels S .. L-2 of the n frames of a chunk live level-major in every workspace array of this stage: level l is
// [n][h_l][w_l] at element n * off[l] (PhaseGeom), so that one launch covers all of them and the collapse reads a level as the plain
// [n, h, w] array launch_pyr_up expects.
//
//   * k_phase_time<NS, BLUR>: a lane owns one level pixel and walks the n frames.  (Ip, R1p, R2p, Pc, Ps) and the 2 x NS x 2 filter
//     states stay in registers for the whole chunk; they are loaded from the rm_phase object before the first frame (zero on the first
//     push after create / reset) and stored after the last: 5 + 4 nsec planes of [NP].  Per frame it reads I and its four neighbours
//     (the lanes of a wave are 64 consecutive x of one row, so the centre load is coalesced and the neighbours come from the lines the
//     wave and the rows above / below have just fetched), one frame ahead of the arithmetic, and writes A, A Fc, A Fs (BLUR) or
//     Fc, Fs (RM_PHASE_NO_BLUR).  NS = 1 .. 4 are straight-line instances; NS = 8 serves 5 .. 8 sections with the section count tested
//     at run time (uniform), so that the common orders keep their register count.
//   * k_phase_space<BLUR>: a workgroup of 512 threads owns a 64 x 16 tile of one level of one frame.  It stages the three planes with a
//     4-pixel halo (indices reflected 101, repeatedly: a level may be smaller than the halo) in LDS, runs the 9-tap binomial along x for
//     the 16 + 8 staged rows and then along y, forms the quotient, the sine / cosine and the phase shift with R1, R2 recomputed from I,
//     and writes L'.
//   * k_phase_convert<Tout>: the collapsed float64 frames to the output dtype with rm_magnify's conversions (mag_out, rm_magnify.h).
#pragma once
#include "rm_magnify.h"          // mag_out: the conversion / clamp epilogue of rm_magnify
#include "rm_stream_kernels.h"   // SosCoef

namespace rm {

constexpr int PHASE_MAX_LEVELS = 16;   // processed levels of one object
constexpr int PH_TW = 64, PH_TH = 16, PH_HALO = 4, PH_THREADS = 512;
constexpr int PH_SW = PH_TW + 2 * PH_HALO, PH_SH = PH_TH + 2 * PH_HALO;    // the staged tile
constexpr int PH_LDS_DOUBLES = 3 * PH_SH * PH_SW + 3 * PH_SH * PH_TW;      // staged planes + their x-pass: 78 336 bytes

// processed level i (pyramid level S + i): size, element offset inside a frame's [NP] (times n: inside a chunk's workspace array) and
// the first block of the level in the two launches
struct PhaseGeom {
    int nl;
    int h[PHASE_MAX_LEVELS], w[PHASE_MAX_LEVELS];
    unsigned long long off[PHASE_MAX_LEVELS];
    unsigned tb0[PHASE_MAX_LEVELS + 1];   // k_phase_time: h * ceil(w / 64) single-wave blocks per level
    unsigned sb0[PHASE_MAX_LEVELS + 1];   // k_phase_space: ceil(h / 16) * ceil(w / 64) tiles per level
};

__device__ __forceinline__ int phase_level_of(const unsigned *b0, int nl, unsigned b)
{
    int i = 0;
    while (i + 1 < nl && b >= b0[i + 1]) ++i;   // (uniform: a handful of scalar compares)
    return i;
}

// the five values one frame of the time kernel needs
struct PhasePx { double c, l, r, u, d; };
__device__ __forceinline__ PhasePx phase_load(const double *f, size_t ic, size_t il, size_t ir, size_t iu, size_t id)
{
    return PhasePx{f[ic], f[il], f[ir], f[iu], f[id]};
}

// one step of rm_sosfilt's recurrence (rm_stream_kernels.h), from the state in registers, scale 1
template <int NS>
__device__ __forceinline__ double phase_sos_step(const SosCoef &c, double cur, double (&z0)[NS], double (&z1)[NS])
{
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (NS > 4 && s >= c.n) break;   // NS == 8: 5 .. 8 sections, counted at run time
        const double nw = c.b0[s] * cur + z0[s];
        z0[s] = (c.b1[s] * cur - c.a1[s] * nw) + z1[s];
        z1[s] = c.b2[s] * cur - c.a2[s] * nw;
        cur = nw;
    }
    return cur;
}

// grid: g.tb0[g.nl] single-wave workgroups (level, row, 64 columns).  lap: the Laplacian levels of the chunk; pa / pb / pc: A, A Fc, A Fs
// (BLUR) or -, Fc, Fs; state: [5 + 4 c.n][NP].  first: the chunk begins a stream (state starts at zero, frame 0 has no predecessor).
template <int NS, bool BLUR>
__global__ __launch_bounds__(64) void k_phase_time(const double *lap, int n, PhaseGeom g, size_t NP, SosCoef c, int first, double *pa, double *pb,
                                                   double *pc, double *state)
{
    const int li = phase_level_of(g.tb0, g.nl, blockIdx.x);
    const int h = g.h[li], w = g.w[li];
    const unsigned nbx = (unsigned)(w + 63) / 64, rb = blockIdx.x - g.tb0[li];
    const int y = (int)(rb / nbx), x = (int)(rb % nbx) * 64 + (int)threadIdx.x;
    if (x >= w) return;
    const size_t fs = (size_t)h * w, base = (size_t)n * g.off[li];
    const size_t ic = (size_t)y * w + x;
    const size_t il = (size_t)y * w + reflect101(x - 1, w), ir = (size_t)y * w + reflect101(x + 1, w);
    const size_t iu = (size_t)reflect101(y - 1, h) * w + x, id = (size_t)reflect101(y + 1, h) * w + x;
    const size_t p = (size_t)g.off[li] + ic;   // the pixel's place in a state plane
    const int ns = NS > 4 ? c.n : NS;

    double Ip = 0.0, R1p = 0.0, R2p = 0.0, Pc = 0.0, Ps = 0.0;
    double zc0[NS], zc1[NS], zs0[NS], zs1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) { zc0[s] = 0.0; zc1[s] = 0.0; zs0[s] = 0.0; zs1[s] = 0.0; }
    if (!first) {
        Ip = state[p]; R1p = state[NP + p]; R2p = state[2 * NP + p]; Pc = state[3 * NP + p]; Ps = state[4 * NP + p];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (NS > 4 && s >= ns) break;
            zc0[s] = state[(size_t)(5 + 2 * s) * NP + p];
            zc1[s] = state[(size_t)(6 + 2 * s) * NP + p];
            zs0[s] = state[(size_t)(5 + 2 * ns + 2 * s) * NP + p];
            zs1[s] = state[(size_t)(6 + 2 * ns + 2 * s) * NP + p];
        }
    }
    const double *f = lap + base;
    PhasePx nx = phase_load(f, ic, il, ir, iu, id);
    for (int t = 0; t < n; ++t) {
        const PhasePx v = nx;
        if (t + 1 < n) nx = phase_load(f + (size_t)(t + 1) * fs, ic, il, ir, iu, id);   // one frame ahead of the arithmetic
        const double I = v.c;
        const double R1 = 0.5 * (v.r - v.l), R2 = 0.5 * (v.d - v.u);
        double dc = 0.0, ds = 0.0;
        if (!(first && t == 0)) {
            const double re = (I * Ip + R1 * R1p) + R2 * R2p;
            const double qx = Ip * R1 - I * R1p, qy = Ip * R2 - I * R2p;
            const double hyp = sqrt(qx * qx + qy * qy);
            const double d = atan2(hyp, re);
            dc = hyp > 0.0 ? d * (qx / hyp) : 0.0;
            ds = hyp > 0.0 ? d * (qy / hyp) : 0.0;
        }
        Pc += dc; Ps += ds;
        const double Fc = phase_sos_step<NS>(c, Pc, zc0, zc1), Fs = phase_sos_step<NS>(c, Ps, zs0, zs1);
        const size_t o = base + (size_t)t * fs + ic;
        if constexpr (BLUR) {
            const double A = sqrt((I * I + R1 * R1) + R2 * R2);
            pa[o] = A; pb[o] = A * Fc; pc[o] = A * Fs;
        } else {
            pb[o] = Fc; pc[o] = Fs;
        }
        Ip = I; R1p = R1; R2p = R2;
    }
    state[p] = Ip; state[NP + p] = R1p; state[2 * NP + p] = R2p; state[3 * NP + p] = Pc; state[4 * NP + p] = Ps;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (NS > 4 && s >= ns) break;
        state[(size_t)(5 + 2 * s) * NP + p] = zc0[s];
        state[(size_t)(6 + 2 * s) * NP + p] = zc1[s];
        state[(size_t)(5 + 2 * ns + 2 * s) * NP + p] = zs0[s];
        state[(size_t)(6 + 2 * ns + 2 * s) * NP + p] = zs1[s];
    }
}

// the 9-tap binomial (1, 8, 28, 56, 70, 56, 28, 8, 1) / 256 over v[0], v[stride], ...: the left-to-right sum of k[i] * v[i]
__device__ __forceinline__ double phase_blur9(const double *v, int stride)
{
    double acc = (1.0 / 256) * v[0];
    acc += (8.0 / 256) * v[stride];
    acc += (28.0 / 256) * v[2 * stride];
    acc += (56.0 / 256) * v[3 * stride];
    acc += (70.0 / 256) * v[4 * stride];
    acc += (56.0 / 256) * v[5 * stride];
    acc += (28.0 / 256) * v[6 * stride];
    acc += (8.0 / 256) * v[7 * stride];
    acc += (1.0 / 256) * v[8 * stride];
    return acc;
}

// grid: (g.sb0[g.nl] tiles, n frames), PH_THREADS threads; dynamic LDS: PH_LDS_DOUBLES doubles (BLUR; none otherwise).
// out: L' of the processed levels, laid out as lap.
template <bool BLUR>
__global__ __launch_bounds__(PH_THREADS) void k_phase_space(const double *lap, int n, PhaseGeom g, double amp, const double *pa, const double *pb,
                                                     const double *pc, double *out)
{
    HIP_DYNAMIC_SHARED(double, lds)
    const int li = phase_level_of(g.sb0, g.nl, blockIdx.x);
    const int h = g.h[li], w = g.w[li], t = (int)blockIdx.y;
    const unsigned ntx = (unsigned)(w + PH_TW - 1) / PH_TW, rb = blockIdx.x - g.sb0[li];
    const int y0 = (int)(rb / ntx) * PH_TH, x0 = (int)(rb % ntx) * PH_TW;
    const size_t plane = (size_t)n * g.off[li] + (size_t)t * h * w;
    const int tid = (int)threadIdx.x;
    double den = 0.0, nc = 0.0, ns = 0.0;
    const int lx = tid & (PH_TW - 1), ly0 = tid >> 6;   // the thread's column and its first row (rows ly0, ly0 + PH_THREADS / 64, ...)
    if constexpr (BLUR) {
        double *stg = lds, *xp = lds + 3 * PH_SH * PH_SW;
        for (int e = tid; e < PH_SH * PH_SW; e += PH_THREADS) {
            const int sy = e / PH_SW, sx = e - sy * PH_SW;
            const size_t i = plane + (size_t)reflect101(y0 + sy - PH_HALO, h) * w + reflect101(x0 + sx - PH_HALO, w);
            stg[e] = pa[i]; stg[PH_SH * PH_SW + e] = pb[i]; stg[2 * PH_SH * PH_SW + e] = pc[i];
        }
        __syncthreads();
        for (int e = tid; e < 3 * PH_SH * PH_TW; e += PH_THREADS) {   // along x: every staged row of the three planes
            const int k = e / (PH_SH * PH_TW), r = e - k * (PH_SH * PH_TW), sy = r / PH_TW, x = r - sy * PH_TW;
            xp[e] = phase_blur9(stg + (k * PH_SH + sy) * PH_SW + x, 1);
        }
        __syncthreads();
    }
#pragma unroll
    for (int rr = 0; rr < PH_TH / (PH_THREADS / 64); ++rr) {
        const int ly = ly0 + (PH_THREADS / 64) * rr, y = y0 + ly, x = x0 + lx;
        if (y >= h || x >= w) continue;
        const size_t i = plane + (size_t)y * w + x;
        double bc, bs;
        if constexpr (BLUR) {
            const double *xp = lds + 3 * PH_SH * PH_SW;
            den = phase_blur9(xp + ly * PH_TW + lx, PH_TW);       // along y: staged rows ly .. ly + 8 are level rows y - 4 .. y + 4
            nc = phase_blur9(xp + (PH_SH + ly) * PH_TW + lx, PH_TW);
            ns = phase_blur9(xp + (2 * PH_SH + ly) * PH_TW + lx, PH_TW);
            bc = den > 0.0 ? nc / den : 0.0;
            bs = den > 0.0 ? ns / den : 0.0;
        } else {
            bc = pb[i]; bs = pc[i];
        }
        const double *f = lap + plane;
        const double I = f[(size_t)y * w + x];
        const double R1 = 0.5 * (f[(size_t)y * w + reflect101(x + 1, w)] - f[(size_t)y * w + reflect101(x - 1, w)]);
        const double R2 = 0.5 * (f[(size_t)reflect101(y + 1, h) * w + x] - f[(size_t)reflect101(y - 1, h) * w + x]);
        const double m = sqrt(bc * bc + bs * bs);
        const double am = amp * m;
        double sn, cs;
        sincos(am, &sn, &cs);
        const double ux = m > 0.0 ? bc / m : 0.0, uy = m > 0.0 ? bs / m : 0.0;
        out[i] = I * cs - (R1 * ux + R2 * uy) * sn;
    }
}

template <typename Tout>
__global__ __launch_bounds__(256) void k_phase_convert(const double *v, size_t count, Tout *out)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) out[i] = mag_out<Tout>(v[i]);
}

}  // namespace rm
