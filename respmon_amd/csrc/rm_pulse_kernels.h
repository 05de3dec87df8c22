// respmon_amd/csrc/rm_pulse_kernels.h -- the pulse beside the breath (rm_pulse.hip): per-channel sums of a BGR buffer over the blocks of
// a grid or over rectangles, and the POS projection ("plane orthogonal to skin": Wang, den Brinker, Stuijk, de Haan, Algorithmic
// Principles of Remote PPG, IEEE TBME 2017) that turns those sums into a pulse signal.  The rule, operation by operation, is the
// comment of rm_pulse_pos in include/respmon_hip.h; DESIGN.md 4.16 has the bytes model.
#pragma once
#include "../../include/respmon_hip.h"
#include "rm_kernels.h"
#include "rm_down_chain.h"   // Raw16

namespace rm {

// ----------------------------------------------------------------------------------------
// block sums: sums[n][by][bx][c] = sum of channel c over the pixels of frame n inside block (by, bx)
// ----------------------------------------------------------------------------------------
// 48 bytes are 16 whole pixels: B G R B | G R B G | R B G R, so dword j of a 16-pixel group has the phase j % 3 and byte i of it
// carries channel (j + i) % 3.  v_dot4_u32_u8 against these byte weights adds the bytes of one channel to an accumulator.
__host__ __device__ constexpr unsigned bgr_channel_weights(int phase, int c)
{
    unsigned m = 0;
    for (int i = 0; i < 4; ++i)
        if ((phase + i) % 3 == c) m |= 1u << (8 * i);
    return m;
}

// one row of a lane's 16-pixel group into its accumulators: acc[q][c], q = the block of the NB the group spans (12 / NB dwords each)
template <int NB>
__device__ __forceinline__ void bgr_row_acc(const Raw16 &a, const Raw16 &b, const Raw16 &c, unsigned (&acc)[NB][3])
{
    const unsigned d[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 12; ++j)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            acc[j / (12 / NB)][ch] = __builtin_amdgcn_udot4(d[j], bgr_channel_weights(j % 3, ch), acc[j / (12 / NB)][ch], false);
}

// A lane owns the 16-pixel group `g` (columns 16 g .. 16 g + 15) of one block row of one frame and adds its rows in registers down the
// block: BLOCK >= 16 puts BLOCK / 16 neighbouring lanes on one block (folded by shuffles, one store per block and channel), BLOCK < 16
// puts 16 / BLOCK blocks on a lane.  A wave is 64 groups of one block row (threadIdx.y: four block rows per workgroup); the groups
// are padded to whole blocks (G <= Wb * BLOCK / 16), so the lanes of a block never straddle a wave.  Every block of the output is
// written by exactly one lane: nothing is zeroed first, no atomics.
//   FAST: W % 16 == 0 and a 16-byte aligned buffer -- every group of every row is three aligned 16-byte loads, four rows in flight;
//   otherwise the same lanes read their pixels byte by byte (any W, any alignment; partial groups and blocks at the right edge).
// rows = N * Hb; grid (ceil(rows / 4), ceil(Wb * max(BLOCK / 16, 1) / 64)), block (64, 4).
template <int BLOCK, bool FAST>
__global__ __launch_bounds__(256) void k_bgr_block_sums(const uint8_t *frames, int H, int W, int Hb, int Wb, int G, unsigned rows, uint32_t *sums)
{
    constexpr int NB = BLOCK >= 16 ? 1 : 16 / BLOCK;
    constexpr int L = BLOCK >= 16 ? BLOCK / 16 : 1;
    const unsigned row = blockIdx.x * 4 + threadIdx.y;
    const int g = (int)(blockIdx.y * 64 + threadIdx.x);
    const bool live = row < rows && g < G;
    unsigned acc[NB][3];
#pragma unroll
    for (int q = 0; q < NB; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0u;
    if (live) {
        const int n = (int)(row / (unsigned)Hb), by = (int)(row - (unsigned)n * (unsigned)Hb);
        const int y0 = by * BLOCK, y1 = min(H, y0 + BLOCK);
        const size_t pitch = (size_t)W * 3;
        const uint8_t *p = frames + ((size_t)n * H + y0) * pitch + (size_t)g * 48;
        if (FAST) {
            int y = y0;
            for (; y + 4 <= y1; y += 4, p += 4 * pitch) {
                Raw16 v[4][3];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) v[r][k] = *(const Raw16 *)(p + r * pitch + 16 * k);
#pragma unroll
                for (int r = 0; r < 4; ++r) bgr_row_acc<NB>(v[r][0], v[r][1], v[r][2], acc);
            }
            for (; y < y1; ++y, p += pitch)
                bgr_row_acc<NB>(*(const Raw16 *)p, *(const Raw16 *)(p + 16), *(const Raw16 *)(p + 32), acc);
        } else {
            const int npx = min(16, W - 16 * g);
            for (int y = y0; y < y1; ++y, p += pitch)
                for (int i = 0; i < npx; ++i) {
                    const int q = BLOCK >= 16 ? 0 : i / BLOCK;
                    acc[q][0] += p[3 * i];
                    acc[q][1] += p[3 * i + 1];
                    acc[q][2] += p[3 * i + 2];
                }
        }
    }
    // (every lane of the wave takes part: a dead lane adds zeros)
#pragma unroll
    for (int m = 1; m < L; m <<= 1)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[0][ch] += __shfl_xor(acc[0][ch], m);
    if (live && g % L == 0) {
        const int bx0 = BLOCK >= 16 ? g / L : g * NB;
#pragma unroll
        for (int q = 0; q < NB; ++q)
            if (bx0 + q < Wb) {
                uint32_t *o = sums + ((size_t)row * Wb + (bx0 + q)) * 3;
                o[0] = acc[q][0]; o[1] = acc[q][1]; o[2] = acc[q][2];
            }
    }
}

// ----------------------------------------------------------------------------------------
// rectangle sums: sums[n][k][c] over rectangle k of frame n; workgroup n * K + k, a wave per row, a lane per column
// ----------------------------------------------------------------------------------------
struct PulseRois { int v[4 * RM_MAX_ROIS]; };   // x, y, w, h per rectangle: a kernel argument, so the caller's list is read before the call returns

RM_KERNEL __launch_bounds__(256) void k_bgr_roi_sums(const uint8_t *frames, size_t frame_bytes, int W, PulseRois rois, int K, uint32_t *sums)
{
    __shared__ unsigned s_part[4][3];
    const int k = (int)(blockIdx.x % (unsigned)K);
    const size_t n = blockIdx.x / (unsigned)K;
    const int x = rois.v[4 * k], y = rois.v[4 * k + 1], w = rois.v[4 * k + 2], h = rois.v[4 * k + 3];
    const uint8_t *f = frames + n * frame_bytes;
    unsigned a[3] = {0u, 0u, 0u};
    for (int r = (int)(threadIdx.x >> 6); r < h; r += 4) {
        const uint8_t *p = f + ((size_t)(y + r) * W + x) * 3;
        for (int c = (int)(threadIdx.x & 63); c < w; c += 64) {
            a[0] += p[3 * c];
            a[1] += p[3 * c + 1];
            a[2] += p[3 * c + 2];
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a[ch] += __shfl_xor(a[ch], m);
    if ((threadIdx.x & 63) == 0)
        for (int ch = 0; ch < 3; ++ch) s_part[threadIdx.x >> 6][ch] = a[ch];
    __syncthreads();
    if (threadIdx.x < 3) sums[(size_t)blockIdx.x * 3 + threadIdx.x] = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
}

// ----------------------------------------------------------------------------------------
// POS (include/respmon_hip.h rm_pulse_pos).  s[N][NP][3] uint32; columns are the fast index of both kernels, so a wave reads
// [.][p][3] coalesced.  Every operation below is one float64 rounding in the order of the rule.
// ----------------------------------------------------------------------------------------
// the two projections of frame k of a window: x_c = (s_c * l) / S_c (the product is exact), S1 = x_G - x_B, S2 = (x_G + x_B) - 2 x_R
__device__ __forceinline__ void pos_project(const uint32_t *s3, double dl, const double *S, double &S1, double &S2)
{
    const double xb = ((double)s3[0] * dl) / S[0], xg = ((double)s3[1] * dl) / S[1], xr = ((double)s3[2] * dl) / S[2];
    S1 = xg - xb;
    S2 = (xg + xb) - 2.0 * xr;
}

// a lane per (column p, window n = blockIdx.y): S_c (exact, stored as float64; a window with a zero S_c is skipped by everyone who
// reads it) and a = sqrt(v1 / v2).  Sw[n][p][3], alpha[n][p].
RM_KERNEL __launch_bounds__(256) void k_pos_windows(const uint32_t *s, size_t NP, int l, double *Sw, double *alpha)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const size_t n = blockIdx.y;
    const uint32_t *q = s + (n * NP + p) * 3;
    unsigned long long Si[3] = {0ull, 0ull, 0ull};
    for (int k = 0; k < l; ++k)
        for (int c = 0; c < 3; ++c) Si[c] += q[(size_t)k * NP * 3 + c];
    const double S[3] = {(double)Si[0], (double)Si[1], (double)Si[2]};
    double a = 0.0;
    if (Si[0] != 0 && Si[1] != 0 && Si[2] != 0) {
        const double dl = (double)l;
        double v1 = 0.0, v2 = 0.0;
        for (int k = 0; k < l; ++k) {
            double S1, S2;
            pos_project(q + (size_t)k * NP * 3, dl, S, S1, S2);
            v1 = v1 + S1 * S1;
            v2 = v2 + S2 * S2;
        }
        a = v2 > 0.0 ? sqrt(v1 / v2) : 0.0;
    }
    double *o = Sw + (n * NP + p) * 3;
    o[0] = S[0]; o[1] = S[1]; o[2] = S[2];
    alpha[n * NP + p] = a;
}

// a lane per (column p, frame t = blockIdx.y): the overlap-add over the at most l windows that hold frame t, ascending n
RM_KERNEL __launch_bounds__(256) void k_pos_overlap_add(const uint32_t *s, int N, size_t NP, int l, const double *Sw, const double *alpha, double *out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    const int t = (int)blockIdx.y;
    const uint32_t *s3 = s + ((size_t)t * NP + p) * 3;
    const double dl = (double)l;
    double acc = 0.0;
    const int n1 = min(t, N - l);
    for (int n = max(0, t - l + 1); n <= n1; ++n) {
        const double *S = Sw + ((size_t)n * NP + p) * 3;
        if (S[0] == 0.0 || S[1] == 0.0 || S[2] == 0.0) continue;
        double S1, S2;
        pos_project(s3, dl, S, S1, S2);
        acc = acc + (S1 + alpha[(size_t)n * NP + p] * S2);
    }
    out[(size_t)t * NP + p] = acc;
}

}  // namespace rm
