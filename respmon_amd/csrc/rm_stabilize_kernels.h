// respmon_amd/csrc/rm_stabilize_kernels.h -- rm_stab_*, rm_warp_shift: the global shift of a frame against a fixed reference frame
// (translation-only Gauss-Newton, coarse to fine on the Gaussian pyramid) and the bilinear warp that takes it out (the rule, operation
// by operation: include/respmon_hip.h).  Everything is float64 and every operation rounds once (the library is built with
// -ffp-contract=off).
//
// A chunk of n frames lives in ONE workspace array: Gaussian level j of the chunk is [C][h_j][w_j] at element StabGeom::off[j]
// (C: the chunk capacity of the call), j = 0 .. level_coarse.  The reference's levels level_fine .. level_coarse and their
// (a, bb, c, det) live in the session's own allocation: four doubles per level index, then R_l at StabGeom::roff[l].
//
//   * k_stab_gray<Tin>: G_0 = the float64 gray frame (load_px: the conversions of the pyramid entry points; RM_BGR8: the integer
//     cvtColor of k_bgr_to_gray, then * (1./255)).
//   * k_stab_down: G_j = pyrDown(G_j-1), the tile body of k_pyr_down (rm_pyr_kernels.h pyr_down_tile), over (tile, frame).
//   * k_stab_hsums / k_stab_hfold: a, bb, c of a reference level.  A workgroup of 256 owns a 64 x 16 tile of the LEVEL (not of the
//     region), wave v rows 4 v .. 4 v + 3 of it, a lane one column: a lane adds its four rows top down (pixels outside the region add
//     nothing), the wave folds on DPP (wave_reduce, rm_kernels.h), the four waves through LDS in wave order: one partial per tile.
//     One wave then folds the partials -- lane k takes tiles k, k + 64, ... in that order, then wave_reduce -- and forms det.
//   * k_stab_resid: the same tiling over (tile, frame) for gx, gy at the frame's present shift; Rx, Ry are formed again from R.
//   * k_stab_update: one wave per frame folds that frame's partials the same way and does the 2 x 2 update, the clamp and the flags
//     on the device.  The shift is kept in level-0 pixels between the launches (s = d / 2^l and d = s 2^l are exact).
//   * k_stab_warp<Tin, Tout> / k_stab_warp_bgr: out = bilinear(frame, x + d.x, y + d.y), converted by rm_magnify's output rules
//     (mag_out); a lane per output element, a workgroup 256 consecutive elements of one row.
// The tiling and both orders are functions of (h_l, w_l) alone: a sum does not depend on N, the chunking or the frame's place in a call.
// No floating-point atomics anywhere.
#pragma once
#include "rm_pyr_kernels.h"   // pyr_down_tile
#include "rm_magnify.h"       // mag_out, MagPx<bgr8_t>::widen

namespace rm {

constexpr int STAB_MAX_LEVEL = 8;
constexpr int STAB_LEVELS = STAB_MAX_LEVEL + 1;           // G_0 .. G_8
constexpr int STAB_TW = 64, STAB_RPW = 4, STAB_TH = 4 * STAB_RPW;   // the reduction tile: 64 x 16, four rows per wave
constexpr int STAB_FLAG_LEVEL_SKIPPED = 1, STAB_FLAG_CLAMPED = 2;

struct StabGeom {
    int lc, lf;
    int h[STAB_LEVELS], w[STAB_LEVELS];
    unsigned long long off[STAB_LEVELS];    // element offset of [C][h_j][w_j] in the chunk workspace
    unsigned long long roff[STAB_LEVELS];   // element offset of R_l in the session's allocation (l = lf .. lc)
};

template <typename Tin> __device__ __forceinline__ double stab_gray(const Tin *f, size_t i) { return load_px(f, i); }
template <> __device__ __forceinline__ double stab_gray<bgr8_t>(const bgr8_t *f, size_t i)
{
    return MagPx<bgr8_t>::widen(reinterpret_cast<const uint8_t *>(f) + 3 * i);
}

// grid: (blocks, n)
template <typename Tin>
__global__ __launch_bounds__(256) void k_stab_gray(const Tin *frames, size_t px, double *g0)
{
    const Tin *f = frames + (size_t)blockIdx.y * px;
    double *g = g0 + (size_t)blockIdx.y * px;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < px; i += (size_t)gridDim.x * 256) g[i] = stab_gray(f, i);
}

// grid: (tiles of G_j, n)
__global__ __launch_bounds__(256) void k_stab_down(StabGeom g, double *wsp, int j)
{
    __shared__ double s_src[PD_SY][PD_SX + 1];
    __shared__ double s_row[PD_SY][PD_TX];
    const int h = g.h[j - 1], w = g.w[j - 1], dh = g.h[j], dw = g.w[j];
    const unsigned ntx = (unsigned)(dw + PD_TX - 1) / PD_TX;
    const int ty0 = (int)(blockIdx.x / ntx) * PD_TY, tx0 = (int)(blockIdx.x % ntx) * PD_TX;
    const double *sp = wsp + g.off[j - 1] + (size_t)blockIdx.y * h * w;
    double *dp = wsp + g.off[j] + (size_t)blockIdx.y * dh * dw;
    pyr_down_tile(sp, h, w, dp, dh, dw, ty0, tx0, s_src, s_row);
}

// the sums of one workgroup: NC values per lane -> one value per tile in out[0 .. NC), in the fixed order lanes (DPP), then waves
template <int NC>
__device__ __forceinline__ void stab_block_fold(double (&v)[NC], double (&red)[4][NC], double *out)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const auto add = [](double o, double x) { return o + x; };
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = wave_reduce(v[c], add);
    if (lane == 0)
        for (int c = 0; c < NC; ++c) red[wave][c] = v[c];
    __syncthreads();
    if ((int)threadIdx.x < NC) {
        const int c = (int)threadIdx.x;
        out[c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    }
}

// the partials of NC sums, [ntiles][NC], folded by ONE wave: lane k adds tiles k, k + 64, ... in that order, then the lanes on DPP
template <int NC>
__device__ __forceinline__ void stab_wave_fold(const double *part, int ntiles, double (&s)[NC])
{
    const int lane = (int)threadIdx.x & 63;
    const auto add = [](double o, double x) { return o + x; };
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double acc = 0.0;
        for (int j = lane; j < ntiles; j += 64) acc += part[(size_t)j * NC + c];
        s[c] = wave_reduce(acc, add);
    }
}

// grid: (tiles of the level); R: h x w; b: the border of the region; part: [ntiles][3]
__global__ __launch_bounds__(256) void k_stab_hsums(const double *R, int h, int w, int b, double *part)
{
    __shared__ double red[4][3];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int ntx = (w + STAB_TW - 1) / STAB_TW;
    const int x = (int)(blockIdx.x % (unsigned)ntx) * STAB_TW + lane, y0 = (int)(blockIdx.x / (unsigned)ntx) * STAB_TH + wave * STAB_RPW;
    double v[3] = {0.0, 0.0, 0.0};
    for (int r = 0; r < STAB_RPW; ++r) {
        const int y = y0 + r;
        if (x >= b && x <= w - 1 - b && y >= b && y <= h - 1 - b) {
            const double *p = R + (size_t)y * w + x;
            const double Rx = 0.5 * (p[1] - p[-1]), Ry = 0.5 * (p[w] - p[-w]);
            v[0] += Rx * Rx; v[1] += Rx * Ry; v[2] += Ry * Ry;
        }
    }
    stab_block_fold<3>(v, red, part + (size_t)blockIdx.x * 3);
}

// one wave; hs: (a, bb, c, det) of the level
__global__ __launch_bounds__(64) void k_stab_hfold(const double *part, int ntiles, double *hs)
{
    double s[3];
    stab_wave_fold<3>(part, ntiles, s);
    if (threadIdx.x == 0) {
        hs[0] = s[0]; hs[1] = s[1]; hs[2] = s[2];
        hs[3] = s[0] * s[2] - s[1] * s[1];
    }
}

// clamp(v, 0, n - 1) of an integral double as an int; a NaN gives 0, so that no shift can lead a load out of the image
__device__ __forceinline__ int stab_clamp_index(double v, int n) { return v >= 0.0 ? (v <= (double)(n - 1) ? (int)v : n - 1) : 0; }

// bilinear(F, fx, fy) of the rule; F(j, i) loads row j, column i of an h x w image as float64
template <typename Img>
__device__ __forceinline__ double stab_bilinear(const Img &F, int h, int w, double fx, double fy)
{
    const double x0 = floor(fx), y0 = floor(fy);
    const double ax = fx - x0, ay = fy - y0;
    const int i0 = stab_clamp_index(x0, w), i1 = stab_clamp_index(x0 + 1.0, w);
    const int j0 = stab_clamp_index(y0, h), j1 = stab_clamp_index(y0 + 1.0, h);
    const double f00 = F(j0, i0), f01 = F(j0, i1), f10 = F(j1, i0), f11 = F(j1, i1);
    return ((1.0 - ax) * f00 + ax * f01) * (1.0 - ay) + ((1.0 - ax) * f10 + ax * f11) * ay;
}

__global__ __launch_bounds__(64) void k_stab_init(double *d, int32_t *flags, int n, int base_flags)
{
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= n) return;
    d[2 * i] = 0.0; d[2 * i + 1] = 0.0;
    flags[i] = base_flags;
}

// grid: (tiles of level l, n); inv = 1 / 2^l; d: [n][2] in level-0 pixels; part: [n][ntiles][2]
__global__ __launch_bounds__(256) void k_stab_resid(StabGeom g, const double *wsp, const double *state, int l, int b, double inv, const double *d,
                                                    double *part)
{
    __shared__ double red[4][2];
    const int h = g.h[l], w = g.w[l];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int ntx = (w + STAB_TW - 1) / STAB_TW;
    const int x = (int)(blockIdx.x % (unsigned)ntx) * STAB_TW + lane, y0 = (int)(blockIdx.x / (unsigned)ntx) * STAB_TH + wave * STAB_RPW;
    const double sx = d[2 * (size_t)blockIdx.y] * inv, sy = d[2 * (size_t)blockIdx.y + 1] * inv;
    const double *R = state + g.roff[l];
    const GlobalImg F{wsp + g.off[l] + (size_t)blockIdx.y * h * w, w};
    double v[2] = {0.0, 0.0};
    for (int r = 0; r < STAB_RPW; ++r) {
        const int y = y0 + r;
        if (x >= b && x <= w - 1 - b && y >= b && y <= h - 1 - b) {
            const double *p = R + (size_t)y * w + x;
            const double Rx = 0.5 * (p[1] - p[-1]), Ry = 0.5 * (p[w] - p[-w]);
            const double e = stab_bilinear(F, h, w, (double)x + sx, (double)y + sy) - p[0];
            v[0] += Rx * e; v[1] += Ry * e;
        }
    }
    stab_block_fold<2>(v, red, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

// grid: (n), one wave per frame.  hs: (a, bb, c, det) of the level; lim = max_shift / 2^l; scale = 2^l, inv = 1 / 2^l
__global__ __launch_bounds__(64) void k_stab_update(const double *part, int ntiles, const double *hs, double lim, double scale, double inv,
                                                    int last_of_fine, double *d, int32_t *flags)
{
    double gsum[2];
    stab_wave_fold<2>(part + (size_t)blockIdx.x * ntiles * 2, ntiles, gsum);
    if (threadIdx.x != 0) return;
    const double a = hs[0], bb = hs[1], c = hs[2], det = hs[3];
    if (!(det > 0.0 && det <= 1.7976931348623157e308)) {   // not finite or not > 0: the level is skipped
        flags[blockIdx.x] |= STAB_FLAG_LEVEL_SKIPPED;
        return;
    }
    const double gx = gsum[0], gy = gsum[1];
    double sx = d[2 * (size_t)blockIdx.x] * inv, sy = d[2 * (size_t)blockIdx.x + 1] * inv;
    sx = sx - (c * gx - bb * gy) / det;
    sy = sy - (a * gy - bb * gx) / det;
    const bool clamped = sx < -lim || sx > lim || sy < -lim || sy > lim;
    sx = sx < -lim ? -lim : (sx > lim ? lim : sx);
    sy = sy < -lim ? -lim : (sy > lim ? lim : sy);
    d[2 * (size_t)blockIdx.x] = sx * scale; d[2 * (size_t)blockIdx.x + 1] = sy * scale;
    if (last_of_fine && clamped) flags[blockIdx.x] |= STAB_FLAG_CLAMPED;
}

template <typename Tin> struct StabFrame {
    const Tin *p; int w;
    __device__ __forceinline__ double operator()(int j, int i) const { return load_px(p, (size_t)j * w + i); }
};
struct StabChannel {   // one channel of a BGR frame: k * (1./255)
    const uint8_t *p; int w;
    __device__ __forceinline__ double operator()(int j, int i) const { return (double)p[((size_t)j * w + i) * 3] * (1.0 / 255); }
};

// grid: (ceil(W / 256), rows, n), a workgroup 256 consecutive pixels of ONE row (no division per pixel; a wave stores 64 consecutive
// elements); rows beyond the grid's y limit are taken in further passes.  d: [n][2]
template <typename Tin, typename Tout>
__global__ __launch_bounds__(256) void k_stab_warp(const Tin *frames, int H, int W, const double *d, Tout *out)
{
    const int x = (int)(blockIdx.x * 256 + threadIdx.x);
    if (x >= W) return;
    const size_t px = (size_t)H * W;
    const StabFrame<Tin> F{frames + (size_t)blockIdx.z * px, W};
    const double fx = (double)x + d[2 * (size_t)blockIdx.z], dy = d[2 * (size_t)blockIdx.z + 1];
    Tout *o = out + (size_t)blockIdx.z * px;
    for (int y = (int)blockIdx.y; y < H; y += (int)gridDim.y) o[(size_t)y * W + x] = mag_out<Tout>(stab_bilinear(F, H, W, fx, (double)y + dy));
}

// the colour form: grid (ceil(3 W / 256), rows, n), a lane per output byte of one row, channel by channel
__global__ __launch_bounds__(256) void k_stab_warp_bgr(const uint8_t *frames, int H, int W, const double *d, uint8_t *out)
{
    const int e = (int)(blockIdx.x * 256 + threadIdx.x);
    if (e >= 3 * W) return;
    const int x = e / 3, ch = e - 3 * x;
    const size_t px = (size_t)H * W;
    const StabChannel F{frames + (size_t)blockIdx.z * px * 3 + ch, W};
    const double fx = (double)x + d[2 * (size_t)blockIdx.z], dy = d[2 * (size_t)blockIdx.z + 1];
    uint8_t *o = out + (size_t)blockIdx.z * px * 3;
    for (int y = (int)blockIdx.y; y < H; y += (int)gridDim.y) o[(size_t)y * 3 * W + e] = mag_out<uint8_t>(stab_bilinear(F, H, W, fx, (double)y + dy));
}

// ---- rm_stab_sim_*, rm_warp_similarity: the similarity model (rotation, zoom, shift) beside the shift model above.  Parameters
// p = (p0, p1, tx, ty), p0 = s cos(theta) - 1, p1 = s sin(theta); between the launches the shift d = (tx, ty) [n][2] and the linear part
// q = (p0, p1) [n][2] are kept apart, so that the levels above level_linear run k_stab_resid / k_stab_update as they are.
//   * k_stab_hsums_sim / k_stab_hfold_sim: the ten sums H_ij = sum J_i J_j (i >= j) of a reference level, tiled and folded as above; the
//     one wave that folds the tiles also factors H = L D L^T and stores (L10, L20, L21, L30, L31, L32, D0 .. D3, valid) of the level.
//   * k_stab_resid_sim: g_i = sum J_i e at the frame's present parameters; the taps are gathered (the positions form no grid), every
//     index through stab_clamp_index.
//   * k_stab_update_sim: one wave per frame folds the tiles, does the two substitutions, the clamps and the flags.
//   * k_stab_pack_sim: (q, d) -> params [n][4], what the warp reads and the caller gets.
//   * k_stab_warp_sim<Tin, Tout> / k_stab_warp_sim_bgr: out = bilinear(frame, fx, fy) at the level-0 position of the rule.
constexpr int STAB_FLAG_LINEAR_CLAMPED = 4;
constexpr int STAB_SIM_HDR = 16;   // doubles per level in the session's header: (a, bb, c, det) of a shift level, or L (6), D (4), valid

// the position in the frame of reference pixel (c.x + u, c.y + v): fx = (cx + (m u - p1 v)) + tx, fy = (cy + (p1 u + m v)) + ty
__device__ __forceinline__ double stab_sim_fx(double cx, double u, double v, double m, double p1, double tx) { return (cx + (m * u - p1 * v)) + tx; }
__device__ __forceinline__ double stab_sim_fy(double cy, double u, double v, double m, double p1, double ty) { return (cy + (p1 * u + m * v)) + ty; }

// grid: (tiles of the level); R: h x w; b: the border of the region; (cx, cy): the centre in level pixels; part: [ntiles][10]
__global__ __launch_bounds__(256) void k_stab_hsums_sim(const double *R, int h, int w, int b, double cx, double cy, double *part)
{
    __shared__ double red[4][10];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int ntx = (w + STAB_TW - 1) / STAB_TW;
    const int x = (int)(blockIdx.x % (unsigned)ntx) * STAB_TW + lane, y0 = (int)(blockIdx.x / (unsigned)ntx) * STAB_TH + wave * STAB_RPW;
    double s[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < STAB_RPW; ++r) {
        const int y = y0 + r;
        if (x >= b && x <= w - 1 - b && y >= b && y <= h - 1 - b) {
            const double *p = R + (size_t)y * w + x;
            const double Rx = 0.5 * (p[1] - p[-1]), Ry = 0.5 * (p[w] - p[-w]);
            const double u = (double)x - cx, v = (double)y - cy;
            const double J[4] = {Rx * u + Ry * v, Ry * u - Rx * v, Rx, Ry};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) s[k++] += J[i] * J[j];
        }
    }
    stab_block_fold<10>(s, red, part + (size_t)blockIdx.x * 10);
}

// one wave; hs: STAB_SIM_HDR doubles of the level.  H = L D L^T row by row, no square root; every inner sum left to right
__global__ __launch_bounds__(64) void k_stab_hfold_sim(const double *part, int ntiles, double *hs)
{
    double s[10];
    stab_wave_fold<10>(part, ntiles, s);
    if (threadIdx.x != 0) return;
    const double H00 = s[0], H10 = s[1], H11 = s[2], H20 = s[3], H21 = s[4], H22 = s[5], H30 = s[6], H31 = s[7], H32 = s[8], H33 = s[9];
    const double D0 = H00;
    const double L10 = H10 / D0;
    const double D1 = H11 - (L10 * L10) * D0;
    const double L20 = H20 / D0;
    const double L21 = (H21 - (L20 * L10) * D0) / D1;
    const double D2 = H22 - ((L20 * L20) * D0 + (L21 * L21) * D1);
    const double L30 = H30 / D0;
    const double L31 = (H31 - (L30 * L10) * D0) / D1;
    const double L32 = (H32 - ((L30 * L20) * D0 + (L31 * L21) * D1)) / D2;
    const double D3 = H33 - (((L30 * L30) * D0 + (L31 * L31) * D1) + (L32 * L32) * D2);
    const double big = 1.7976931348623157e308;
    const bool ok = D0 > 0.0 && D0 <= big && D1 > 0.0 && D1 <= big && D2 > 0.0 && D2 <= big && D3 > 0.0 && D3 <= big;
    hs[0] = L10; hs[1] = L20; hs[2] = L21; hs[3] = L30; hs[4] = L31; hs[5] = L32;
    hs[6] = D0; hs[7] = D1; hs[8] = D2; hs[9] = D3;
    hs[10] = ok ? 1.0 : 0.0;
}

// grid: (tiles of level l, n); inv = 1 / 2^l; d, q: [n][2], d in level-0 pixels; (cx, cy): the centre in level pixels; part: [n][ntiles][4]
__global__ __launch_bounds__(256) void k_stab_resid_sim(StabGeom g, const double *wsp, const double *state, int l, int b, double inv, double cx, double cy,
                                                        const double *d, const double *q, double *part)
{
    __shared__ double red[4][4];
    const int h = g.h[l], w = g.w[l];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int ntx = (w + STAB_TW - 1) / STAB_TW;
    const int x = (int)(blockIdx.x % (unsigned)ntx) * STAB_TW + lane, y0 = (int)(blockIdx.x / (unsigned)ntx) * STAB_TH + wave * STAB_RPW;
    const double sx = d[2 * (size_t)blockIdx.y] * inv, sy = d[2 * (size_t)blockIdx.y + 1] * inv;
    const double m = 1.0 + q[2 * (size_t)blockIdx.y], p1 = q[2 * (size_t)blockIdx.y + 1];
    const double *R = state + g.roff[l];
    const GlobalImg F{wsp + g.off[l] + (size_t)blockIdx.y * h * w, w};
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < STAB_RPW; ++r) {
        const int y = y0 + r;
        if (x >= b && x <= w - 1 - b && y >= b && y <= h - 1 - b) {
            const double *p = R + (size_t)y * w + x;
            const double Rx = 0.5 * (p[1] - p[-1]), Ry = 0.5 * (p[w] - p[-w]);
            const double u = (double)x - cx, v = (double)y - cy;
            const double e = stab_bilinear(F, h, w, stab_sim_fx(cx, u, v, m, p1, sx), stab_sim_fy(cy, u, v, m, p1, sy)) - p[0];
            s[0] += (Rx * u + Ry * v) * e; s[1] += (Ry * u - Rx * v) * e; s[2] += Rx * e; s[3] += Ry * e;
        }
    }
    stab_block_fold<4>(s, red, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

// grid: (n), one wave per frame.  hs: the level's header; lim = max_shift / 2^l; lin = max_linear; scale = 2^l, inv = 1 / 2^l
__global__ __launch_bounds__(64) void k_stab_update_sim(const double *part, int ntiles, const double *hs, double lim, double lin, double scale, double inv,
                                                        int last_of_fine, double *d, double *q, int32_t *flags)
{
    double gs[4];
    stab_wave_fold<4>(part + (size_t)blockIdx.x * ntiles * 4, ntiles, gs);
    if (threadIdx.x != 0) return;
    if (!(hs[10] == 1.0)) {   // a D_j not finite or not > 0: the level is skipped
        flags[blockIdx.x] |= STAB_FLAG_LEVEL_SKIPPED;
        return;
    }
    const double L10 = hs[0], L20 = hs[1], L21 = hs[2], L30 = hs[3], L31 = hs[4], L32 = hs[5];
    // L z = g
    const double z0 = gs[0];
    const double z1 = gs[1] - L10 * z0;
    const double z2 = gs[2] - (L20 * z0 + L21 * z1);
    const double z3 = gs[3] - ((L30 * z0 + L31 * z1) + L32 * z2);
    // y = z / D
    const double y0 = z0 / hs[6], y1 = z1 / hs[7], y2 = z2 / hs[8], y3 = z3 / hs[9];
    // L^T x = y
    const double x3 = y3;
    const double x2 = y2 - L32 * x3;
    const double x1 = y1 - (L21 * x2 + L31 * x3);
    const double x0 = y0 - ((L10 * x1 + L20 * x2) + L30 * x3);
    double p0 = q[2 * (size_t)blockIdx.x] - x0, p1 = q[2 * (size_t)blockIdx.x + 1] - x1;
    double sx = d[2 * (size_t)blockIdx.x] * inv - x2, sy = d[2 * (size_t)blockIdx.x + 1] * inv - x3;
    const bool lin_clamped = p0 < -lin || p0 > lin || p1 < -lin || p1 > lin;
    const bool clamped = sx < -lim || sx > lim || sy < -lim || sy > lim;
    p0 = p0 < -lin ? -lin : (p0 > lin ? lin : p0);
    p1 = p1 < -lin ? -lin : (p1 > lin ? lin : p1);
    sx = sx < -lim ? -lim : (sx > lim ? lim : sx);
    sy = sy < -lim ? -lim : (sy > lim ? lim : sy);
    q[2 * (size_t)blockIdx.x] = p0; q[2 * (size_t)blockIdx.x + 1] = p1;
    d[2 * (size_t)blockIdx.x] = sx * scale; d[2 * (size_t)blockIdx.x + 1] = sy * scale;
    if (last_of_fine && clamped) flags[blockIdx.x] |= STAB_FLAG_CLAMPED;
    if (last_of_fine && lin_clamped) flags[blockIdx.x] |= STAB_FLAG_LINEAR_CLAMPED;
}

// params[i] = (q[i], d[i]) = (p0, p1, tx, ty)
__global__ __launch_bounds__(64) void k_stab_pack_sim(const double *d, const double *q, double *params, int n)
{
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= n) return;
    params[4 * (size_t)i] = q[2 * i]; params[4 * (size_t)i + 1] = q[2 * i + 1];
    params[4 * (size_t)i + 2] = d[2 * i]; params[4 * (size_t)i + 3] = d[2 * i + 1];
}

// grid and lanes as k_stab_warp.  params: [n][4]
template <typename Tin, typename Tout>
__global__ __launch_bounds__(256) void k_stab_warp_sim(const Tin *frames, int H, int W, const double *params, Tout *out)
{
    const int x = (int)(blockIdx.x * 256 + threadIdx.x);
    if (x >= W) return;
    const size_t px = (size_t)H * W;
    const StabFrame<Tin> F{frames + (size_t)blockIdx.z * px, W};
    const double *p = params + 4 * (size_t)blockIdx.z;
    const double cx = (double)(W - 1) * 0.5, cy = (double)(H - 1) * 0.5, m = 1.0 + p[0], p1 = p[1], tx = p[2], ty = p[3];
    const double u = (double)x - cx;
    Tout *o = out + (size_t)blockIdx.z * px;
    for (int y = (int)blockIdx.y; y < H; y += (int)gridDim.y) {
        const double v = (double)y - cy;
        o[(size_t)y * W + x] = mag_out<Tout>(stab_bilinear(F, H, W, stab_sim_fx(cx, u, v, m, p1, tx), stab_sim_fy(cy, u, v, m, p1, ty)));
    }
}

// the colour form: grid and lanes as k_stab_warp_bgr
__global__ __launch_bounds__(256) void k_stab_warp_sim_bgr(const uint8_t *frames, int H, int W, const double *params, uint8_t *out)
{
    const int e = (int)(blockIdx.x * 256 + threadIdx.x);
    if (e >= 3 * W) return;
    const int x = e / 3, ch = e - 3 * x;
    const size_t px = (size_t)H * W;
    const StabChannel F{frames + (size_t)blockIdx.z * px * 3 + ch, W};
    const double *p = params + 4 * (size_t)blockIdx.z;
    const double cx = (double)(W - 1) * 0.5, cy = (double)(H - 1) * 0.5, m = 1.0 + p[0], p1 = p[1], tx = p[2], ty = p[3];
    const double u = (double)x - cx;
    uint8_t *o = out + (size_t)blockIdx.z * px * 3;
    for (int y = (int)blockIdx.y; y < H; y += (int)gridDim.y) {
        const double v = (double)y - cy;
        o[(size_t)y * 3 * W + e] = mag_out<uint8_t>(stab_bilinear(F, H, W, stab_sim_fx(cx, u, v, m, p1, tx), stab_sim_fy(cy, u, v, m, p1, ty)));
    }
}

}  // namespace rm
