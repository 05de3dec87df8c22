// respmon_amd/csrc/rm_phase_motion_kernels.h -- rm_phase_motion_*: the amplitude-weighted mean phase velocity of an ROI, the third
// motion signal of extract_motion (the rule, operation by operation: include/respmon_hip.h).  Everything is float64 and every
// operation rounds once (the library is built with -ffp-contract=off).
//
// A chunk of n frames and K subjects (a subject: rectangle, level l, its rm_phase_motion state) lives in ONE workspace array: subject
// k's Gaussian level j is [C][h_j][w_j] at element PmSubject::off[j] (C: the chunk capacity of the call), j = 0 .. l + 1.  Every kernel
// runs over (block, frame, subject); a block beyond the subject's own count leaves at once, whole.
//
//   * k_pm_crop<Tin>: G_0 = the float64 crop (load_px: the conversions of the pyramid entry points).
//   * k_pm_down: G_j = pyrDown(G_j-1), the tile body of k_pyr_down (rm_pyr_kernels.h pyr_down_tile) on the subject's own image: borders
//     reflect at the crop's edge.
//   * k_pm_level: I = G_l - pyrUp(G_l+1), up_at of k_pyr_up, written over G_l.
//   * k_pm_reduce: the hot kernel.  A workgroup of 256 owns a 64 x 4 tile of the level, a lane ONE pixel, and walks the n frames of
//     the chunk with the previous frame's I, R1, R2, A in registers (the frame before the chunk: the state's Ip plane, R1p / R2p / Ap
//     recomputed from it).  Per frame it loads I and its four neighbours one frame ahead of the arithmetic (the lanes of a wave are 64
//     consecutive x of one row: the centre load is coalesced, left / right come from the lines the wave has just fetched, up / down from
//     the lines of the neighbouring waves of the workgroup), forms wgt, wgt dc, wgt ds, reduces each over the wave on DPP
//     (wave_reduce, rm_kernels.h), over the four waves through LDS in wave order, and writes one partial per (frame, subject, tile).
//     It reads the state plane `parity` and writes the last frame's I to the other one: no workgroup reads what another writes.
//   * k_pm_finish: a lane per (frame, subject, sum) adds the subject's tiles in tile order.
// The tiling and both orders are functions of (lh, lw) alone: a sum does not depend on N, K, the chunking or the other subjects.
#pragma once
#include "rm_pyr_kernels.h"   // pyr_down_tile, up_at

namespace rm {

constexpr int PM_MAX_LEVEL = 8;
constexpr int PM_LEVELS = PM_MAX_LEVEL + 2;      // G_0 .. G_l+1
constexpr int PM_TW = 64, PM_TH = 4;             // the reduction tile: one wave per row

struct PmSubject {
    int x, y, level;
    int h[PM_LEVELS], w[PM_LEVELS];              // G_j: h[0] x w[0] is the rectangle
    unsigned long long off[PM_LEVELS];           // element offset of [C][h_j][w_j] in the chunk workspace
    int ntx, ntiles;                             // tiles of level l: ceil(lw / 64) x ceil(lh / 4)
    unsigned tile0;                              // the subject's first partial inside a frame's row of partials
    int first, parity;                           // at the call's first chunk: the state is fresh; the plane that holds Ip
    double *state;                               // [2][lh * lw]
};

template <typename Tin>
__global__ __launch_bounds__(256) void k_pm_crop(const Tin *frames, size_t frame_px, int W, const PmSubject *tab, double *wsp)
{
    const PmSubject &S = tab[blockIdx.z];
    const int w = S.w[0];
    const size_t px = (size_t)S.h[0] * w;
    const Tin *f = frames + (size_t)blockIdx.y * frame_px + (size_t)S.y * W + S.x;
    double *g = wsp + S.off[0] + (size_t)blockIdx.y * px;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < px; i += (size_t)gridDim.x * 256) {
        const size_t r = i / w, c = i - r * w;
        g[i] = load_px(f, r * W + c);
    }
}

// grid: (max tiles of G_j over the subjects, n, K)
__global__ __launch_bounds__(256) void k_pm_down(const PmSubject *tab, double *wsp, int j)
{
    __shared__ double s_src[PD_SY][PD_SX + 1];
    __shared__ double s_row[PD_SY][PD_TX];
    const PmSubject &S = tab[blockIdx.z];
    if (j > S.level + 1) return;
    const int h = S.h[j - 1], w = S.w[j - 1], dh = S.h[j], dw = S.w[j];
    const unsigned ntx = (unsigned)(dw + PD_TX - 1) / PD_TX, nty = (unsigned)(dh + PD_TY - 1) / PD_TY;
    if (blockIdx.x >= ntx * nty) return;
    const int ty0 = (int)(blockIdx.x / ntx) * PD_TY, tx0 = (int)(blockIdx.x % ntx) * PD_TX;
    const double *sp = wsp + S.off[j - 1] + (size_t)blockIdx.y * h * w;
    double *dp = wsp + S.off[j] + (size_t)blockIdx.y * dh * dw;
    pyr_down_tile(sp, h, w, dp, dh, dw, ty0, tx0, s_src, s_row);
}

// grid: (ceil(max level pixels / 256), n, K)
__global__ __launch_bounds__(256) void k_pm_level(const PmSubject *tab, double *wsp)
{
    const PmSubject &S = tab[blockIdx.z];
    const int l = S.level, h = S.h[l], w = S.w[l], sh = S.h[l + 1], sw = S.w[l + 1];
    const size_t px = (size_t)h * w;
    double *g = wsp + S.off[l] + (size_t)blockIdx.y * px;
    const GlobalImg up{wsp + S.off[l + 1] + (size_t)blockIdx.y * sh * sw, sw};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < px; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i - (size_t)y * w);
        g[i] = g[i] - up_at(up, y, x, sh, sw);
    }
}

struct PmPx { double c, l, r, u, d; };
__device__ __forceinline__ PmPx pm_load(const double *f, size_t ic, size_t il, size_t ir, size_t iu, size_t id)
{
    return PmPx{f[ic], f[il], f[ir], f[iu], f[id]};
}

// grid: (max tiles over the subjects, K), 256 threads.  n: frames of the chunk; chunk: its index in the call (the state plane
// alternates per chunk); part: [n][TT][3], TT the tiles of all subjects.
__global__ __launch_bounds__(256) void k_pm_reduce(const PmSubject *tab, const double *wsp, int n, int chunk, unsigned TT, double *part)
{
    __shared__ double red[2][PM_TH][3];
    const PmSubject &S = tab[blockIdx.y];
    if ((int)blockIdx.x >= S.ntiles) return;
    const int l = S.level, h = S.h[l], w = S.w[l];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int x = (int)(blockIdx.x % (unsigned)S.ntx) * PM_TW + lane, y = (int)(blockIdx.x / (unsigned)S.ntx) * PM_TH + wave;
    const bool in = x < w && y < h;
    const int xc = in ? x : 0, yc = in ? y : 0;       // a lane outside the level reads pixel (0, 0) and adds zeros
    const size_t fs = (size_t)h * w;
    const size_t ic = (size_t)yc * w + xc;
    const size_t il = (size_t)yc * w + reflect101(xc - 1, w), ir = (size_t)yc * w + reflect101(xc + 1, w);
    const size_t iu = (size_t)reflect101(yc - 1, h) * w + xc, id = (size_t)reflect101(yc + 1, h) * w + xc;
    const bool fresh = S.first && chunk == 0;
    const int par = (S.parity + chunk) & 1;

    double Ip = 0.0, R1p = 0.0, R2p = 0.0, Ap = 0.0;
    if (!fresh) {
        const PmPx v = pm_load(S.state + (size_t)par * fs, ic, il, ir, iu, id);
        Ip = v.c; R1p = 0.5 * (v.r - v.l); R2p = 0.5 * (v.d - v.u);
        Ap = sqrt((Ip * Ip + R1p * R1p) + R2p * R2p);
    }
    const double *f = wsp + S.off[l];
    PmPx nx = pm_load(f, ic, il, ir, iu, id);
    for (int t = 0; t < n; ++t) {
        const PmPx v = nx;
        if (t + 1 < n) nx = pm_load(f + (size_t)(t + 1) * fs, ic, il, ir, iu, id);   // one frame ahead of the arithmetic
        const double I = v.c;
        const double R1 = 0.5 * (v.r - v.l), R2 = 0.5 * (v.d - v.u);
        const double A = sqrt((I * I + R1 * R1) + R2 * R2);
        double sw = 0.0, sc = 0.0, ss = 0.0;
        if (in && !(fresh && t == 0)) {
            const double re = (I * Ip + R1 * R1p) + R2 * R2p;
            const double qx = Ip * R1 - I * R1p, qy = Ip * R2 - I * R2p;
            const double hyp = sqrt(qx * qx + qy * qy);
            const double d = atan2(hyp, re);
            const double dc = hyp > 0.0 ? d * (qx / hyp) : 0.0;
            const double ds = hyp > 0.0 ? d * (qy / hyp) : 0.0;
            const double wgt = A * Ap;
            sw = wgt; sc = wgt * dc; ss = wgt * ds;
        }
        Ip = I; R1p = R1; R2p = R2; Ap = A;
        const auto add = [](double o, double v2) { return o + v2; };
        sw = wave_reduce(sw, add); sc = wave_reduce(sc, add); ss = wave_reduce(ss, add);
        double(&r)[PM_TH][3] = red[t & 1];
        if (lane == 0) { r[wave][0] = sw; r[wave][1] = sc; r[wave][2] = ss; }
        __syncthreads();   // (one barrier per frame: the other half of `red` is next written behind the NEXT barrier)
        if (threadIdx.x < 3) {
            const int c = (int)threadIdx.x;
            part[((size_t)t * TT + S.tile0 + blockIdx.x) * 3 + c] = ((r[0][c] + r[1][c]) + r[2][c]) + r[3][c];
        }
    }
    if (in) S.state[(size_t)(par ^ 1) * fs + ic] = Ip;
}

// n * K * 3 lanes; res: [N][K][3] of the call, frame0 = the chunk's first frame
__global__ __launch_bounds__(64) void k_pm_finish(const PmSubject *tab, const double *part, int n, int K, unsigned TT, int frame0, double *res)
{
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= n * K * 3) return;
    const int c = i % 3, k = (i / 3) % K, t = i / (3 * K);
    const PmSubject &S = tab[k];
    const double *p = part + ((size_t)t * TT + S.tile0) * 3 + c;
    double s = p[0];
    for (int j = 1; j < S.ntiles; ++j) s += p[3 * (size_t)j];
    res[((size_t)(frame0 + t) * K + k) * 3 + c] = s;
}

}  // namespace rm
