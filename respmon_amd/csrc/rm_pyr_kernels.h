// respmon_amd/csrc/rm_pyr_kernels.h -- cv2.pyrDown / cv2.pyrUp on whole [T, h, w] levels (pyramid.py:9-28, 51-69): the kernels of
// rm_pyramid.hip.  up_h / up_at are also the per-pixel arithmetic the LDS kernels of rm_small_kernels.h restate.
#pragma once
#include "rm_kernels.h"

namespace rm {

// ----------------------------------------------------------------------------------------
// K1  cv2.pyrDown (pyramid.py:14) on every frame: [T,h,w] Tin -> [T,dh,dw] f64
//     LDS-staged tile; horizontal 5-tap first, vertical second (OpenCV order).
// ----------------------------------------------------------------------------------------
constexpr int PD_TY = 8, PD_TX = 64;
constexpr int PD_SY = 2 * PD_TY + 3, PD_SX = 2 * PD_TX + 3;

// the tile body: 256 threads stage rows 2 ty0 - 2 .. and columns 2 tx0 - 2 .. of ONE image `sp` (h x w, reflected 101) in s_src, filter along
// x into s_row, then along y into the PD_TY x PD_TX outputs at (ty0, tx0) of `dp` (dh x dw).  A device function so that a kernel with
// another block-to-image mapping (rm_phase_motion_kernels.h: pixel block, frame, subject) runs this arithmetic and no copy of it.
template <typename Tin>
__device__ __forceinline__ void pyr_down_tile(const Tin *sp, int h, int w, double *dp, int dh, int dw, int ty0, int tx0,
                                              double (&s_src)[PD_SY][PD_SX + 1], double (&s_row)[PD_SY][PD_TX])
{
    const int tid = threadIdx.x;
    for (int i = tid; i < PD_SY * PD_SX; i += 256) {
        int r = i / PD_SX, c = i - r * PD_SX;
        int sy = reflect101(2 * ty0 - 2 + r, h), sx = reflect101(2 * tx0 - 2 + c, w);
        s_src[r][c] = load_px(sp, (size_t)sy * w + sx);
    }
    __syncthreads();
    for (int i = tid; i < PD_SY * PD_TX; i += 256) {
        int r = i / PD_TX, x = i - r * PD_TX;
        const double *s = &s_src[r][2 * x];
        s_row[r][x] = s[2] * 6 + (s[1] + s[3]) * 4 + s[0] + s[4];
    }
    __syncthreads();
    for (int i = tid; i < PD_TY * PD_TX; i += 256) {
        int y = i / PD_TX, x = i - y * PD_TX;
        int oy = ty0 + y, ox = tx0 + x;
        if (oy < dh && ox < dw) {
            int r = 2 * y;
            double v = (s_row[r + 2][x] * 6 + (s_row[r + 1][x] + s_row[r + 3][x]) * 4 + s_row[r][x] + s_row[r + 4][x]) *
                       (1.0 / 256);
            dp[(size_t)oy * dw + ox] = v;
        }
    }
}

template <typename Tin>
__global__ __launch_bounds__(256) void k_pyr_down(const Tin *src, int h, int w, size_t frame_stride,
                                                  double *dst, int dh, int dw)
{
    __shared__ double s_src[PD_SY][PD_SX + 1];
    __shared__ double s_row[PD_SY][PD_TX];
    const int t = blockIdx.z;
    pyr_down_tile(src + (size_t)t * frame_stride, h, w, dst + (size_t)t * dh * dw, dh, dw, blockIdx.y * PD_TY, blockIdx.x * PD_TX, s_src, s_row);
}

// ----------------------------------------------------------------------------------------
// K2  cv2.pyrUp with explicit dstsize (pyramid.py:25-26, 55), SURVEY B2.
//     `up_at` evaluates one output pixel from a source image addressed through a functor so the
//     same code serves global memory (materialising kernels) and LDS tiles (fused collapse).
// ----------------------------------------------------------------------------------------
// horizontal value of source row r at destination column x (unnormalised, x8 kernel)
template <typename Src>
__device__ __forceinline__ double up_h(const Src &s, int r, int x, int sw)
{
    if (sw == 1) return s(r, 0) * 8;
    int j = x >> 1;
    if (x & 1) {
        if (j == sw - 1) return s(r, j) * 8;
        return (s(r, j) + s(r, j + 1)) * 4;
    }
    if (j == 0) return s(r, 0) * 6 + s(r, 1) * 2;
    if (j == sw - 1) return s(r, j - 1) + s(r, j) * 7;
    return s(r, j - 1) + s(r, j) * 6 + s(r, j + 1);
}

template <typename Src>
__device__ __forceinline__ double up_at(const Src &s, int y, int x, int sh, int sw)
{
    int i = y >> 1;
    if (y & 1) {
        int r2 = (i == sh - 1) ? i : i + 1;
        return ((up_h(s, i, x, sw) + up_h(s, r2, x, sw)) * 4) * (1.0 / 64);
    }
    int r0 = (i == 0) ? (sh > 1 ? 1 : 0) : i - 1;
    int r2 = (i == sh - 1) ? i : i + 1;
    return (up_h(s, r0, x, sw) + up_h(s, i, x, sw) * 6 + up_h(s, r2, x, sw)) * (1.0 / 64);
}

struct GlobalImg {
    const double *p; int w;
    __device__ __forceinline__ double operator()(int r, int c) const { return p[(size_t)r * w + c]; }
};

// mode 0: dst = up(src); 1: dst = other - up(src); 2: dst = up(src) + other
// src_fs / dst_fs / other_fs: frame strides in doubles (frames of several levels may share one [T, NP] buffer)
RM_KERNEL __launch_bounds__(256) void k_pyr_up(const double *src, int sh, int sw, size_t src_fs, double *dst, int dh, int dw,
                                                size_t dst_fs, int mode, const double *other, size_t other_fs)
{
    int x = blockIdx.x * 64 + (threadIdx.x & 63);
    int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    int t = blockIdx.z;
    if (x >= dw || y >= dh) return;
    GlobalImg s{src + (size_t)t * src_fs, sw};
    double u = up_at(s, y, x, sh, sw);
    size_t o = (size_t)y * dw + x;
    if (mode == 1) u = other[(size_t)t * other_fs + o] - u;
    else if (mode == 2) u = u + other[(size_t)t * other_fs + o];
    dst[(size_t)t * dst_fs + o] = u;
}

// The same for large levels: a thread produces the 2 x 2 outputs that hang under source pixel (i, j).  Their taps all lie
// in its 3 x 3 neighbourhood, so the four up_at() calls share 9 loads (instead of 9 + 6 + 6 + 4 for four threads), the
// address arithmetic is paid once, and a lane stores 16 contiguous bytes per row.  Same expressions per output, same bits.
RM_KERNEL __launch_bounds__(256) void k_pyr_up_2x2(const double *__restrict__ src, int sh, int sw, size_t src_fs,
                                                    double *dst, int dh, int dw, size_t dst_fs, int mode,
                                                    const double *other, size_t other_fs)
{
    const int x = 2 * (blockIdx.x * 64 + (threadIdx.x & 63));
    const int y = 2 * (blockIdx.y * 4 + (threadIdx.x >> 6));
    const int t = blockIdx.z;
    if (x >= dw || y >= dh) return;
    const bool x1 = x + 1 < dw, y1 = y + 1 < dh;
    GlobalImg s{src + (size_t)t * src_fs, sw};
    double u00 = up_at(s, y, x, sh, sw);
    double u01 = x1 ? up_at(s, y, x + 1, sh, sw) : 0.0;
    double u10 = y1 ? up_at(s, y + 1, x, sh, sw) : 0.0;
    double u11 = (x1 && y1) ? up_at(s, y + 1, x + 1, sh, sw) : 0.0;
    const size_t o0 = (size_t)y * dw + x, o1 = o0 + dw;
    if (mode != 0) {
        const double *op = other + (size_t)t * other_fs;
        const double a00 = op[o0], a01 = x1 ? op[o0 + 1] : 0.0, a10 = y1 ? op[o1] : 0.0, a11 = (x1 && y1) ? op[o1 + 1] : 0.0;
        if (mode == 1) { u00 = a00 - u00; u01 = a01 - u01; u10 = a10 - u10; u11 = a11 - u11; }
        else { u00 = u00 + a00; u01 = u01 + a01; u10 = u10 + a10; u11 = u11 + a11; }
    }
    double *dp = dst + (size_t)t * dst_fs;
    dp[o0] = u00;
    if (x1) dp[o0 + 1] = u01;
    if (y1) { dp[o1] = u10; if (x1) dp[o1 + 1] = u11; }
}

}  // namespace rm
