// respmon_amd/csrc/rm_roi_kernels.h -- frame dtype conversions (rm_ctx.hip), the time average of a clip (rm_temporal.hip), ROI mean and
// ROI crop (rm_motion.hip).
#pragma once
#include "rm_kernels.h"

namespace rm {

// np.average(video, axis=0) of a [T, npix] array of any frame dtype (base.py:562, 579, 587, 589): float64 sum in t
// order, then / T -- the order numpy's pairwise-free axis-0 reduction uses.
template <typename Tin>
__global__ __launch_bounds__(256) void k_time_average(const Tin *v, int T, size_t npix, double *out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    double acc = 0.0;
    for (int t = 0; t < T; ++t) acc = acc + load_px(v, (size_t)t * npix + p);
    out[p] = acc / (double)T;
}

// ----------------------------------------------------------------------------------------
// dtype helpers and ROI reductions
// ----------------------------------------------------------------------------------------
RM_KERNEL __launch_bounds__(256) void k_u8_to_f64(const uint8_t *src, double *dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        dst[i] = (double)src[i] * (1.0 / 255);
}

RM_KERNEL __launch_bounds__(256) void k_f64_to_u8(const double *src, uint8_t *dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        dst[i] = f64_to_u8_trunc(src[i] * 255);
}

// the 16-bit pair (RM_U16, include/respmon_hip.h): k * (1./65535), and the C truncation of v * 65535
RM_KERNEL __launch_bounds__(256) void k_u16_to_f64(const uint16_t *src, double *dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        dst[i] = load_px(src, i);
}

RM_KERNEL __launch_bounds__(256) void k_f64_to_u16(const double *src, uint16_t *dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        dst[i] = f64_to_u16_trunc(src[i] * 65535);
}

// np.average(frame[y:y+h, x:x+w]) (base.py:357): numpy's pairwise order is not reproduced; any
// float64 order is within ~1e-13 relative of it.  One block; wave partials summed in lane order.
template <typename Tin>
__device__ __forceinline__ void roi_mean_block(const Tin *frame, int W, int x, int y, int w, int h, double *out, double *s_part)
{
    double acc = 0.0;
    int n = w * h;
    for (int i = threadIdx.x; i < n; i += 256) {
        int r = i / w, c = i - r * w;
        acc = acc + load_px(frame, (size_t)(y + r) * W + x + c);
    }
    for (int m = 32; m >= 1; m >>= 1) acc = acc + __shfl_xor(acc, m);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]) / (double)n;
}

template <typename Tin>
__global__ __launch_bounds__(256) void k_roi_mean(const Tin *frame, int W, int x, int y, int w, int h, double *out)
{
    __shared__ double s_part[4];
    roi_mean_block(frame, W, x, y, w, h, out, s_part);
}

// the same reduction for every frame of a resident [N,H,W] clip: workgroup i sums frame i in k_roi_mean's order (rm_roi_mean_clip)
template <typename Tin>
__global__ __launch_bounds__(256) void k_roi_mean_clip(const Tin *frames, size_t frame_px, int W, int x, int y, int w, int h, double *out)
{
    __shared__ double s_part[4];
    roi_mean_block(frames + (size_t)blockIdx.x * frame_px, W, x, y, w, h, out + blockIdx.x, s_part);
}

template <typename Tin>
__device__ __forceinline__ void roi_to_u8_grid(const Tin *frame, int W, int x, int y, int w, int h, uint8_t *dst)
{
    int n = w * h;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        int r = i / w, c = i - r * w;
        dst[i] = f64_to_u8_trunc(load_px(frame, (size_t)(y + r) * W + x + c) * 255);
    }
}

template <typename Tin>
__global__ __launch_bounds__(256) void k_roi_to_u8(const Tin *frame, int W, int x, int y, int w, int h, uint8_t *dst)
{
    roi_to_u8_grid(frame, W, x, y, w, h, dst);
}

// cv2.cvtColor(BGR2GRAY), base.py:230: Y = (B*1868 + G*9617 + R*4899 + 8192) >> 14
RM_KERNEL __launch_bounds__(256) void k_bgr_to_gray(const uint8_t *bgr, size_t npix, uint8_t *gray)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        int b = bgr[3 * i], g = bgr[3 * i + 1], r = bgr[3 * i + 2];
        gray[i] = (uint8_t)((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14);
    }
}

// four pixels (three words) per thread and trip -> one word of gray; `nquads` = npix / 4, both pointers 4-byte aligned
RM_KERNEL __launch_bounds__(256) void k_bgr_to_gray_quads(const unsigned *bgr, size_t nquads, unsigned *gray)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nquads; i += (size_t)gridDim.x * 256) {
        const unsigned d0 = bgr[3 * i], d1 = bgr[3 * i + 1], d2 = bgr[3 * i + 2];
        const unsigned g0 = bgr_gray_x8<0>(d0, d1), g1 = bgr_gray_x8<3>(d0, d1), g2 = bgr_gray_x8<2>(d1, d2), g3 = bgr_gray_x8<1>(d2, d2);
        gray[i] = (g0 >> 3) | (g1 << 5) | (g2 << 13) | (g3 << 21);
    }
}

}  // namespace rm
