// respmon_amd/csrc/rm_flow_clip.h -- extract_motion('flow') over a whole resident clip in one call (rm_flow_clip, rm_motion.hip):
//   frame-parallel front   crops (k_roi_to_u8_clip, rm_kernels.h), uint8 pyrDown levels and Scharr derivatives of all frames of a
//                          chunk, the grid over (pixel block, frame); the arithmetic is rm_flow.h's pyr_down_u8_px / scharr_px
//   point-parallel tracker one wavefront per point walks the chunk's frames in order (lk_track_point, the per-frame body of
//                          k_lk_track); its input for frame t is its own output for frame t - 1.  Waves never talk to each other.
//   frame-parallel finish  per frame the float32 mean of old - new over the live points in point order (flow_finish_wave, the body of
//                          k_flow_finish) and, for the clip's last frame, the survivors packed in point order
// Points keep their index through the whole clip (a lost point stays dead: the reference drops st == 0 points, base.py:377-382, and
// the mean of base.py:388 runs over the survivors in point order, packed or not), so nothing is compacted between frames or chunks.
#pragma once
#include "rm_flow.h"

namespace rm {

// images of a chunk lie `stride` bytes apart per level; blockIdx.y is the image
RM_KERNEL __launch_bounds__(256) void k_pyr_down_u8_clip(const uint8_t *src, size_t src_stride, int h, int w, uint8_t *dst, size_t dst_stride, int dh, int dw)
{
    pyr_down_u8_px(src + (size_t)blockIdx.y * src_stride, h, w, dst + (size_t)blockIdx.y * dst_stride, dh, dw, blockIdx.x * 256 + threadIdx.x);
}

RM_KERNEL __launch_bounds__(256) void k_scharr_clip(const uint8_t *src, size_t stride, int h, int w, short *d)
{
    scharr_px(src + (size_t)blockIdx.y * stride, h, w, d + 2 * (size_t)blockIdx.y * stride, blockIdx.x * 256 + threadIdx.x);
}

// One wavefront per point over the `nframes` frames of a chunk.  L describes image 0 (prev) and image 1 (next) of the chunk with the
// distance between consecutive images per level (L.stride): frame t tracks from image t to image t + 1.
// start / start_alive: the point's position and whether it still lives when the chunk begins; pos [nframes][npts][2] and
// status [nframes][npts]: what k_lk_track would have written frame after frame (status 0 for every frame behind the one that lost the
// point: its wave leaves); end / end_alive: what the next chunk starts from.
template <int ROUNDS>
__global__ __launch_bounds__(64) void k_lk_track_clip(LKLevels L, int nframes, const float *start, const uint8_t *start_alive, int npts, int win_w,
                                                      int win_h, int max_count, double epsilon, float *pos, uint8_t *status, float *end,
                                                      uint8_t *end_alive)
{
    __shared__ short s_I[LK_MAX_WIN];
    __shared__ short s_dI[2 * LK_MAX_WIN];
    __shared__ __attribute__((aligned(16))) float s_t0[LK_MAX_WIN], s_t1[LK_MAX_WIN], s_t2[LK_MAX_WIN];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= npts) return;
    float px = start[2 * p], py = start[2 * p + 1];
    int st = start_alive[p];
    int t = 0;
    if (st) {
        for (; t < nframes; ++t) {
            float ox, oy;
            lk_track_point<ROUNDS>(L, (size_t)t, px, py, win_w, win_h, max_count, epsilon, s_I, s_dI, s_t0, s_t1, s_t2, ox, oy, st);
            if (lane == 0) {
                pos[2 * ((size_t)t * npts + p)] = ox; pos[2 * ((size_t)t * npts + p) + 1] = oy;
                status[(size_t)t * npts + p] = (uint8_t)st;
            }
            px = ox; py = oy;
            if (!st) { ++t; break; }
        }
    }
    for (int u = t + lane; u < nframes; u += 64) status[(size_t)u * npts + p] = 0;
    if (lane == 0) { end[2 * p] = px; end[2 * p + 1] = py; end_alive[p] = (uint8_t)st; }
}

// frame t of the chunk: old = the positions frame t - 1 left (start for t == 0), new = pos[t]; res[4 t .. 4 t + 2] = {mean_x, mean_y,
// n_good}; next_pts (may be null): where the LAST frame's survivors are packed
RM_KERNEL __launch_bounds__(64) void k_flow_finish_clip(const float *start, const float *pos, const uint8_t *status, int npts, int nframes, float *res,
                                                        float *next_pts)
{
    HIP_DYNAMIC_SHARED(float, s_d)
    const int t = blockIdx.x;
    flow_finish_wave(t ? pos + 2 * (size_t)(t - 1) * npts : start, pos + 2 * (size_t)t * npts, status + (size_t)t * npts, npts, res + 4 * t,
                     t == nframes - 1 ? next_pts : nullptr, s_d);
}
// (more points than the staging holds: one thread per frame, global memory)
RM_KERNEL void k_flow_finish_clip_seq(const float *start, const float *pos, const uint8_t *status, int npts, int nframes, float *res, float *next_pts)
{
    const int t = blockIdx.x;
    flow_finish_seq(t ? pos + 2 * (size_t)(t - 1) * npts : start, pos + 2 * (size_t)t * npts, status + (size_t)t * npts, npts, res + 4 * t,
                    t == nframes - 1 ? next_pts : nullptr);
}

// rm_pca_reduce of every window of a motion list in one launch: workgroup b reduces rows max(0, j + 1 - window) .. j, j = first + b
RM_KERNEL __launch_bounds__(64) void k_pca_reduce_windows(const float *motion, int first, int window, double *out)
{
    const int j = first + blockIdx.x;
    const int lo = j + 1 - window > 0 ? j + 1 - window : 0, n = j + 1 - lo;
    if (n < 2) { if (threadIdx.x == 0) out[blockIdx.x] = 0.0; return; }   // base.py:406-407
    pca_reduce_wave(motion + 2 * (size_t)lo, n, out + blockIdx.x);
}

}  // namespace rm
