// respmon_amd/csrc/rm_flow_multi.h -- extract_motion('flow') over a whole resident clip in one call, for one subject or several
// (rm_flow_clip = the K == 1 entry, rm_flow_multi_clip, rm_pca_reduce_windows, rm_pca_reduce_windows_multi; rm_motion.hip):
//   frame-parallel front   crops, uint8 pyrDown levels and Scharr derivatives of all frames of a chunk; the grid is (pixel block,
//                          image of the chunk, subject), a workgroup beyond its subject's pixel or level count leaves at once
//   point-parallel tracker one wavefront per (subject, point) walks the chunk's frames in order (lk_track_point, the per-frame body
//                          of k_lk_track); its input for frame t is its own output for frame t - 1.  Waves never talk to each other,
//                          and the tracks of different subjects are as independent as the tracks of different points.
//   frame-parallel finish  one workgroup per (frame, subject): the float32 mean of old - new over the live points in point order
//                          (flow_finish_wave, the body of k_flow_finish) and, for the clip's last frame, the survivors packed in
//                          point order
// Points keep their index through the whole clip (a lost point stays dead: the reference drops st == 0 points, base.py:377-382, and
// the mean of base.py:388 runs over the survivors in point order, packed or not), so nothing is compacted between frames or chunks.
// Only kernels live here.  Their arithmetic is the shared __device__ bodies of rm_flow.h / rm_kernels.h as they stand
// (roi_to_u8_grid, pyr_down_u8_px, scharr_px, lk_track_point, flow_finish_wave, flow_finish_seq, pca_reduce_wave), which is why
// a subject's numbers equal rm_flow_step's on its own state bit for bit.
#pragma once
#include "rm_flow.h"

namespace rm {

// One row of the per-call subject table (device memory, uploaded with the per-point subject indices in one copy).  ROIs differ in
// size, so they differ in level count, image sizes and point count.  L is the subject's LKLevels as lk_track_point takes it: per
// level h, w, the distance between consecutive images of the chunk (stride), and the addresses of image 0 (prev), image 1 (next)
// and the derivatives of image 0 -- the pooled arenas' bases plus the subject's offsets, added by the host.
struct FlowSubject {
    int x, y, w, h;         // rectangle inside the frame
    int npts, pt0;          // points of the subject, index of its first one among all points of the call (a prefix sum)
    uint8_t *crop_dst;      // where the crop of the launch's first frame goes: image 1 of level 0, or -- a subject without points -- its state's crop
    float *next_pts;        // where the survivors of the clip's last frame are packed: the state's own "next points" buffer
    LKLevels L;             // L.n == 0: a subject without points (no pyramid, no tracking)
};

// crops of `gridDim.y` frames: blockIdx.z is the subject (row of tab), blockIdx.y the frame, crops lie L.stride[0] bytes apart
template <typename Tin>
__global__ __launch_bounds__(256) void k_flow_multi_crop(const Tin *frames, size_t frame_px, int W, const FlowSubject *__restrict__ tab)
{
    const FlowSubject &S = tab[blockIdx.z];
    if ((size_t)blockIdx.x * 256 >= (size_t)S.w * S.h) return;
    roi_to_u8_grid(frames + (size_t)blockIdx.y * frame_px, W, S.x, S.y, S.w, S.h, S.crop_dst + (size_t)blockIdx.y * ((size_t)S.w * S.h));
}

// level l of the pyramids of images 0 .. gridDim.y - 1 of every subject that has such a level
RM_KERNEL __launch_bounds__(256) void k_flow_multi_pyr_down(const FlowSubject *__restrict__ tab, int l)
{
    const FlowSubject &S = tab[blockIdx.z];
    if (l >= S.L.n || (size_t)blockIdx.x * 256 >= S.L.stride[l]) return;
    pyr_down_u8_px(S.L.prev[l - 1] + (size_t)blockIdx.y * S.L.stride[l - 1], S.L.h[l - 1], S.L.w[l - 1],
                   const_cast<uint8_t *>(S.L.prev[l]) + (size_t)blockIdx.y * S.L.stride[l], S.L.h[l], S.L.w[l], blockIdx.x * 256 + threadIdx.x);
}

// Scharr derivatives of level l of images 0 .. gridDim.y - 1
RM_KERNEL __launch_bounds__(256) void k_flow_multi_scharr(const FlowSubject *__restrict__ tab, int l)
{
    const FlowSubject &S = tab[blockIdx.z];
    if (l >= S.L.n || (size_t)blockIdx.x * 256 >= S.L.stride[l]) return;
    scharr_px(S.L.prev[l] + (size_t)blockIdx.y * S.L.stride[l], S.L.h[l], S.L.w[l],
              const_cast<short *>(S.L.deriv[l]) + 2 * (size_t)blockIdx.y * S.L.stride[l], blockIdx.x * 256 + threadIdx.x);
}

// the chunk's last image (index n) becomes image 0 of the next chunk: level 0 only, the pyramid is rebuilt with the others
RM_KERNEL __launch_bounds__(256) void k_flow_multi_carry(const FlowSubject *__restrict__ tab, int n)
{
    const FlowSubject &S = tab[blockIdx.y];
    const size_t px = S.L.stride[0];
    uint8_t *img0 = const_cast<uint8_t *>(S.L.prev[0]);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < px; i += (size_t)gridDim.x * 256) img0[i] = img0[(size_t)n * px + i];
}

// One wavefront per point over the `nframes` frames of a chunk: workgroup p (one wave) is global point p, subject pt_subject[p].
// The subject's LKLevels, read from its table row with wave-uniform loads, describes image 0 (prev) and image 1 (next) of the chunk
// with the distance between consecutive images per level (L.stride): frame t tracks from image t to image t + 1.
// start / start_alive [P]: the point's position and whether it still lives when the chunk begins; pos [nframes][P][2] and
// status [nframes][P]: what k_lk_track would have written frame after frame (status 0 for every frame behind the one that lost the
// point: its wave leaves); end / end_alive [P]: what the next chunk starts from.  All are indexed by the global point index, so
// subject k's rows lie at offset S.pt0.
template <int ROUNDS>
__global__ __launch_bounds__(64) void k_lk_track_multi_clip(const FlowSubject *__restrict__ tab, const int *__restrict__ pt_subject, int nframes,
                                                            const float *start, const uint8_t *start_alive, int npts_all, int win_w, int win_h,
                                                            int max_count, double epsilon, float *pos, uint8_t *status, float *end, uint8_t *end_alive)
{
    __shared__ short s_I[LK_MAX_WIN];
    __shared__ short s_dI[2 * LK_MAX_WIN];
    __shared__ __attribute__((aligned(16))) float s_t0[LK_MAX_WIN], s_t1[LK_MAX_WIN], s_t2[LK_MAX_WIN];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= npts_all) return;
    const LKLevels &L = tab[pt_subject[p]].L;
    float px = start[2 * p], py = start[2 * p + 1];
    int st = start_alive[p];
    int t = 0;
    if (st) {
        for (; t < nframes; ++t) {
            float ox, oy;
            lk_track_point<ROUNDS>(L, (size_t)t, px, py, win_w, win_h, max_count, epsilon, s_I, s_dI, s_t0, s_t1, s_t2, ox, oy, st);
            if (lane == 0) {
                pos[2 * ((size_t)t * npts_all + p)] = ox; pos[2 * ((size_t)t * npts_all + p) + 1] = oy;
                status[(size_t)t * npts_all + p] = (uint8_t)st;
            }
            px = ox; py = oy;
            if (!st) { ++t; break; }
        }
    }
    for (int u = t + lane; u < nframes; u += 64) status[(size_t)u * npts_all + p] = 0;
    if (lane == 0) { end[2 * p] = px; end[2 * p + 1] = py; end_alive[p] = (uint8_t)st; }
}

// frame t = blockIdx.x of the chunk, subject blockIdx.y, on the subject's slice of the point arrays: old = the positions frame
// t - 1 left (start for t == 0), new = pos[t]; res [nframes][nsub][4] = {mean_x, mean_y, n_good, -}.  pack: the chunk ends the
// clip, its last frame's survivors go to S.next_pts.  The two kernels share a grid; each leaves the subjects of the other kind
// alone (npts against FLOW_FINISH_MAX, as rm_flow_step decides: the second one walks global memory with one thread).
RM_KERNEL __launch_bounds__(64) void k_flow_finish_multi(const FlowSubject *__restrict__ tab, const float *start, const float *pos, const uint8_t *status,
                                                         int npts_all, int nframes, float *res, int pack)
{
    HIP_DYNAMIC_SHARED(float, s_d)   // sized by the host for the largest subject staged here
    const int t = blockIdx.x;
    const FlowSubject &S = tab[blockIdx.y];
    if (S.npts > FLOW_FINISH_MAX) return;
    const size_t p0 = (size_t)S.pt0;
    flow_finish_wave(t ? pos + 2 * ((size_t)(t - 1) * npts_all + p0) : start + 2 * p0, pos + 2 * ((size_t)t * npts_all + p0),
                     status + (size_t)t * npts_all + p0, S.npts, res + 4 * ((size_t)t * gridDim.y + blockIdx.y),
                     pack && t == nframes - 1 ? S.next_pts : nullptr, s_d);
}
RM_KERNEL void k_flow_finish_multi_seq(const FlowSubject *__restrict__ tab, const float *start, const float *pos, const uint8_t *status, int npts_all,
                                       int nframes, float *res, int pack)
{
    const int t = blockIdx.x;
    const FlowSubject &S = tab[blockIdx.y];
    if (S.npts <= FLOW_FINISH_MAX) return;
    const size_t p0 = (size_t)S.pt0;
    flow_finish_seq(t ? pos + 2 * ((size_t)(t - 1) * npts_all + p0) : start + 2 * p0, pos + 2 * ((size_t)t * npts_all + p0),
                    status + (size_t)t * npts_all + p0, S.npts, res + 4 * ((size_t)t * gridDim.y + blockIdx.y),
                    pack && t == nframes - 1 ? S.next_pts : nullptr);
}

// rm_pca_reduce of every window of several motion lists in one launch: output b belongs to the list whose first row is map[2 b]
// and is that list's row j = map[2 b + 1]; workgroup b reduces rows max(0, j + 1 - window) .. j of its own list
RM_KERNEL __launch_bounds__(64) void k_pca_reduce_windows_multi(const float *motion, const int *__restrict__ map, int window, double *out)
{
    const int row0 = map[2 * blockIdx.x], j = map[2 * blockIdx.x + 1];
    const int lo = j + 1 - window > 0 ? j + 1 - window : 0, n = j + 1 - lo;
    if (n < 2) { if (threadIdx.x == 0) out[blockIdx.x] = 0.0; return; }   // base.py:406-407
    pca_reduce_wave(motion + 2 * ((size_t)row0 + lo), n, out + blockIdx.x);
}

}  // namespace rm
