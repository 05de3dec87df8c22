// respmon_amd/csrc/rm_subjects.h -- several subjects per frame: the ROI means of K rectangles over a resident clip in one launch
// (rm_roi_mean_multi_clip).  The ranked contour list the rectangles usually come from (rm_heatmap_to_rois / rm_locate_multi) is a
// host stage: rm_contour.cpp ranked_external_contours_bits.
#pragma once
#include "rm_roi_kernels.h"

namespace rm {

// np.average(frame[y:y+h, x:x+w]) (base.py:357) for every (frame, rectangle) pair of a resident [N,H,W] clip.  Workgroup
// b = i * K + k reduces rectangle k of frame i with roi_mean_block -- k_roi_mean's summation order: 256 lanes striding the ROI, the
// xor-shuffle inside each wave, the four wave partials added in order -- so out[i * K + k] equals rm_roi_mean of that frame and
// rectangle bit for bit.  rois: K x {x, y, w, h} in device memory, checked against the frame by the host before the launch; the
// four values are wave-uniform loads.  The grid is flat over the pairs (N * K may pass a grid's y limit), a pair per workgroup:
// neither the launch count nor a loop inside a workgroup grows with N or K.
template <typename Tin>
__global__ __launch_bounds__(256) void k_roi_mean_multi_clip(const Tin *frames, size_t frame_px, int W, const int *rois, int K, double *out)
{
    __shared__ double s_part[4];
    const unsigned int b = blockIdx.x;
    const unsigned int i = b / (unsigned int)K, k = b - i * (unsigned int)K;
    const int *r = rois + 4 * (size_t)k;
    roi_mean_block(frames + (size_t)i * frame_px, W, r[0], r[1], r[2], r[3], out + b, s_part);
}

}  // namespace rm
