// respmon_amd/csrc/rm_down_u16.hip -- the fused Gaussian chains for uint16 frame buffers (RM_U16, rm_down_u16.h): the all-register chain
// k_down_chain_u8<S, uint16_t> where the width allows it, the LDS front end k_down_chain<uint16_t, S> for every other shape
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_down_launch.h"
#include "rm_down_u16.h"

using namespace rm;

// frames[T,H,W] uint16 -> G_S[T,h_S,w_S] in one launch: launch_down_chain's decisions (rm_down.hip) for this dtype
int launch_down_chain_u16(rm_ctx *ctx, const void *frames, int T, const std::vector<int> &h, const std::vector<int> &w, int S, double *out,
                          hipStream_t s, bool tiny)
{
    const int V = dtype_vec(RM_U16);
    const bool vec_ok = (w[0] % V == 0) && (((size_t)h[0] * w[0] * dtype_size(RM_U16)) % 16 == 0) && (((uintptr_t)frames) % 16 == 0);
    if (S < 1 || S > 5) return fail(RM_E_UNSUPPORTED, "fused pyrDown chain supports 1..5 levels, got %d", S);
    DownGeom g8;
    // (segments per frame as for the float16 buffer, rm_down_narrow.hip: the same bytes and the same geometry)
    if (vec_ok && !ctx->dbg.dc_lds_front_end && make_down_geom_u8(S, h.data(), w.data(), T, g8, tiny, ctx->dbg.dc_segs, 2048)) {
        g8.prio = ctx->dbg.dc_prio;
        const size_t fs = (size_t)h[0] * w[0];
        const unsigned grid = (unsigned)(((T + 7) / 8) * 8 * g8.strips * g8.segs);
        const uint16_t *f = (const uint16_t *)frames;
        const size_t ring = narrow_ring_bytes<uint16_t>();
        switch (S) {
        case 1: hipLaunchKernelGGL((k_down_chain_u8<1, uint16_t>), dim3(grid), dim3(64), ring, s, f, fs, g8, out); break;
        case 2: hipLaunchKernelGGL((k_down_chain_u8<2, uint16_t>), dim3(grid), dim3(64), ring, s, f, fs, g8, out); break;
        case 3: hipLaunchKernelGGL((k_down_chain_u8<3, uint16_t>), dim3(grid), dim3(64), ring, s, f, fs, g8, out); break;
        default: hipLaunchKernelGGL((k_down_chain_u8<4, uint16_t>), dim3(grid), dim3(64), ring, s, f, fs, g8, out); break;
        }
        LAUNCH_CHECK();
        return RM_OK;
    }
    return launch_down_chain_t<uint16_t>(ctx, frames, T, h, w, S, vec_ok ? 1 : 0, out, s, tiny);
}
