// respmon_amd/csrc/rm_down_f64.hip -- k_down_chain<double, S>: the frame-buffer kernel of the reference's float64 calibration_buffer (base.py:119)
// (one translation unit of librespmon_hip.so; shared host-side declarations: rm_internal.h)
#include "rm_down_launch.h"

using namespace rm;

int launch_down_chain_f64(rm_ctx *ctx, const void *frames, int T, const std::vector<int> &h, const std::vector<int> &w, int S, int vec_ok, double *out,
                          hipStream_t s, bool tiny)
{
    return launch_down_chain_t<double>(ctx, frames, T, h, w, S, vec_ok, out, s, tiny);
}

// include/respmon_hip_debug.h: the geometry a float64 [T,H,W] buffer with 16-byte aligned rows would be launched with under the
// context's switches (the same make_down_geom call as launch_down_chain_t), and the counters of the last launch
extern "C" int rm_debug_chain_stitch(rm_ctx *ctx, int S, int H, int W, int T, long long *out, void *stream)
{
    if (!out) return fail(RM_E_BADARG, "rm_debug_chain_stitch: bad argument");
    DebugKnobs dbg;
    if (ctx) dbg = ctx->dbg;
    else { dbg.dc_segs = (int)out[0]; dbg.dc_wpg = (int)out[1]; dbg.dc_split = (int)out[2]; dbg.dc_stitch = (int)out[3]; }   // host-only query
    for (int i = 0; i < RM_CHAIN_STITCH_WORDS; ++i) out[i] = 0;
    out[6] = dbg.dc_stitch_stall_frame;
    if (ctx && ctx->dc_counted) {
        auto it = ctx->bufs.find("dc_handoff_count");
        if (it != ctx->bufs.end() && it->second.p) {
            unsigned host[2 * DC_COUNT_STRIPES];
            hipStream_t s = (hipStream_t)stream;
            HIP_TRY(hipSetDevice(ctx->device));
            HIP_TRY(hipMemcpyAsync(host, it->second.p, sizeof(host), hipMemcpyDeviceToHost, s));
            HIP_TRY(stream_wait(s));
            for (int i = 0; i < DC_COUNT_STRIPES; ++i) { out[4] += host[i]; out[5] += host[DC_COUNT_STRIPES + i]; }
        }
    }
    if (S == 0) return RM_OK;   // counters only
    if (S < 1 || S > 5 || H < 1 || W < 1 || T < 1) return fail(RM_E_BADARG, "rm_debug_chain_stitch: bad geometry");
    int h[MAX_CHAIN], w[MAX_CHAIN];
    h[0] = H; w[0] = W;
    for (int k = 1; k <= S; ++k) { h[k] = (h[k - 1] + 1) / 2; w[k] = (w[k - 1] + 1) / 2; }
    DownGeom g;
    if (!make_down_geom(S, h, w, T, (W % 2 == 0) ? 1 : 0, 0, h[S], g, false, dbg.dc_segs, dbg.dc_wpg, dbg.dc_split, dbg.dc_stitch ? 1 : 0))
        return fail(RM_E_UNSUPPORTED, "down chain geometry");
    out[0] = g.stitch; out[1] = g.segs; out[2] = g.seg_split; out[3] = g.strips;
    if (g.seg_split > 0) {
        DownRanges r;
        down_chain_ranges(g, r);
        for (int k = 0; k <= S; ++k) {
            long long *o = out + 8 + 6 * k;
            o[0] = r.up_first[k]; o[1] = r.up_last[k]; o[2] = r.inj_first[k]; o[3] = r.inj_last[k]; o[4] = r.lo_first[k]; o[5] = r.lo_last[k];
        }
    }
    return RM_OK;
}
