// respmon_amd/csrc/rm_down_launch.h -- launcher templates of k_down_chain (rm_down_chain.h), instantiated per frame dtype by
// rm_down_f64.hip (the reference's buffer dtype: the roofline kernel) and rm_down_generic.hip (narrow dtypes through its LDS front end)
#pragma once
#include "rm_internal.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------
// fused Gaussian chain (rm_down_chain.h)
// ------------------------------------------------------------------------------------------
template <typename Tin, bool VB>
static int launch_down_chain_g(const Tin *f, int T, const DownGeom &g, double *out, hipStream_t s)
{
    const size_t fs = (size_t)g.h[0] * g.w[0];
    (void)T;
    const unsigned grid = down_chain_grid(g), block = down_chain_block(g);
    if constexpr (std::is_same<Tin, double>::value && !VB) {
        if (g.stitch) {   // a launch that hands its segment boundary over: the kernel that holds that code
#define RM_DC_STITCH_CASE(SS)                                                                                  \
    case SS:                                                                                                   \
        hipLaunchKernelGGL((k_down_chain_stitch<SS>), dim3(grid), dim3(block),                                 \
                           (sizeof(double) * down_chain_lds_doubles<double, SS>() * g.wpg), s, f, fs, g, out); \
        break;
            switch (g.S) {
                RM_DC_STITCH_CASE(2) RM_DC_STITCH_CASE(3) RM_DC_STITCH_CASE(4)
            default: return fail(RM_E_UNSUPPORTED, "the segment hand-off exists for chains of depth 2..4, got %d", g.S);
            }
#undef RM_DC_STITCH_CASE
            LAUNCH_CHECK();
            return RM_OK;
        }
    }
#define RM_DC_CASE(SS)                                                                                        \
    case SS:                                                                                                   \
        hipLaunchKernelGGL((k_down_chain<Tin, SS, VB>), dim3(grid), dim3(block),                               \
                           (sizeof(double) * down_chain_lds_doubles<Tin, SS>() * g.wpg), s, f, fs, g, out);    \
        break;
    switch (g.S) {
        RM_DC_CASE(1) RM_DC_CASE(2) RM_DC_CASE(3) RM_DC_CASE(4) RM_DC_CASE(5)
    default: return fail(RM_E_UNSUPPORTED, "fused pyrDown chain supports 1..5 levels, got %d", g.S);
    }
#undef RM_DC_CASE
    LAUNCH_CHECK();
    return RM_OK;
}

// doubles of one (frame, strip) hand-off block of the float64 chain of depth S (DCLayout::hand_total)
static inline size_t down_chain_hand_doubles(int S)
{
    return S == 2 ? (size_t)DCLayout<2, StripWidth<2>::SW, 2>::hand_total() : S == 3 ? (size_t)DCLayout<3, StripWidth<3>::SW, 2>::hand_total()
         : S == 4 ? (size_t)DCLayout<4, StripWidth<4>::SW, 2>::hand_total() : 0;
}

// buffers, epoch and test hooks of a launch that hands its segment boundary over (g.stitch, rm_down_chain.h).  The flags carry the
// launch's epoch, so nothing is cleared between launches: a flag counts only when it holds THIS launch's value.  (The epoch is a
// launch argument: such a launch must not be captured into a graph and replayed.)
static int down_chain_stitch_setup(rm_ctx *ctx, DownGeom &g, hipStream_t s)
{
    const size_t pairs = (size_t)g.T * g.strips;
    RM_TRY(ws(ctx, "dc_handoff", pairs * down_chain_hand_doubles(g.S), &g.hand));
    RM_TRY(ws(ctx, "dc_handoff_flags", pairs * DC_FLAG_STRIDE, &g.hand_flag));
    const DevBuf &fb = ctx->bufs["dc_handoff_flags"];
    if (fb.p != ctx->dc_flags_seen || fb.cap != ctx->dc_flags_cap || ctx->dc_epoch == 0xffffffffu) {   // a fresh allocation holds anything: zero it once, start the epochs again
        HIP_TRY(hipMemsetAsync(fb.p, 0, fb.cap, s));
        ctx->dc_flags_seen = fb.p; ctx->dc_flags_cap = fb.cap; ctx->dc_epoch = 0;
    }
    g.stitch_epoch = ++ctx->dc_epoch;
    g.stitch_swap = ctx->dbg.dc_stitch_swap ? 1 : 0;
    g.stitch_stall = ctx->dbg.dc_stitch_stall_frame >= 0 ? ctx->dbg.dc_stitch_stall_frame + 1 : 0;
    return RM_OK;
}

// one launch over all level-S rows: the hot instantiation whenever every level has >= 3 rows
template <typename Tin>
static int launch_down_chain_t(rm_ctx *ctx, const void *frames, int T, const std::vector<int> &h, const std::vector<int> &w, int S, int vec_ok,
                               double *out, hipStream_t s, bool tiny)
{
    const Tin *f = (const Tin *)frames;
    DownGeom g;
    const int stitch = (std::is_same<Tin, double>::value && ctx->dbg.dc_stitch) ? 1 : 0;
    if (!make_down_geom(S, h.data(), w.data(), T, vec_ok, 0, h[S], g, tiny, ctx->dbg.dc_segs, ctx->dbg.dc_wpg, ctx->dbg.dc_split, stitch)) return fail(RM_E_UNSUPPORTED, "down chain geometry");
    g.prio = ctx->dbg.dc_prio;
    if (ctx->dbg.dc_prio_shift >= 1 && ctx->dbg.dc_prio_shift <= 12) g.prio_shift = ctx->dbg.dc_prio_shift;
    ctx->dc_counted = false;
    if (g.stitch) RM_TRY(down_chain_stitch_setup(ctx, g, s));
    else g.stitch_swap = 0;
    if (ctx->dbg.dc_stitch_count && std::is_same<Tin, double>::value) {
        // (frame, strip) pairs that injected / fell back, striped; zero for a launch that does not hand over (rm_debug_chain_stitch)
        unsigned *cnt = nullptr;
        RM_TRY(ws(ctx, "dc_handoff_count", (size_t)2 * DC_COUNT_STRIPES, &cnt));
        HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned) * 2 * DC_COUNT_STRIPES, s));
        if (g.stitch) g.hand_count = cnt;
        ctx->dc_counted = true;
    }
    if (down_chain_hot_ok(S, h.data())) return launch_down_chain_g<Tin, false>(f, T, g, out, s);
    return launch_down_chain_g<Tin, true>(f, T, g, out, s);
}
