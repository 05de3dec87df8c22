/*
 * include/respmon_hip_debug.h -- developer switches, test hooks and diagnostics of librespmon_hip.so.
 *
 * NOT part of the drop-in interface (include/respmon_hip.h): nothing a caller of the reference's path needs is declared here,
 * and a reference-side binding never includes this file.  tests/, bench.py's diagnostics legs and tools/ do.
 * Every switch selects between implementations with identical results, or shrinks a tuning constant so that a test reaches a
 * rare path; the library never reads the process environment.
 */
#ifndef RESPMON_HIP_DEBUG_H
#define RESPMON_HIP_DEBUG_H

#include "respmon_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rm_calibrate / rm_locate flags that exist for tests only */
#define RM_FLAG_TINY_STORE 4u     /* a value store of 8 slots, so that nearly every selection overflows into the store-less sum kernel */
#define RM_FLAG_TINY_STRIPS 8u    /* 3-column strips / 2-row segments in the fused pyrDown chain */
#define RM_FLAG_FF_PER_LEVEL 512u /* the filter-first small pyramid with one launch per level although it would fit LDS */

/* per-context switches; unknown key -> RM_E_BADARG.  The keys and their meaning: struct DebugKnobs in respmon_amd/csrc/rm_internal.h
 * ("temporal_valu" 0|1, "dc_segs" n, "dense_split" 0|1|2|4, "store_slots" n, "exchange_dense" 0|1, ...).
 * "exchange_dense" changes which collective a step issues: set it identically on EVERY rank of a communicator.
 * "flow_clip_bytes" n lowers the workspace cap of one chunk of rm_flow_clip and rm_flow_multi_clip (0: 256 MiB), so that a test splits
 * a small clip into several chunks: a chunk holds max(1, n / slot - 1) frames, slot = 5 bytes per pixel of every LK pyramid level of
 * the ROI -- for rm_flow_multi_clip the sum of that over the subjects that still have points.
 * "stream_frames" n: frames per internal chunk of rm_stream_push and rm_phase_push (0: by their workspace caps of 256 MiB / 2 GiB, at most 256), so that a test
 * reaches the split with a handful of frames.
 * "phase_motion_frames" n: frames per internal chunk of rm_phase_motion_clip and rm_phase_motion_multi_clip at most (0: by their 256 MiB
 * workspace cap), so that a test reaches the split -- and the alternation of the state's two planes -- with a handful of frames.
 * "stab_frames" n: frames per internal chunk of rm_stab_push and rm_stab_sim_push at most (0: by their 256 MiB workspace cap), so that a
 * test reaches the split with a handful of frames.
 * "rate_wide" 0|1: the K-split / the wave-per-16-columns form of the rate map's kernel whatever the level size (-1: by size). */
int rm_debug_set(rm_ctx *ctx, const char *key, long long value);

/* counters of the last rm_calibrate on this context: out_host[0] = (frame, tile) pairs, [1] = pairs evaluated at full resolution
 * by the selection's evaluation pass, [2] = pairs the selection kept for the masked sum, [3] = capacity of the value store (pairs);
 * 0 = the store-less sum kernel took the sum (it recomputes every pair itself, [1] then counts only the pairs evaluated for the
 * exact raw.min() / raw.max()) */
int rm_debug_counters(rm_ctx *ctx, long long *out_host, void *stream);

/* first 16 hex digits of the sha256 over the sources of the frame-buffer kernels this library was built from (csrc/Makefile
 * STAMP_SRCS, concatenated in that order).  The committed PMC figures (profiles/hbm_traffic.json, profiles/valu_issue.json) carry the
 * stamp of the library they were measured on; bench.py reports them only while the stamps agree. */
const char *rm_debug_kernel_source_stamp(void);

/* The frame-buffer kernel's hand-off of its segment boundary (float64 buffers, two segments per frame; DESIGN 4.1 "the stitch";
 * switches "dc_stitch" 0|1, "dc_stitch_count" 0|1, test hooks "dc_stitch_swap" 0|1 and "dc_stitch_stall_frame" f (-1: none)).
 * Fills out_host[0 .. RM_CHAIN_STITCH_WORDS) for the launch a float64 [T,H,W] buffer with 16-byte aligned rows and a chain of depth
 * S would get under the context's switches ("dc_segs", "dc_wpg", "dc_split", "dc_stitch"):
 *   [0] 1 = the launch hands over, [1] segments per frame, [2] first level-S row of the lower segment (0: not the two-segment
 *   geometry; no ranges then), [3] strips per frame,
 *   [4] / [5] (frame, strip) pairs that took the hand-off / marched on without it in the LAST float64 launch of this context
 *   (counted only under "dc_stitch_count" 1; read after the work queued on `stream`),
 *   [6] the per-frame override in force ("dc_stitch_stall_frame"; -1 none), [7] reserved,
 *   [8 + 6 k .. 8 + 6 k + 5], k = 0 .. S: inclusive row ranges at level k (0 = the input): rows the upper wave reads or computes
 *   itself (first, last), rows it takes from the hand-off (first, last; first > last: none), rows the lower wave reads or emits.
 * S = 0: the counters only.  ctx = NULL: a host-only query that needs no device -- the four switches are read from out_host[0 .. 3]
 * ("dc_segs", "dc_wpg", "dc_split", "dc_stitch") before it is filled, and no counters are reported. */
#define RM_CHAIN_STITCH_WORDS 64
int rm_debug_chain_stitch(rm_ctx *ctx, int S, int H, int W, int T, long long *out_host, void *stream);

/* a copy of the first `bytes` bytes of the context's workspace buffer `name` as the last call left it ("tile_lo", "tile_hi": the
 * [unique frame][tile] bounds of the selection; "cS": the collapsed band-passed level) -- tests check the bounds themselves with it */
int rm_debug_workspace(rm_ctx *ctx, const char *name, void *out_host, size_t bytes, void *stream);

/* the ring of an rm_window as it lies in memory: rows [row0, row0 + nrows) of NP doubles each (row r holds frame j of the stream with
 * j mod T == r), copied to out_host after the work queued on `stream` */
int rm_debug_window_rows(rm_ctx *ctx, const rm_window *win, int row0, int nrows, double *out_host, void *stream);

/* host timeline of the last rm_locate on this context, microseconds on the steady clock relative to the entry of that call:
 * out_host[0] = entry of the call minus the return of the PREVIOUS rm_locate (what the caller spent between two calls),
 * [1] = first kernel launch issued, [2] = every launch issued, [3] = device work seen complete, [4] = host contour stage done
 * (the call returns right after).  bench.py reports the medians as `host_timeline_us`. */
#define RM_HOST_MARKS 5
int rm_debug_host_timeline(rm_ctx *ctx, double *out_host);

/* how the host contour stage of the last ROI extraction on this context found its contour (base.py:568-575) */
#define RM_ROI_PATH_NONE 0          /* no extraction yet, or settled without the host stage */
#define RM_ROI_PATH_ONE_BLOB 1      /* the one-blob rule on the row records / packed rows */
#define RM_ROI_PATH_SCAN 2          /* every border followed on the host */
#define RM_ROI_PATH_LABELLED 3      /* device labelling: the borders that can win followed */
#define RM_ROI_PATH_AREA_BOUND 4    /* device labelling: the top component's area bound beat every rival's box, no border followed */
int rm_debug_roi_path(rm_ctx *ctx, int *path_out);

#ifdef __cplusplus
}
#endif
#endif /* RESPMON_HIP_DEBUG_H */
