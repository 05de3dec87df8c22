// respmon_amd/csrc/rm_tile_eval.h -- TileEval, the wave-private evaluator of a 64 x 16 tile of raw[t], and the collapse kernels built on it
//
//   raw[t] = pyrUp^S(C_S[t])                        (pyramid.py:51-57 below `skip`: transforms.py:150-160 leaves those levels zero)
//   heat   = (1 / T) sum_t (raw[t] >= top ? min : raw[t])      (transforms.py:184-192, base.py:562), sequentially in t
//
// The generic evaluation of a kept (tile, frame) pair (rm_select_kernels.h k_eval_pairs: a single-wave workgroup runs the pyrUp chain in LDS)
// costs ~2 800 instructions per pair and 20+ us of latency; with the value store behind it (8 KB per pair) and k_masked_sum_tiles that
// was 28 + 21 us per step at 1080p x 256 for 2 600 pairs, 21 MB written and read back.  Here:
//   * TileEval<S> (TileFoot / TileSetup / tile_setup / te_step / tile_eval / tile_eval_below): ONE wave evaluates a 64 x 16 tile of
//     a frame from the tile's level-S footprint with everything frame-invariant settled before the frame loop, as rm_dense_sum.h's
//     DenseW does for S <= 2: the footprint of the tile at level k is the fixed VIRTUAL rectangle rows (16 ty >> k) - 1 .. by
//     columns (64 tx >> k) - 1 .. (10 x 34, 7 x 19, 5 x 11, 4 x 7 at k = 1 .. 4); virtual rows outside the image are materialised as
//     the rows OpenCV's border rules substitute (row -1 := row 1 falls out of the arithmetic, rows past the bottom repeat the last
//     one), columns outside the image only ever meet a zero weight; lane = destination column, the horizontal values of a step stay
//     in registers and the row structure (which rows are even, which three values meet) is compile time. ~300 instructions per
//     (tile, frame) instead of ~2 800. Same expressions per value as up_at() / chain_step() / level0_rows() (commuted additions and
//     merged power-of-two scalings at most): bit-identical to the generic chain.
//   * k_eval_c<S>: the exact raw.min() / raw.max() from the C pairs alone (k_select_pairs' list_a), one wave per pair.
//   * k_eval_pairs_fast<S>: k_eval_pairs' job with TileEval -- extrema from every listed pair, the kept pairs' values parked in the
//     value store for k_masked_sum_tiles.
//   * k_dense_sum_t<S>: the masked time sum without a value store, one wave per tile, frame after frame: the tile's kept frames
//     evaluated in TIME order and added, with the pruned frames' `min` in between, to sixteen running sums per lane.  Same values,
//     same order of additions as k_masked_sum_tiles / k_dense_sum: bit-identical.  Nothing but C_S is read, nothing but the heatmap
//     written.
// rm_magnify.h (k_magnify) and rm_bounds_l1.h (k_bounds_up1) use TileEval too.
#pragma once
#include "rm_dense_sum.h"

namespace rm {

// geometry of the virtual footprints
template <int S> struct TileFoot {
    static_assert(S >= 1 && S <= 4, "TileEval covers skip_levels_at_top 1 .. 4");
    static constexpr int nc(int k) { return k == 1 ? 34 : k == 2 ? 19 : k == 3 ? 11 : 7; }
    // rows of level k the evaluation holds in its buffer
    static constexpr int nr(int k) { return k == 1 ? 10 : k == 2 ? 7 : k == 3 ? 5 : 4; }
    static constexpr int size(int k) { return nr(k) * nc(k); }
    static constexpr int off(int k) { int o = 0; for (int i = 1; i < k; ++i) o += size(i); return o; }   // level 1 first
    static constexpr int TOTAL = off(S) + size(S);    // doubles of LDS per wave
    static constexpr int NST = size(S);               // staged elements
    static constexpr int PF = (NST + 63) / 64;        // ... per lane
    static constexpr int NV = 16;                     // level-0 values per lane
};

inline bool tile_eval_ok(const ChainGeom &g)
{
    if (g.S < 1 || g.S > 4) return false;
    for (int k = 1; k <= g.S; ++k) if (g.h[k] < 2 || g.w[k] < 2) return false;
    return true;
}

// everything about a tile that does not depend on the frame
template <int S> struct TileSetup {
    using F = TileFoot<S>;
    int off_g[F::PF];             // staged element lane + 64 p: offset inside a frame of C_S (virtual rows / columns resolved)
    int ha[S + 1], hb[S + 1], hc[S + 1];   // step k -> k - 1 (k = 2 .. S), lane < nc(k - 1): element offsets of the three column taps in a source row
    double wa[S + 1], wb[S + 1], wc[S + 1];
    int lastrow[S + 1];           // level k (k = 1 .. S - 1): last buffer row that lies inside the image; later rows repeat it
    double we_a, we_b, we_c, wo_b, wo_c;   // level 1 -> 0, this lane's column pair
    int l0off;                    // ... its taps of source row k: slice[l0off + k * nc(1) + {0, 1, 2}]
    int X, Y0;                    // ... its pixels: columns X, X + 1, rows Y0 .. Y0 + NV / 2 - 1
};

template <int S>
__device__ __forceinline__ void tile_setup(const ChainGeom &g, int tx, int ty, int lane, TileSetup<S> &ts)
{
    using F = TileFoot<S>;
    const int hS = g.h[S], wS = g.w[S];
    {   // staging: virtual rows / columns of the level-S footprint resolved to addresses
        const int fy = ((16 * ty) >> S) - 1, fx = ((64 * tx) >> S) - 1;
#pragma unroll
        for (int p = 0; p < F::PF; ++p) {
            const int i = min(lane + 64 * p, F::NST - 1);
            const int r = i / F::nc(S), c = i - r * F::nc(S);
            const int yv = fy + r, xv = fx + c;
            const int ya = yv < 0 ? 1 : (yv > hS - 1 ? hS - 1 : yv), xa = min(max(xv, 0), wS - 1);
            ts.off_g[p] = ya * wS + xa;
        }
    }
#pragma unroll
    for (int k = 2; k <= S; ++k) {
        // lane c owns destination column xv of level k - 1; its taps j - 1, j, j + 1 of level k (make_htap's five shapes)
        const int fxd = ((64 * tx) >> (k - 1)) - 1, fxs = ((64 * tx) >> k) - 1;
        const int xv = fxd + lane;
        const int sw = g.w[k], dw = g.w[k - 1];
        ts.ha[k] = ts.hb[k] = ts.hc[k] = 0; ts.wa[k] = ts.wb[k] = ts.wc[k] = 0.0;   // (outside the image / beyond the footprint: a finite value nobody reads with a non-zero weight)
        if (lane < F::nc(k - 1) && xv >= 0 && xv < dw) {
            const HTap t = make_htap(xv, sw);
            ts.ha[k] = t.ia - fxs; ts.hb[k] = t.ib - fxs; ts.hc[k] = t.ic - fxs;
            ts.wa[k] = t.wa; ts.wb[k] = t.wb; ts.wc[k] = t.wc;
        }
    }
#pragma unroll
    for (int k = 1; k < S; ++k) ts.lastrow[k] = (g.h[k] - 1) - (((16 * ty) >> k) - 1);
    // level 1 -> 0: lane = (column pair cp, row group rg): columns X, X + 1, rows 16 ty + 8 rg .. + 7
    const int cp = lane & 31, rg = lane >> 5;
    const int sw1 = g.w[1];
    ts.X = 64 * tx + 2 * cp;
    ts.Y0 = 16 * ty + 8 * rg;
    {
        const int j = ts.X >> 1;
        const bool left = j == 0, right = j >= sw1 - 1;
        ts.we_a = left ? 0.0 : 1.0; ts.we_b = right ? 7.0 : 6.0; ts.we_c = left ? 2.0 : (right ? 0.0 : 1.0);
        ts.wo_b = right ? 8.0 : 4.0; ts.wo_c = right ? 0.0 : 4.0;
    }
    // source rows (Y0 >> 1) - 1 .. of level 1; the buffer's first row is virtual row 8 ty - 1
    ts.l0off = F::off(1) + 4 * rg * F::nc(1) + cp;
}

// one pyrUp step inside the wave's slice, level K -> K - 1 (K >= 2)
// lmin (nullable): running minimum of the destination values this lane forms (lanes beyond the footprint leave it alone)
template <int S, int K>
__device__ __forceinline__ void te_step(const TileSetup<S> &ts, double *sl, int lane, double *lmin = nullptr)
{
    using F = TileFoot<S>;
    constexpr int NRS = F::nr(K), PS = F::nc(K), NRD = F::nr(K - 1), PD = F::nc(K - 1);
    static_assert(((NRD - 1) >> 1) + ((NRD - 1) & 1 ? 2 : 1) <= NRS - 1, "source rows of the last destination row");
    const double *src = sl + F::off(K);
    double *dst = sl + F::off(K - 1);
    const int oa = ts.ha[K], ob = ts.hb[K], oc = ts.hc[K];
    const double wa = ts.wa[K], wb = ts.wb[K], wc = ts.wc[K];
    double hq[NRS];
#pragma unroll
    for (int q = 0; q < NRS; ++q) hq[q] = dw_tap3(src[q * PS + oa], src[q * PS + ob], src[q * PS + oc], wa, wb, wc);
    // buffer row p of level K - 1 <-> an odd virtual row for even p (the values of rows q, q + 1 of level K), an even one for odd p
    // (rows q, q + 1, q + 2): up_at() with the exact power-of-two scalings merged
    const int last = ts.lastrow[K - 1];
    if (last >= NRD - 1) {   // (uniform) every buffer row lies inside the image: the common case, no selects
#pragma unroll
        for (int p = 0; p < NRD; ++p) {
            const int q = p >> 1;
            const double v = (p & 1) ? (hq[q] + hq[q + 1] * 6 + hq[q + 2]) * (1.0 / 64) : (hq[q] + hq[q + 1]) * (1.0 / 16);
            if (lane < PD) dst[p * PD + lane] = v;
            if (lmin && lane < PD) *lmin = (v < *lmin) ? v : *lmin;
        }
        return;
    }
    double prev = 0.0;
#pragma unroll
    for (int p = 0; p < NRD; ++p) {
        const int q = p >> 1;
        double v = (p & 1) ? (hq[q] + hq[q + 1] * 6 + hq[q + 2]) * (1.0 / 64) : (hq[q] + hq[q + 1]) * (1.0 / 16);
        if (p > last) v = prev;   // (uniform) virtual row past the bottom of the image: the last row again (up_at()'s r2)
        prev = v;
        if (lane < PD) dst[p * PD + lane] = v;
        if (lmin && lane < PD) *lmin = (v < *lmin) ? v : *lmin;
    }
}

// lmin1 (nullable): the step that forms level 1 tracks this lane's minimum of it
template <int S, int K> struct TeChain {
    static __device__ __forceinline__ void run(const TileSetup<S> &ts, double *sl, int lane, double *lmin1 = nullptr)
    {
        te_step<S, K>(ts, sl, lane, K == 2 ? lmin1 : nullptr);
        wave_sync();
        TeChain<S, K - 1>::run(ts, sl, lane, lmin1);
    }
};
template <int S> struct TeChain<S, 1> {
    static __device__ __forceinline__ void run(const TileSetup<S> &, double *, int, double * = nullptr) {}
};

// the staged level S of the frame is in the slice (and visible): run the chain; out[8 o + r] =
// raw[t, Y0 + r, X + o]
// the last step, level 1 (in the slice) -> level 0 (registers)
template <int S>
__device__ __forceinline__ void tile_eval_level0(const TileSetup<S> &ts, double *sl, double (&out)[TileFoot<S>::NV]);

// tile_eval() that may stop at level 1: every level-0 value is a convex combination of the tile's level-1 footprint (pyrUp's weights
// are positive and sum to one), so when the minimum of that footprint clears `top` by the pruning margin every pixel of the tile is
// masked and the last step need not run.  Returns false in that case (wave-uniform; `out` is not written).  The convexity bound of level 1 is far tighter than the level-S footprint bound the selection works with: on a frame
// of sensor noise (1080p, skip 4) 16 % of the pairs pass it against 39 %, at 4K skip 2 27 % against 98 %.
template <int S>
__device__ __forceinline__ bool tile_eval_below(const TileSetup<S> &ts, double *sl, int lane, double top_plus_margin, double (&out)[TileFoot<S>::NV])
{
    static_assert(S >= 2, "level 1 is staged, not computed, at skip 1");
    double lmin1 = __builtin_huge_val();
    TeChain<S, S>::run(ts, sl, lane, &lmin1);
    if (wave_min(lmin1) >= top_plus_margin) return false;
    tile_eval_level0<S>(ts, sl, out);
    return true;
}

template <int S>
__device__ __forceinline__ void tile_eval(const TileSetup<S> &ts, double *sl, int lane, double (&out)[TileFoot<S>::NV])
{
    TeChain<S, S>::run(ts, sl, lane);
    tile_eval_level0<S>(ts, sl, out);
}

template <int S>
__device__ __forceinline__ void tile_eval_level0(const TileSetup<S> &ts, double *sl, double (&out)[TileFoot<S>::NV])
{
    using F = TileFoot<S>;
    constexpr int P1 = F::nc(1), NM = F::NV / 4, NK = NM + 2;   // NM source rows own an (even, odd) output row pair
    const double *l0src = sl + ts.l0off;
    double hve[NK], hvo[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const double *row = l0src + k * P1;
        const double a = row[0], b = row[1], c = row[2];
        hve[k] = dw_tap3(a, b, c, ts.we_a, ts.we_b, ts.we_c);
        hvo[k] = __builtin_fma(c, ts.wo_c, b * ts.wo_b);   // b * 4 + c * 4 (or b * 8 + c * 0): both products exact
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        out[2 * m] = (hve[m] + hve[m + 1] * 6 + hve[m + 2]) * (1.0 / 64);
        out[2 * m + 1] = (hve[m + 1] + hve[m + 2]) * (1.0 / 16);
        out[F::NV / 2 + 2 * m] = (hvo[m] + hvo[m + 1] * 6 + hvo[m + 2]) * (1.0 / 64);
        out[F::NV / 2 + 2 * m + 1] = (hvo[m + 1] + hvo[m + 2]) * (1.0 / 16);
    }
}

// ---- exact raw.min() / raw.max() (transforms.py:185, 187) from the C pairs: one wave per listed pair -------------------------------
template <int S>
__global__ __launch_bounds__(64) void k_eval_c(const double *cS, ChainGeom g, int ntiles, const unsigned int *list_a, CollapseState *st)
{
    RM_TRACE_SCOPE(5);
    using F = TileFoot<S>;
    HIP_DYNAMIC_SHARED(double, lds)
    const int lane = threadIdx.x;
    // the first list entry is requested together with the list length (the list buffer is valid memory whatever it turns out to be)
    const unsigned first_idx = list_a[blockIdx.x];
    const unsigned nA = st->n_list_a;
    const double inf = __builtin_huge_val();
    const size_t fs = (size_t)g.h[S] * g.w[S];
    const int H0 = g.h[0], W0 = g.w[0];
    double mn = inf, mx = -inf;
    for (unsigned c = blockIdx.x; c < nA; c += gridDim.x) {
        const unsigned idx = (unsigned)uniform((int)(c == blockIdx.x ? first_idx : list_a[c]));
        const int u = idx / ntiles, tile = idx - u * ntiles;
        const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
        TileSetup<S> ts;
        tile_setup<S>(g, tx, ty, lane, ts);
        const double *src = cS + (size_t)u * fs;
        double stg[F::PF];
#pragma unroll
        for (int p = 0; p < F::PF; ++p) stg[p] = src[ts.off_g[p]];
        wave_sync();   // the previous pair's reads of the slice are behind us
#pragma unroll
        for (int p = 0; p < F::PF; ++p) if (lane + 64 * p < F::NST) lds[F::off(S) + lane + 64 * p] = stg[p];
        wave_sync();
        double v[16];
        tile_eval<S>(ts, lds, lane, v);
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (ts.Y0 + r < H0 && ts.X + o < W0) { const double x = v[8 * o + r]; mn = (x < mn) ? x : mn; mx = (x > mx) ? x : mx; }
    }
    mn = wave_min(mn); mx = wave_max(mx);
    if (lane == 0 && blockIdx.x < nA) {
        const unsigned long long kmn = f64_key(mn), kmx = f64_key(mx);
        const int sp_ = blockIdx.x & (NSTRIPE - 1);
        striped_min_max(st->min_keys, st->max_keys, sp_, kmn, kmx);
    }
}

// ---- the flat evaluation pass of the sparse path with the wave-private evaluator (k_eval_pairs' job, rm_select_kernels.h) ---------------------
// One wave per listed pair, every SIMD of the chip busy whatever tile the pairs belong to: exact min / max from all evaluated pairs,
// the values of the kept ones parked in their slot of the value store ([slot][row][column], 16 bytes per lane and row) for
// k_masked_sum_tiles.  ~500 instructions per pair instead of ~2 800.
template <int S>
__global__ __launch_bounds__(64) void k_eval_pairs_fast(const double *cS, ChainGeom g, int ntiles, const unsigned int *list_a, const unsigned int *list_b,
                                                        int *slot_of, CollapseState *st, double *store, SumPlan sp, int Th)
{
    RM_TRACE_SCOPE(5);
    using F = TileFoot<S>;
    HIP_DYNAMIC_SHARED(double, lds)
    const int lane = threadIdx.x;
    const unsigned first_idx = list_a[blockIdx.x];
    const unsigned nA = st->n_list_a, nB = st->n_list_b;
    const bool dense = sum_is_dense(st, sp);
    const unsigned n = nA + (dense ? 0u : nB);
    const double inf = __builtin_huge_val();
    const double top_ub = st->top_ub;   // upper bound of `top` from the tile bounds (k_select_pairs)
    const size_t fs = (size_t)g.h[S] * g.w[S];
    const int H0 = g.h[0], W0 = g.w[0];
    double mn = inf, mx = -inf;
    for (unsigned c = blockIdx.x; c < n; c += gridDim.x) {
        RM_TRACE_MARK(5, 0);
        const unsigned raw_idx = c < nA ? (c == blockIdx.x ? first_idx : list_a[c]) : list_b[c - nA];
        const unsigned idx = (unsigned)uniform((int)raw_idx);
        const int u = idx / ntiles, tile = idx - u * ntiles;
        const int slot = dense ? SLOT_PRUNED : uniform(slot_of[slot_index(u, tile, Th)]);   // (needed after the chain: requested now)
        const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
        RM_TRACE_MARK(5, 1);
        TileSetup<S> ts;
        tile_setup<S>(g, tx, ty, lane, ts);
        const double *src = cS + (size_t)u * fs;
        double stg[F::PF];
#pragma unroll
        for (int p = 0; p < F::PF; ++p) stg[p] = src[ts.off_g[p]];
        RM_TRACE_MARK(5, 2);
        wave_sync();   // the previous pair's reads of the slice are behind us
#pragma unroll
        for (int p = 0; p < F::PF; ++p) if (lane + 64 * p < F::NST) lds[F::off(S) + lane + 64 * p] = stg[p];
        wave_sync();
        RM_TRACE_MARK(5, 3);
        double v[16];
        tile_eval<S>(ts, lds, lane, v);
        RM_TRACE_MARK(5, 4);
        double pmn = inf;   // minimum of this pair's tile
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (ts.Y0 + r < H0 && ts.X + o < W0) { const double x = v[8 * o + r]; pmn = (x < pmn) ? x : pmn; mx = (x > mx) ? x : mx; }
        mn = (pmn < mn) ? pmn : mn;
        if (slot != SLOT_PRUNED) {   // wave-uniform
            pmn = wave_min(pmn);
            // nothing of this tile can fall below top (top <= top_ub): every pixel adds `min`, exactly like a pruned pair --
            // no values to park, and the sum pass never sees the frame
            if (__builtin_isfinite(top_ub) && pmn >= top_ub) {
                if (lane == 0) slot_of[slot_index(u, tile, Th)] = SLOT_PRUNED;
            } else {
                // lane (column pair cp, row half rg): rows 8 rg .. 8 rg + 7 of the tile, columns 2 cp, 2 cp + 1: 16 bytes per row
                F64Pair *d = reinterpret_cast<F64Pair *>(store + (size_t)slot * (CT_H * CT_W) + (size_t)(8 * (lane >> 5)) * CT_W + 2 * (lane & 31));
#pragma unroll
                for (int r = 0; r < 8; ++r) d[r * (CT_W / 2)] = F64Pair{v[r], v[8 + r]};
            }
        }
        RM_TRACE_MARK(5, 5);
    }
    mn = wave_min(mn); mx = wave_max(mx);
    RM_TRACE_MARK(5, 6);
    if (lane == 0 && blockIdx.x < n) {
        // non-returning atomics and NO load in front of them: a load here would wait (vmcnt) for the acknowledgement of the value
        // stores above, 4-15 us at 1080p x 256 (workgroup timelines, profiles/r04) -- the wave may end while its stores are in flight
        const int sp_ = blockIdx.x & (NSTRIPE - 1);
        atomicMin(&st->min_keys[sp_], f64_key(mn));
        atomicMax(&st->max_keys[sp_], f64_key(mx));
    }
}

// ---- the masked time sum of a DENSE selection at skip 3 / 4: one wave per tile, frame after frame (k_dense_sum_w's form, rm_dense_sum.h) -----
// When (nearly) every (tile, frame) pair is kept -- sensor noise in every pixel, bench.py `worst_case` -- the value store is the
// materialised video in disguise (2.1 GB written and read back at 1080p x 256).  Here a wave owns a 64 x 16 tile of the heatmap for ALL frames: TileEval of frame t
// from a private 4.4 KB slice of LDS, `raw >= top ? min : raw` added to 16 running sums per lane in frame order; a pair the selection
// pruned adds `min` to every pixel without being evaluated; no barrier, no store, no separate constant fill, every SIMD of the chip
// busy with two or three independent waves.  Same values, same order of additions as every other sum kernel: bit-identical.
constexpr int DST_MAXW = (MAX_T / 2 + 1 + 63) / 64;   // 64-frame words of a tile's kept mask

template <int S>
__global__ __launch_bounds__(64) RM_WAVES_PER_EU_IF(S <= 2, 4, 3) void k_dense_sum_t(const double *cS, ChainGeom g, int t_first, int t_end, int T, int ntiles, const int *slot_of,
                                                    CollapseState *st, double threshold, double *heat_sum, int avg_T, int *tile_nkept, SumPlan sp,
                                                    int only_if_dense, int *ran_host, const double *lo, int l1_stop)
{
    using F = TileFoot<S>;
    HIP_DYNAMIC_SHARED(double, lds)                 // the wave's footprint slice, the kept mask (DST_MAXW words), the kept frames in time order (T 16-bit entries)
    unsigned long long *s_mask = reinterpret_cast<unsigned long long *>(lds + F::TOTAL);
    unsigned short *s_list = reinterpret_cast<unsigned short *>(s_mask + DST_MAXW);
    const int lane = threadIdx.x;
    if (only_if_dense && !sum_is_dense(st, sp)) return;   // (uniform over the grid: the sparse kernel in front took the sum)
    if (ran_host && blockIdx.x == 0 && lane == 0) *ran_host = 2;   // (pinned: tells rm_locate that the stand-in it enqueued on a hint was needed)
    const int tile = dense_tile_of_block((int)blockIdx.x, ntiles);   // XCD x takes the x-th eighth of the tiles (rm_dense_sum.h)
    if (tile >= ntiles) return;
    const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    const int Th = sym_frames(T);
    const double min_val = f64_unkey(fold_min_keys(st->min_keys, st->min_key)), max_val = f64_unkey(fold_max_keys(st->max_keys, st->max_key));
    const double top = max_val - (max_val - min_val) * threshold;   // transforms.py:184-189
    if (blockIdx.x == 0 && lane == 0) { st->min_val = min_val; st->max_val = max_val; st->top = top; }
    // Which unique frames of this tile can hold a value below `top`?  The selection (k_select_pairs) had to decide with an UPPER
    // bound of top -- the exact extrema did not exist yet -- and with a loose one it keeps (nearly) every pair of a noisy stream.  Here
    // the exact top is known: a pair whose lower bound lo (minimum of its level-S footprint; every pyrUp output is a convex
    // combination of it) clears top by the pruning margin adds `min` to every pixel, evaluated or not.  Effect of this test alone (same
    // process, switch on / off): 1080p full-frame noise, skip 4: step 1.44 -> 1.20 ms; 720p skip 2 with this kernel forced: 0.567 ->
    // 0.552 (its level-2 bounds are loose -- the same test in k_dense_sum_wf, the kernel 720p takes, with a compacted frame list to keep
    // its four waves balanced, measured 115.3 against 115.0 us and was dropped).  (tile-major slot_of: a few cache lines; lo is
    // [unique frame][tile].)
    const double margin = st->margin;
    // (the exhaustive baseline and the developer switch evaluate every kept pair to the end: no level-1 minimum reaches +inf; so does
    //  a call whose top or margin is not finite -- k_select_pairs found no finite threshold, or the value range overflows float64)
    const bool prune = lo != nullptr && __builtin_isfinite(top + margin) && __builtin_isfinite(margin);
    const double top_m = prune ? top + margin : __builtin_huge_val();
    if (!prune) l1_stop = 0;   // (nothing may stop at level 1 then: a tile of NaN has no level-1 minimum below +inf, and would add `min`)
    for (int c0 = 0; c0 < Th; c0 += 64) {
        const int u = c0 + lane;
        bool kept = u < Th && slot_of[slot_index(u, tile, Th)] != SLOT_PRUNED;
        if (kept && prune) kept = !(lo[(size_t)u * ntiles + tile] - margin >= top);   // (a NaN bound keeps the pair: NaN must reach the sum)
        const unsigned long long mk = __ballot(kept);
        if (lane == 0) s_mask[c0 >> 6] = mk;
    }
    TileSetup<S> ts;
    tile_setup<S>(g, tx, ty, lane, ts);
    const size_t fs = (size_t)g.h[S] * g.w[S];
    const int H0 = g.h[0], W0 = g.w[0];
    wave_sync();
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0;
    // The kept frames of [t_first, t_end) in TIME order (round 6): the frame loop used to walk every t -- two LDS look-ups of the mask,
    // the register copies of the prefetch ring and a branch per frame, kept or not: ~25 instructions x 3 M frames that add `min`
    // anyway at 4K x 512, a sixth of the kernel's issue slots.  Now it walks the list; the frames between two entries are a count.
    int nlist = 0;
    for (int c0 = t_first; c0 < t_end; c0 += 64) {
        const int t = c0 + lane;
        bool kept = false;
        if (t < t_end) { const int u = sym_frame(t, T); kept = ((s_mask[u >> 6] >> (u & 63)) & 1ull) != 0; }
        const unsigned long long mk = __ballot(kept);
        if (kept) s_list[nlist + __popcll(mk & ((1ull << lane) - 1ull))] = (unsigned short)t;
        nlist += __popcll(mk);
    }
    wave_sync();
    // The footprints of the next two kept frames travel while this one is evaluated.  A frame that adds `min` to every pixel --
    // stopped at level 1 by tile_eval_below() -- only counts up `gap`; the additions happen, in order, in front of the next frame that
    // has real values (and at the end): ONE site with the masked additions, one with the plain ones.  A frame that stopped at level 1
    // also clears its bit in the kept mask: the band-passed signal is even in time, frame T - u is frame u again, and the second
    // visit of the pair (its list entry is looked at, its footprint not used) then costs sixteen additions.
    // l1_stop == 0: the bounds the mask was built from ARE the level-1 extrema (rm_bounds_l1.h) -- a kept pair cannot stop at level 1,
    // the running minimum of tile_eval_below() and its wave reduction (~70 instructions a visit) are left out.
    // (ONE loop body -- the frame in `cur`, the next two in n1 / n2, moved up by register copies: unrolling the body per prefetch slot
    //  doubled the evaluator's code and cost a wave per SIMD)
    double cur[F::PF], n1[F::PF], n2[F::PF];
#pragma unroll
    for (int p = 0; p < F::PF; ++p) { cur[p] = 0.0; n1[p] = 0.0; n2[p] = 0.0; }
    auto fetch = [&](double (&dst)[F::PF], int i) __attribute__((always_inline)) {
        if (i >= nlist) return;   // (uniform)
        const int t = uniform((int)s_list[i]);
        if (l1_stop) { const int u = sym_frame(t, T); if (!((s_mask[u >> 6] >> (u & 63)) & 1ull)) return; }   // (uniform) its first visit stopped at level 1: nothing to fetch
        const double *src = cS + (size_t)sym_frame(t, T) * fs;
#pragma unroll
        for (int p = 0; p < F::PF; ++p) dst[p] = src[ts.off_g[p]];
    };
    fetch(cur, 0); fetch(n1, 1);
    int nkept = 0, gap = 0, t_done = t_first;
#pragma nounroll
    for (int i = 0; i < nlist; ++i) {
        fetch(n2, i + 2);
        const int t = uniform((int)s_list[i]);
        const int u = sym_frame(t, T);
        gap += t - t_done;              // the frames in front of this one that were not kept
        t_done = t + 1;
        const bool kept = !l1_stop || ((s_mask[u >> 6] >> (u & 63)) & 1ull) != 0;   // (uniform; a first visit that stopped at level 1 cleared the bit)
        bool below = false;             // (uniform) evaluated down to level 0: the tile may hold a value below top
        double v[16];
        if (kept) {
            wave_sync();   // the previous frame's reads of the slice are behind us
#pragma unroll
            for (int p = 0; p < F::PF; ++p) if (lane + 64 * p < F::NST) lds[F::off(S) + lane + 64 * p] = cur[p];
            wave_sync();
            if (S >= 2 && l1_stop) {
                if constexpr (S >= 2) below = tile_eval_below<S>(ts, lds, lane, top_m, v);
            } else { tile_eval<S>(ts, lds, lane, v); below = true; }
            if (!below) {
                if (lane == 0) s_mask[u >> 6] &= ~(1ull << (u & 63));
                wave_sync();
            }
        }
#pragma unroll
        for (int p = 0; p < F::PF; ++p) { cur[p] = n1[p]; n1[p] = n2[p]; }
        if (!below) { ++gap; continue; }
#pragma nounroll
        for (; gap > 0; --gap) {
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = acc[j] + min_val;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = acc[j] + ((v[j] >= top) ? min_val : v[j]);
        ++nkept;
    }
    gap += t_end - t_done;
#pragma nounroll
    for (; gap > 0; --gap) {
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = acc[j] + min_val;
    }
    // base.py:562: np.average = sum / T when the whole buffer was summed here; the heatmap's extrema for base.py:563
    const double cnt = (double)avg_T;
    double hmn = __builtin_huge_val(), hmx = -__builtin_huge_val();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int y = ts.Y0 + r;
        if (y < H0) {
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                if (ts.X + o < W0) {
                    const double a = acc[8 * o + r];
                    const double q = avg_T > 0 ? a / cnt : a;
                    heat_sum[(size_t)y * W0 + ts.X + o] = q;
                    hmn = (q < hmn) ? q : hmn; hmx = (q > hmx) ? q : hmx;
                }
            }
        }
    }
    if (tile_nkept && lane == 0) tile_nkept[tile] = nkept;   // 0: every pixel of the tile is the same constant (sparse heatmap exchange)
    if (avg_T > 0) {
        hmn = wave_min(hmn); hmx = wave_max(hmx);
        if (lane == 0) {
            const unsigned long long kmn = f64_key(hmn), kmx = f64_key(hmx);
            const int sp_ = blockIdx.x & (NSTRIPE - 1);
            striped_min_max(st->heat_min_keys, st->heat_max_keys, sp_, kmn, kmx);
        }
    }
}

}  // namespace rm
