// respmon_amd/csrc/rm_small_kernels.h -- the small pyramid of one frame inside LDS (rm_front.hip), the filter-first collapse of levels
// too large for it, and the per (frame, tile) bounds of the collapsed level C_S (rm_front.hip fused with the collapse,
// rm_collapse_eval.hip on their own).
#pragma once
#include "rm_kernels.h"

namespace rm {

// ----------------------------------------------------------------------------------------
// Small pyramid, one workgroup per frame, everything in LDS (levels S..L-1 of a 1080p frame are 87 KB):
//   k_small_pyramid : G_S[t] -> G_{S+1..L-1} (cv2.pyrDown, pyramid.py:14) -> L_l = G_l - pyrUp(G_{l+1})
//                     for l = L-2..S (pyramid.py:23-26), written side by side into lap_all[t, :]
//   k_small_collapse: band-passed levels bp_all[t, :] -> c = bp_{L-2}; c = pyrUp(c) + bp_l for l = L-3..S
//                     (pyramid.py:51-57) -> C_S[t]
// Same per-pixel arithmetic as k_pyr_down / k_pyr_up (bit-identical); they replace ~13 tiny launches.
// ----------------------------------------------------------------------------------------

// whole-image pyrUp inside LDS for the one-workgroup-per-frame kernels: wave = destination row (parity and the
// border rules of the row index are wave-uniform), lane = destination column (its taps and weights fixed once per
// level, make_htap), so there is no index division and no divergent shape.  Same values as up_at(), bit for bit.
// sink(i, v) receives destination element i = y * dw + x.
template <typename Sink>
__device__ __forceinline__ void small_up_level(const double *src, int sh, int sw, int dh, int dw, int tid, Sink &&sink, int y_begin = 0, int y_end = 0x7fffffff)
{
    const int lane = tid & 63, wave = tid >> 6;
    if (y_end > dh) y_end = dh;   // destination rows [y_begin, y_end): all of them by default
    for (int x = lane; x < dw; x += 64) {
        const HTap t = make_htap(x, sw);
        for (int y = y_begin + wave; y < y_end; y += SMALL_NT / 64) {
            const int i = y >> 1;
            const double *ri = src + i * sw, *r2 = src + ((i == sh - 1) ? i : i + 1) * sw;
            const double hi_ = (ri[t.ia] * t.wa + ri[t.ib] * t.wb) + ri[t.ic] * t.wc;
            const double h2 = (r2[t.ia] * t.wa + r2[t.ib] * t.wb) + r2[t.ic] * t.wc;
            double v;
            if (y & 1) {
                v = ((hi_ + h2) * 4) * (1.0 / 64);
            } else {
                const double *r0 = src + ((i == 0) ? (sh > 1 ? 1 : 0) : i - 1) * sw;
                const double h0 = (r0[t.ia] * t.wa + r0[t.ib] * t.wb) + r0[t.ic] * t.wc;
                v = (h0 + hi_ * 6 + h2) * (1.0 / 64);
            }
            sink(y * dw + x, v);
        }
    }
}

// global -> LDS copy by one SMALL_NT-thread workgroup with 8 loads in flight per lane: a plain
// `for (i) lds[i] = src[i]` compiles to load / s_waitcnt vmcnt(0) / ds_write per iteration, i.e. one HBM round trip
// per 8 KB of a frame -- most of the run time of the one-workgroup-per-frame kernels below
__device__ __forceinline__ void fill_lds(double *dst, const double *src, int n, int tid)
{
    constexpr int U = 8;
    for (int base = 0; base < n; base += U * SMALL_NT) {
        double v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int i = base + tid + k * SMALL_NT;
            v[k] = (i < n) ? src[i] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int i = base + tid + k * SMALL_NT;
            if (i < n) dst[i] = v[k];
        }
    }
}

// st_init (nullable): workgroup 0 also resets the reduction state of the collapse passes that follow on the stream
RM_KERNEL __launch_bounds__(SMALL_NT) void k_small_pyramid(const double *gS, SmallGeom g, double *lap_all, CollapseState *st_init)
{
    RM_TRACE_SCOPE(1);
    if (st_init && blockIdx.x == 0 && threadIdx.x < 64) state_init_lane(st_init, (int)threadIdx.x);
    HIP_DYNAMIC_SHARED(double, lds)
    const int t = blockIdx.x, tid = threadIdx.x;
    const int S = g.S, L = g.L;
    RM_TRACE_MARK(1, 0);
    fill_lds(lds + g.g_off[S], gS + (size_t)t * (g.h[S] * g.w[S]), g.h[S] * g.w[S], tid);
    __syncthreads();
    RM_TRACE_MARK(1, 1);
    for (int l = S + 1; l < L; ++l) {
        const int sh = g.h[l - 1], sw = g.w[l - 1], dh = g.h[l], dw = g.w[l];
        const double *s = lds + g.g_off[l - 1];
        double *d = lds + g.g_off[l];
        for (int x = (tid & 63); x < dw; x += 64) {          // lane = column, wave = row: no index division
            const int c0 = reflect101(2 * x - 2, sw), c1 = reflect101(2 * x - 1, sw), c2 = reflect101(2 * x, sw);
            const int c3 = reflect101(2 * x + 1, sw), c4 = reflect101(2 * x + 2, sw);
            for (int y = (tid >> 6); y < dh; y += SMALL_NT / 64) {
                double r[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const double *row = s + reflect101(2 * y - 2 + k, sh) * sw;
                    r[k] = row[c2] * 6 + (row[c1] + row[c3]) * 4 + row[c0] + row[c4];
                }
                d[y * dw + x] = (r[2] * 6 + (r[1] + r[3]) * 4 + r[0] + r[4]) * (1.0 / 256);
            }
        }
        __syncthreads();
        RM_TRACE_MARK(1, 2 + (l - S - 1));
    }
    double *out = lap_all + (size_t)t * g.NP;
    for (int l = L - 2; l >= S; --l) {
        const int dh = g.h[l], dw = g.w[l], sh = g.h[l + 1], sw = g.w[l + 1];
        const double *base = lds + g.g_off[l];
        double *o = out + g.np_off[l];
        small_up_level(lds + g.g_off[l + 1], sh, sw, dh, dw, tid, [&](int i, double v) { o[i] = base[i] - v; });
        RM_TRACE_MARK(1, 8 + (L - 2 - l));
    }
}

// st_init (nullable): workgroup 0 also resets the reduction state of the collapse passes that follow on the stream
// (k_state_init's job: one tiny launch less on the critical path)
RM_KERNEL __launch_bounds__(SMALL_NT) void k_small_collapse(const double *bp_all, SmallGeom g, double *cS, CollapseState *st_init)
{
    HIP_DYNAMIC_SHARED(double, lds)   // the [NP] frame, levels laid out as in bp_all
    const int t = blockIdx.x, tid = threadIdx.x;
    if (st_init && t == 0 && tid < 64) state_init_lane(st_init, tid);
    const int S = g.S, L = g.L;
    fill_lds(lds, bp_all + (size_t)t * g.NP, g.NP, tid);
    __syncthreads();
    for (int l = L - 3; l >= S; --l) {
        const int dh = g.h[l], dw = g.w[l], sh = g.h[l + 1], sw = g.w[l + 1];
        double *d = lds + g.np_off[l];
        small_up_level(lds + g.np_off[l + 1], sh, sw, dh, dw, tid, [&](int i, double v) { d[i] = v + d[i]; });
        __syncthreads();
    }
    const int n = g.h[S] * g.w[S];
    double *o = cS + (size_t)t * n;
    for (int i = tid; i < n; i += SMALL_NT) o[i] = lds[g.np_off[S] + i];
}

// per (frame, tile) bounds of the level-S footprint: every full-resolution value of the tile
// is a convex combination of these, so  lo - margin <= raw <= hi + margin.
// Layout [t][tile]: consecutive lanes take consecutive tiles of one frame (overlapping, x-contiguous
// footprints -> coalesced reads).
// (k_tile_bounds, below, follows the lattice samples it also takes)

// Lattice samples.  The tile bounds say where raw.min() / raw.max() CAN be; how low `top` can be -- and with it how many
// pairs must be evaluated -- hangs on an UPPER bound of raw.min() and a LOWER bound of raw.max(), and the bounds alone
// give poor ones (min over pairs of hi, max over pairs of lo: -39 / +40 against the true -50 / +51 on the synthetic
// 1080p stream, so top_ub = -12 instead of -19.7 and 9 066 pairs kept instead of ~5 000).  Any true value of raw
// bounds them far better, and some come almost for free: the full-resolution pixel (y << S, x << S) of an interior
// level-S pixel is, through every pyrUp step, the even-even sample of its 3 x 3 level-S neighbourhood -- per axis
// lat_a * (c[y-1] + c[y+1]) + lat_b * c[y] with dyadic weights (S = 4: 85/512, 342/512) -- because position p << k at level
// S-k only ever draws on positions (p << (k-1)) - 1 .. + 1 one level up, none of which touches a border rule for 1 <= p <=
// size - 2.  The weights are applied directly (a few roundings, ~3e-15 relative to max|c|, against the chain's own few), so
// the samples enter the selection with twice the pruning margin (1e-12 relative).  Pruning stays exact: the evaluated
// pairs still yield the exact extrema, only fewer pairs need evaluating.
__device__ __forceinline__ double lattice_sample(const double *r0, const double *r1, const double *r2, int x, double a, double b)
{
    const double h0 = (r0[x - 1] + r0[x + 1]) * a + r0[x] * b;
    const double h1 = (r1[x - 1] + r1[x + 1]) * a + r1[x] * b;
    const double h2 = (r2[x - 1] + r2[x + 1]) * a + r2[x] * b;
    return (h0 + h2) * a + h1 * b;
}

// The four extrema of the bounds (over ALL pairs) are reduced here as well: block-level min/max, then striped
// atomics that are skipped when they cannot change the result.
RM_KERNEL __launch_bounds__(256) void k_tile_bounds(const double *cS, ChainGeom g, int T, int ntiles,
                                                     double *lo, double *hi, CollapseState *st, int *sel_cnt)
{
    const double inf = __builtin_huge_val();
    if (blockIdx.x == 0) for (int i = threadIdx.x; i < ntiles; i += 256) sel_cnt[i] = 0;   // k_select_pairs counts into it
    int idx = blockIdx.x * 256 + threadIdx.x;
    double mn = inf, mx = -inf;
    if (idx < ntiles * T) {
        int t = idx / ntiles, tile = idx - t * ntiles;
        const int S = g.S;
        const Region R = tile_region(g, tile, S);
        const int wS = g.w[S];
        const double *p = cS + (size_t)t * g.h[S] * wS;
        mn = p[(size_t)R.y0 * wS + R.x0]; mx = mn;
        for (int y = R.y0; y <= R.y1; ++y)
            for (int x = R.x0; x <= R.x1; ++x) {
                double v = p[(size_t)y * wS + x];
                mn = (v < mn) ? v : mn;
                mx = (v > mx) ? v : mx;
            }
        lo[idx] = mn; hi[idx] = mx;
    }
    // lanes past the end hold (+inf, -inf): neutral for min-of-lo / max-of-hi; for max-of-lo / min-of-hi they must
    // not take part, so those two use the swapped neutral elements
    double lo_mn = mn, lo_mx = (idx < ntiles * T) ? mn : -inf;
    double hi_mx = mx, hi_mn = (idx < ntiles * T) ? mx : inf;
    block_minmax(lo_mn, lo_mx);
    block_minmax(hi_mn, hi_mx);
    if (threadIdx.x == 0) {
        const unsigned long long k_lo_mx = f64_key(lo_mx), k_lo_mn = f64_key(lo_mn), k_hi_mx = f64_key(hi_mx), k_hi_mn = f64_key(hi_mn);
        const int sp = blockIdx.x & (NSTRIPE - 1);
        striped_min_max(st->lb_min_keys, st->lb_max_keys, sp, k_lo_mn, k_lo_mx);
        striped_min_max(st->ub_min_keys, st->ub_max_keys, sp, k_hi_mn, k_hi_mx);
    }
}

// The same bounds, one workgroup per frame: the level-S footprint of a tile is a rectangle, so its min / max is
// the min / max over the footprint rows of per-row extrema over the footprint columns (exact: min and max are
// associative).  Row extrema for every (row, tile column) go to LDS first; ~3.6x fewer loads than k_tile_bounds
// and no per-thread 2-D loop over global memory.  Used when the [h_S][tiles_x] x 2 table fits LDS.
// blockIdx.y selects a band of `band` tile rows (large levels: the row-extrema table of a whole frame would not fit LDS);
// the table then holds only the level-S rows [y_lo, y_hi] that band's footprints touch (at most `tbl_rows` of them).
RM_KERNEL __launch_bounds__(256) void k_frame_bounds(const double *cS, ChainGeom g, int ntiles, double *lo, double *hi,
                                                      CollapseState *st, int band, int tbl_rows, int *sel_cnt)
{
    HIP_DYNAMIC_SHARED(double, lds)
    if (blockIdx.x == 0 && blockIdx.y == 0) for (int i = threadIdx.x; i < ntiles; i += 256) sel_cnt[i] = 0;   // k_select_pairs counts into it
    const double inf = __builtin_huge_val();
    const int S = g.S, hS = g.h[S], wS = g.w[S], ntx = g.tiles_x;
    const int t = blockIdx.x;
    const int ty0 = blockIdx.y * band, ty1 = min(ty0 + band, g.tiles_y) - 1;             // tile rows of this workgroup
    const int y_lo = tile_region(g, ty0 * ntx, S).y0, y_hi = tile_region(g, ty1 * ntx, S).y1;   // level-S rows they touch
    const int nrows = y_hi - y_lo + 1;
    double *rmin = lds, *rmax = lds + (size_t)tbl_rows * ntx;
    const double *p = cS + (size_t)t * hS * wS;
    const float inv_ntx = 1.0f / (float)ntx;
    double t_mn = inf, t_mx = -inf;
    int p_mn = -1, p_mx = -1;
    for (int i = threadIdx.x; i < nrows * ntx; i += 256) {
        int y, tx;
        split_rc(i, ntx, inv_ntx, y, tx);
        const Region R = tile_region(g, tx, S);   // tile tx of the first tile row: same column range as every tile below it
        const double *row = p + (size_t)(y_lo + y) * wS;
        double mn = row[R.x0], mx = mn;
        int xn = R.x0, xx = R.x0;
        // FB_CHUNK loads in flight per thread (the plain loop waited for every element in turn: ~20 dependent round trips per
        // footprint row at skip 2).  Columns past the footprint repeat its last one: a repeated value changes neither the
        // extrema nor the first position they were met at, so the result is that of the element-by-element scan.
        constexpr int FB_CHUNK = 10;
        for (int x = R.x0 + 1; x <= R.x1; x += FB_CHUNK) {
            double v[FB_CHUNK];
#pragma unroll
            for (int j = 0; j < FB_CHUNK; ++j) v[j] = row[min(x + j, R.x1)];
#pragma unroll
            for (int j = 0; j < FB_CHUNK; ++j) {
                const int xj = min(x + j, R.x1);
                if (v[j] < mn) { mn = v[j]; xn = xj; }
                if (v[j] > mx) { mx = v[j]; xx = xj; }
            }
        }
        rmin[i] = mn; rmax[i] = mx;
        // (where this thread has seen the lowest / highest C_S so far: its lattice samples are taken there)
        if (mn < t_mn) { t_mn = mn; p_mn = (y_lo + y) * wS + xn; }
        if (mx > t_mx) { t_mx = mx; p_mx = (y_lo + y) * wS + xx; }
    }
    __syncthreads();
    double lo_mn = inf, lo_mx = -inf, hi_mn = inf, hi_mx = -inf;
    const int tile_begin = ty0 * ntx, tile_end = (ty1 + 1) * ntx;
    for (int tile = tile_begin + threadIdx.x; tile < tile_end; tile += 256) {
        const int tx = tile % ntx;
        const Region R = tile_region(g, tile, S);
        double mn = rmin[(R.y0 - y_lo) * ntx + tx], mx = rmax[(R.y0 - y_lo) * ntx + tx];
        for (int y = R.y0 + 1; y <= R.y1; ++y) {
            const double a = rmin[(y - y_lo) * ntx + tx], b = rmax[(y - y_lo) * ntx + tx];
            mn = (a < mn) ? a : mn;
            mx = (b > mx) ? b : mx;
        }
        lo[(size_t)t * ntiles + tile] = mn; hi[(size_t)t * ntiles + tile] = mx;
        lo_mn = (mn < lo_mn) ? mn : lo_mn; lo_mx = (mn > lo_mx) ? mn : lo_mx;
        hi_mn = (mx < hi_mn) ? mx : hi_mn; hi_mx = (mx > hi_mx) ? mx : hi_mx;
    }
    // lattice samples (true raw values: see lattice_sample) at the interior pixels nearest to the lowest / highest C_S each
    // thread met in the first loop: two per thread bound the extrema as well as sampling every pixel would (a sample per
    // pixel -- nine global loads each -- made this kernel 6x slower on the 180 x 320 level of the 720p configuration)
    double sm_mn = inf, sm_mx = -inf;
    if (hS >= 3 && wS >= 3) {
        const int cand[2] = {p_mn, p_mx};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (cand[k] < 0) continue;
            int y = cand[k] / wS, x = cand[k] - y * wS;
            y = min(max(y, 1), hS - 2); x = min(max(x, 1), wS - 2);
            const double *r1 = p + (size_t)y * wS;
            const double v = lattice_sample(r1 - wS, r1, r1 + wS, x, g.lat_a, g.lat_b);
            sm_mn = (v < sm_mn) ? v : sm_mn; sm_mx = (v > sm_mx) ? v : sm_mx;
        }
    }
    block_minmax(lo_mn, lo_mx);
    block_minmax(hi_mn, hi_mx);
    block_minmax(sm_mn, sm_mx);
    if (threadIdx.x == 0) {
        const unsigned long long k_lo_mx = f64_key(lo_mx), k_lo_mn = f64_key(lo_mn), k_hi_mx = f64_key(hi_mx), k_hi_mn = f64_key(hi_mn);
        const int sp = (blockIdx.x + blockIdx.y * 7) & (NSTRIPE - 1);
        striped_min_max(st->lb_min_keys, st->lb_max_keys, sp, k_lo_mn, k_lo_mx);
        striped_min_max(st->ub_min_keys, st->ub_max_keys, sp, k_hi_mn, k_hi_mx);
        if (sm_mn <= sm_mx) {
            const unsigned long long k_mn = f64_key(sm_mn), k_mx = f64_key(sm_mx);
            striped_min_max(st->smp_min_keys, st->smp_max_keys, sp, k_mn, k_mx);
        }
    }
}

// k_frame_bounds for wide levels (4K, skip 2), streaming: no row-extrema table, no workgroup barrier.  In k_frame_bounds a
// thread per (row, tile column) reads its footprint straight from memory, lanes 64 >> S columns apart -- every load instruction
// touches 64 cache lines -- and a band's table (100 KB at 4K) leaves one workgroup per CU.  Here a WAVE owns FB_TR consecutive tile
// rows of a frame and walks down the level-S rows their footprints touch: lanes load consecutive columns (FB_MAXNL loads in flight,
// the next row requested before this one is scanned), park the row in a skewed LDS buffer (index i + (i >> 4): the scans of
// neighbouring tile columns hit different banks), lane tx takes the extrema of tile column tx's footprint columns from there and
// folds them into the running extrema of the (at most two) tile rows whose footprint holds this row.  8 KB of LDS per wave.
// Same bounds (min / max are exact in any order); the lattice samples are taken where a LANE met its extreme values, so the
// sample set -- and with it how many pairs the selection keeps, never the result -- differs from k_frame_bounds'.
constexpr int FB_MAXNL = 16;   // row length <= 64 * FB_MAXNL level-S columns
// FB_TR (template): tile rows per wave -- 8 where that still gives every SIMD a few waves (halo rows: 12 %), 2 for small images
__host__ __device__ __forceinline__ int fb_row_pitch(int wS) { return wS + (wS >> 4) + 2; }

template <int FB_TR>
__global__ __launch_bounds__(256) void k_frame_bounds_rows(const double *cS, ChainGeom g, int ntiles, double *lo, double *hi,
                                                           CollapseState *st, int *sel_cnt)
{
    HIP_DYNAMIC_SHARED(double, lds)
    if (blockIdx.x == 0 && blockIdx.y == 0) for (int i = threadIdx.x; i < ntiles; i += 256) sel_cnt[i] = 0;   // k_select_pairs counts into it
    const double inf = __builtin_huge_val();
    const int S = g.S, hS = g.h[S], wS = g.w[S], ntx = g.tiles_x;
    const int t = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ty_first = (blockIdx.y * 4 + wave) * FB_TR;
    const int ty_last = min(ty_first + FB_TR, g.tiles_y) - 1;
    const bool have = ty_first <= ty_last;               // (wave-uniform; waves past the last tile row only keep the barriers company)
    const int y_lo = have ? tile_region(g, ty_first * ntx, S).y0 : 0, y_hi = have ? tile_region(g, ty_last * ntx, S).y1 : -1;
    const int nrows = y_hi - y_lo + 1;
    int nrows_max = 0;                                   // trips every wave of the workgroup makes (host emulation: wave_sync() is a barrier)
    for (int w = 0; w < 4; ++w) {
        const int a = (blockIdx.y * 4 + w) * FB_TR, b = min(a + FB_TR, g.tiles_y) - 1;
        if (a <= b) nrows_max = max(nrows_max, tile_region(g, b * ntx, S).y1 - tile_region(g, a * ntx, S).y0 + 1);
    }
    double *rowbuf = lds + (size_t)wave * fb_row_pitch(wS);
    const double *p = cS + (size_t)t * hS * wS;
    const int nl = (wS + 63) >> 6;
    const int tx = min(lane, ntx - 1);
    const Region Rx = tile_region(g, tx, S);             // column range of tile column tx (the same in every tile row)
    double amn[FB_TR], amx[FB_TR];
#pragma unroll
    for (int k = 0; k < FB_TR; ++k) { amn[k] = inf; amx[k] = -inf; }
    double t_mn = inf, t_mx = -inf;
    int p_mn = -1, p_mx = -1;
    double nxt[FB_MAXNL];
    auto fetch = [&](int y) __attribute__((always_inline)) {
        const double *row = p + (size_t)min(y_lo + max(min(y, nrows - 1), 0), hS - 1) * wS;
#pragma unroll
        for (int j = 0; j < FB_MAXNL; ++j)
            if (j < nl) nxt[j] = row[min(lane + 64 * j, wS - 1)];
    };
    fetch(0);
    for (int y = 0; y < nrows_max; ++y) {
#pragma unroll
        for (int j = 0; j < FB_MAXNL; ++j) {
            const int x = lane + 64 * j;
            if (j < nl && x < wS) rowbuf[x + (x >> 4)] = nxt[j];
        }
        fetch(y + 1);
        wave_sync();
        if (y < nrows) {
            double mn = rowbuf[Rx.x0 + (Rx.x0 >> 4)], mx = mn;
            for (int x = Rx.x0 + 1; x <= Rx.x1; ++x) {
                const double v = rowbuf[x + (x >> 4)];
                mn = (v < mn) ? v : mn; mx = (v > mx) ? v : mx;
            }
            const int ya = y_lo + y;
#pragma unroll
            for (int k = 0; k < FB_TR; ++k) {
                const int ty = ty_first + k;
                if (ty <= ty_last) {
                    const Region R = tile_region(g, ty * ntx, S);
                    if (ya >= R.y0 && ya <= R.y1) { amn[k] = (mn < amn[k]) ? mn : amn[k]; amx[k] = (mx > amx[k]) ? mx : amx[k]; }   // (uniform)
                }
            }
            // the ROW in which this lane met its lowest / highest C_S so far; the column is looked up once, at the end
            if (mn < t_mn) { t_mn = mn; p_mn = ya; }
            if (mx > t_mx) { t_mx = mx; p_mx = ya; }
        }
        wave_sync();
    }
    if (have && lane < ntx) {   // first column of the extreme value inside its row's footprint
        if (p_mn >= 0) { const double *row = p + (size_t)p_mn * wS; int x = Rx.x0; while (x < Rx.x1 && row[x] != t_mn) ++x; p_mn = p_mn * wS + x; }
        if (p_mx >= 0) { const double *row = p + (size_t)p_mx * wS; int x = Rx.x0; while (x < Rx.x1 && row[x] != t_mx) ++x; p_mx = p_mx * wS + x; }
    }
    double lo_mn = inf, lo_mx = -inf, hi_mn = inf, hi_mx = -inf;
    if (have && lane < ntx) {
#pragma unroll
        for (int k = 0; k < FB_TR; ++k) {
            const int ty = ty_first + k;
            if (ty <= ty_last) {
                const size_t o = (size_t)t * ntiles + (size_t)ty * ntx + lane;
                lo[o] = amn[k]; hi[o] = amx[k];
                lo_mn = (amn[k] < lo_mn) ? amn[k] : lo_mn; lo_mx = (amn[k] > lo_mx) ? amn[k] : lo_mx;
                hi_mn = (amx[k] < hi_mn) ? amx[k] : hi_mn; hi_mx = (amx[k] > hi_mx) ? amx[k] : hi_mx;
            }
        }
    }
    double sm_mn = inf, sm_mx = -inf;
    if (have && lane < ntx && hS >= 3 && wS >= 3) {
        const int cand[2] = {p_mn, p_mx};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (cand[k] < 0) continue;
            int y = cand[k] / wS, x = cand[k] - y * wS;
            y = min(max(y, 1), hS - 2); x = min(max(x, 1), wS - 2);
            const double *r1 = p + (size_t)y * wS;
            const double v = lattice_sample(r1 - wS, r1, r1 + wS, x, g.lat_a, g.lat_b);
            sm_mn = (v < sm_mn) ? v : sm_mn; sm_mx = (v > sm_mx) ? v : sm_mx;
        }
    }
    lo_mn = wave_min(lo_mn); lo_mx = wave_max(lo_mx); hi_mn = wave_min(hi_mn); hi_mx = wave_max(hi_mx);
    sm_mn = wave_min(sm_mn); sm_mx = wave_max(sm_mx);
    if (lane == 0 && have) {
        const unsigned long long k_lo_mx = f64_key(lo_mx), k_lo_mn = f64_key(lo_mn), k_hi_mx = f64_key(hi_mx), k_hi_mn = f64_key(hi_mn);
        const int sp = (blockIdx.x + (blockIdx.y * 4 + wave) * 7) & (NSTRIPE - 1);
        striped_min_max(st->lb_min_keys, st->lb_max_keys, sp, k_lo_mn, k_lo_mx);
        striped_min_max(st->ub_min_keys, st->ub_max_keys, sp, k_hi_mn, k_hi_mx);
        if (sm_mn <= sm_mx) {
            const unsigned long long k_mn = f64_key(sm_mn), k_mx = f64_key(sm_mx);
            striped_min_max(st->smp_min_keys, st->smp_max_keys, sp, k_mn, k_mx);
        }
    }
}

// k_small_collapse and k_frame_bounds in one: the collapsed level S of a frame is still in LDS when its tile bounds are
// wanted, so they are taken from there (no second pass over C_S in memory, one kernel boundary less).  Used when the
// row-extrema table of a whole frame fits beside the frame's small pyramid.
// What follows the collapse of a frame, with C_S of the frame in LDS at `c`: copy-out to cS[t], tile bounds (per-row extrema
// over the footprint columns, then extrema over the footprint rows) from the LDS copy, their extrema and the lattice samples
// into the striped state.  rmin / rmax: the row-extrema table, 2 x hS x tiles_x doubles of LDS.  One SMALL_NT-thread workgroup.
// A workgroup may own only PART of the frame (k_small_filter_first puts two workgroups on a frame): tile rows [ty_a, ty_b), whose
// footprints touch the level-S rows [y_lo, y_hi] (valid in `c`), and the rows [y_out_a, y_out_b) it copies out.
__device__ __forceinline__ void frame_bounds_from_lds(const double *c, double *rmin_base, const SmallGeom &sg, const ChainGeom &g, int ntiles, int t,
                                                      double *cS, double *lo, double *hi, CollapseState *st, double (*s_red)[SMALL_NT / 64],
                                                      int (*s_arg)[SMALL_NT / 64], int mark_kid, int ty_a = 0, int ty_b = 0x7fffffff,
                                                      int y_lo = 0, int y_hi = 0x7fffffff, int y_out_a = 0, int y_out_b = 0x7fffffff)
{
    const int tid = threadIdx.x;
    const int S = sg.S;
    const int hS = sg.h[S], wS = sg.w[S], ntx = g.tiles_x;
    if (ty_b > g.tiles_y) ty_b = g.tiles_y;
    if (y_hi > hS - 1) y_hi = hS - 1;
    if (y_out_b > hS) y_out_b = hS;
    double *o = cS + (size_t)t * (hS * wS);
    // (the copy-out loop also finds where this part of the frame's C_S is lowest / highest: the lattice samples are taken there)
    const double inf = __builtin_huge_val();
    double c_mn = inf, c_mx = -inf;
    int i_mn = y_out_a * wS, i_mx = y_out_a * wS;
    for (int i = y_out_a * wS + tid; i < y_out_b * wS; i += SMALL_NT) {
        const double v = c[i];
        o[i] = v;
        if (v < c_mn) { c_mn = v; i_mn = i; }
        if (v > c_mx) { c_mx = v; i_mx = i; }
    }
    RM_TRACE_MARK(mark_kid, 8);
    // tile bounds from the LDS copy: per-row extrema over the footprint columns, then extrema over the footprint rows
    double *rmin = rmin_base, *rmax = rmin + (size_t)hS * ntx;
    const float inv_ntx = 1.0f / (float)ntx;
    for (int i = y_lo * ntx + tid; i < (y_hi + 1) * ntx; i += SMALL_NT) {
        int y, tx;
        split_rc(i, ntx, inv_ntx, y, tx);
        const Region R = tile_region(g, tx, S);
        const double *row = c + y * wS;
        double mn = row[R.x0], mx = mn;
        for (int x = R.x0 + 1; x <= R.x1; ++x) {
            const double v = row[x];
            mn = (v < mn) ? v : mn;
            mx = (v > mx) ? v : mx;
        }
        rmin[i] = mn; rmax[i] = mx;
    }
    __syncthreads();
    RM_TRACE_MARK(mark_kid, 9);
    
    double lo_mn = inf, lo_mx = -inf, hi_mn = inf, hi_mx = -inf;
    (void)ntiles;
    for (int tile = ty_a * ntx + tid; tile < ty_b * ntx; tile += SMALL_NT) {
        const int tx = tile % ntx;
        const Region R = tile_region(g, tile, S);
        double mn = rmin[R.y0 * ntx + tx], mx = rmax[R.y0 * ntx + tx];
        for (int y = R.y0 + 1; y <= R.y1; ++y) {
            const double a = rmin[y * ntx + tx], b = rmax[y * ntx + tx];
            mn = (a < mn) ? a : mn;
            mx = (b > mx) ? b : mx;
        }
        lo[(size_t)t * ntiles + tile] = mn; hi[(size_t)t * ntiles + tile] = mx;
        lo_mn = (mn < lo_mn) ? mn : lo_mn; lo_mx = (mn > lo_mx) ? mn : lo_mx;
        hi_mn = (mx < hi_mn) ? mx : hi_mn; hi_mx = (mx > hi_mx) ? mx : hi_mx;
    }
    lo_mn = wave_min(lo_mn); lo_mx = wave_max(lo_mx); hi_mn = wave_min(hi_mn); hi_mx = wave_max(hi_mx);
    // wave-level arg-min / arg-max of C_S (value and position travel together)
    wave_arg_reduce(c_mn, i_mn, [](double o, double w) { return o < w; });
    wave_arg_reduce(c_mx, i_mx, [](double o, double w) { return o > w; });
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        s_red[0][wave] = lo_mn; s_red[1][wave] = lo_mx; s_red[2][wave] = hi_mn; s_red[3][wave] = hi_mx;
        s_red[4][wave] = c_mn; s_red[5][wave] = c_mx; s_arg[0][wave] = i_mn; s_arg[1][wave] = i_mx;
    }
    __syncthreads();
    RM_TRACE_MARK(mark_kid, 11);
    if (wave != 0) return;
    {   // wave 0 folds the per-wave partials: lane w takes wave w's
        const bool have = tid < SMALL_NT / 64;
        lo_mn = have ? s_red[0][tid] : inf; lo_mx = have ? s_red[1][tid] : -inf;
        hi_mn = have ? s_red[2][tid] : inf; hi_mx = have ? s_red[3][tid] : -inf;
        c_mn = have ? s_red[4][tid] : inf; c_mx = have ? s_red[5][tid] : -inf;
        i_mn = have ? s_arg[0][tid] : 0; i_mx = have ? s_arg[1][tid] : 0;
        lo_mn = wave_min(lo_mn); lo_mx = wave_max(lo_mx); hi_mn = wave_min(hi_mn); hi_mx = wave_max(hi_mx);
        wave_arg_reduce(c_mn, i_mn, [](double o, double w) { return o < w; });
        wave_arg_reduce(c_mx, i_mx, [](double o, double w) { return o > w; });
    }
    if (tid == 0) {
        const unsigned long long k_lo_mx = f64_key(lo_mx), k_lo_mn = f64_key(lo_mn), k_hi_mx = f64_key(hi_mx), k_hi_mn = f64_key(hi_mn);
        const int sp = blockIdx.x & (NSTRIPE - 1);
        atomicMax(&st->lb_max_keys[sp], k_lo_mx);
        atomicMin(&st->lb_min_keys[sp], k_lo_mn);
        atomicMax(&st->ub_max_keys[sp], k_hi_mx);
        atomicMin(&st->ub_min_keys[sp], k_hi_mn);
        // lattice samples (true raw values: see lattice_sample) at the interior pixels nearest to this frame's lowest and
        // highest C_S: on the synthetic 1080p stream they bound the extrema as tightly as sampling every pixel would
        if (hS >= 3 && wS >= 3) {
            int ya = i_mn / wS, xa = i_mn - ya * wS, yb = i_mx / wS, xb = i_mx - yb * wS;
            const int y_first = max(1, y_lo + 1), y_last = max(y_first, min(hS - 2, y_hi - 1));   // rows whose 3 x 3 neighbourhood is valid in `c`
            ya = min(max(ya, y_first), y_last); xa = min(max(xa, 1), wS - 2);
            yb = min(max(yb, y_first), y_last); xb = min(max(xb, 1), wS - 2);
            const double *ra = c + ya * wS, *rb = c + yb * wS;
            const double va = lattice_sample(ra - wS, ra, ra + wS, xa, g.lat_a, g.lat_b);
            const double vb = lattice_sample(rb - wS, rb, rb + wS, xb, g.lat_a, g.lat_b);
            atomicMin(&st->smp_min_keys[sp], f64_key(va < vb ? va : vb));
            atomicMax(&st->smp_max_keys[sp], f64_key(va > vb ? va : vb));
        }
    }
    RM_TRACE_MARK(mark_kid, 12);
}

RM_KERNEL __launch_bounds__(SMALL_NT) void k_small_collapse_bounds(const double *bp_all, SmallGeom sg, double *cS, CollapseState *st,
                                                                     ChainGeom g, int ntiles, double *lo, double *hi, int *sel_cnt)
{
    RM_TRACE_SCOPE(3);
    if (blockIdx.x == 0) for (int i = threadIdx.x; i < ntiles; i += SMALL_NT) sel_cnt[i] = 0;   // k_select_pairs counts into it
    HIP_DYNAMIC_SHARED(double, lds)   // [NP] frame (levels laid out as in bp_all), then the row-extrema table
    __shared__ double s_red[6][SMALL_NT / 64];
    __shared__ int s_arg[2][SMALL_NT / 64];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int S = sg.S, L = sg.L;
    // (st was reset by an EARLIER kernel on the stream -- k_small_pyramid or k_state_init: the atomics at the end of this
    //  kernel must not race with a reset inside it)
    RM_TRACE_MARK(3, 0);
    fill_lds(lds, bp_all + (size_t)t * sg.NP, sg.NP, tid);
    __syncthreads();
    RM_TRACE_MARK(3, 1);
    for (int l = L - 3; l >= S; --l) {
        const int dh = sg.h[l], dw = sg.w[l], sh = sg.h[l + 1], sw = sg.w[l + 1];
        double *d = lds + sg.np_off[l];
        small_up_level(lds + sg.np_off[l + 1], sh, sw, dh, dw, tid, [&](int i, double v) { d[i] = v + d[i]; });
        __syncthreads();
        RM_TRACE_MARK(3, 2 + (L - 3 - l));
    }
    frame_bounds_from_lds(lds + sg.np_off[S], lds + sg.NP, sg, g, ntiles, t, cS, lo, hi, st, s_red, s_arg, 3);
}

// ---- filter-first form of the small pyramid (round 2) ---------------------------------------------------------------------
// The temporal band-pass is linear and acts per pixel, the pyramid steps are linear and act per frame: they commute.  With
// X_l = B(G_l) = pyrDown^(l-S)(X_S) the band-passed Laplacians are L_l = X_l - pyrUp(X_{l+1}) (pyramid.py:23-26), and the collapse
// (pyramid.py:51-57: img = pyrUp(img) + L_l from a zero coarsest level) telescopes:
//     C_{L-2} = X_{L-2} - pyrUp(X_{L-1}),   C_l = pyrUp(C_{l+1}) + X_l - pyrUp(X_{l+1}) = X_l - pyrUp^(L-1-l)(X_{L-1})
// so  C_S = X_S - pyrUp^(L-1-S)(pyrDown^(L-1-S)(X_S)):  filter G_S once ([T, h_S w_S]), then ONE per-frame kernel walks down to
// the coarsest level, back up, and subtracts.  k_small_pyramid, its [T, NP] Laplacian / band-passed arrays, a quarter of the
// filter's pixels and half of the collapse's pyrUp work go.
// The price is the rounding ORDER: the reference filters the Laplacians and adds them up, this filters their common source, so
// C_S agrees with the per-level path to ~1e-15 relative instead of bit for bit (the ROI and the uint8 heatmap are unaffected
// except on exact ties of the mask threshold -- the same class of event the explicit filter operator already belongs to).
// RM_FLAG_FILTER_LAPLACIANS selects the reference's order (k_small_pyramid / k_small_collapse_bounds above).
// LDS: the levels S .. L-1 (sg.g_off; levels S+1 .. L-2 are overwritten on the way up), then the bounds table.
RM_KERNEL __launch_bounds__(SMALL_NT) void k_small_filter_first(const double *xg, SmallGeom sg, int lds_levels, double *cS, CollapseState *st,
                                                                  ChainGeom g, int ntiles, double *lo, double *hi, int *sel_cnt, int parts)
{
    RM_TRACE_SCOPE(3);
    if (blockIdx.x == 0) for (int i = threadIdx.x; i < ntiles; i += SMALL_NT) sel_cnt[i] = 0;   // k_select_pairs counts into it
    HIP_DYNAMIC_SHARED(double, lds)
    __shared__ double s_red[6][SMALL_NT / 64];
    __shared__ int s_arg[2][SMALL_NT / 64];
    // `parts` workgroups per frame (gridDim.x = frames * parts): each walks the whole way down and back up to level S + 1 (those
    // levels are a quarter of the frame and less), then takes the last step up, the subtraction, the copy-out and the bounds for ITS
    // band of tile rows only -- with one workgroup per unique frame half of the chip's CUs had nothing to do (129 frames at T = 256)
    const int t = blockIdx.x / parts, part = blockIdx.x - t * parts, tid = threadIdx.x;
    const int S = sg.S, L = sg.L;
    const int nS = sg.h[S] * sg.w[S];
    const int ty_a = (int)((long long)g.tiles_y * part / parts), ty_b = (int)((long long)g.tiles_y * (part + 1) / parts);
    const int y_lo = parts == 1 ? 0 : tile_region(g, ty_a * g.tiles_x, S).y0;
    const int y_hi = parts == 1 ? sg.h[S] - 1 : tile_region(g, (ty_b - 1) * g.tiles_x, S).y1;
    // rows this part copies out: the frame's rows cut where the parts' tile rows are cut (inside both neighbours' computed ranges)
    const int y_out_a = part == 0 ? 0 : min(sg.h[S], (ty_a * CT_H) >> S), y_out_b = part == parts - 1 ? sg.h[S] : min(sg.h[S], (ty_b * CT_H) >> S);
    RM_TRACE_MARK(3, 0);
    fill_lds(lds + sg.g_off[S], xg + (size_t)t * nS, nS, tid);
    __syncthreads();
    RM_TRACE_MARK(3, 1);
    for (int l = S + 1; l < L; ++l) {   // cv2.pyrDown chain of the filtered level (pyramid.py:14)
        const int sh = sg.h[l - 1], sw = sg.w[l - 1], dh = sg.h[l], dw = sg.w[l];
        const double *sp = lds + sg.g_off[l - 1];
        double *d = lds + sg.g_off[l];
        for (int x = (tid & 63); x < dw; x += 64) {
            const int c0 = reflect101(2 * x - 2, sw), c1 = reflect101(2 * x - 1, sw), c2 = reflect101(2 * x, sw);
            const int c3 = reflect101(2 * x + 1, sw), c4 = reflect101(2 * x + 2, sw);
            for (int y = (tid >> 6); y < dh; y += SMALL_NT / 64) {
                double r[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const double *row = sp + reflect101(2 * y - 2 + k, sh) * sw;
                    r[k] = row[c2] * 6 + (row[c1] + row[c3]) * 4 + row[c0] + row[c4];
                }
                d[y * dw + x] = (r[2] * 6 + (r[1] + r[3]) * 4 + r[0] + r[4]) * (1.0 / 256);
            }
        }
        __syncthreads();
    }
    RM_TRACE_MARK(3, 2);
    for (int l = L - 2; l >= S; --l) {   // back up: U_l = pyrUp(U_{l+1}) over the dead X_l, and C_S = X_S - U_S in place
        const int dh = sg.h[l], dw = sg.w[l], sh = sg.h[l + 1], sw = sg.w[l + 1];
        double *d = lds + sg.g_off[l];
        const bool last = l == S;
        small_up_level(lds + sg.g_off[l + 1], sh, sw, dh, dw, tid, [&](int i, double v) { d[i] = last ? d[i] - v : v; }, last ? y_lo : 0,
                       last ? y_hi + 1 : 0x7fffffff);
        __syncthreads();
    }
    RM_TRACE_MARK(3, 4);
    frame_bounds_from_lds(lds + sg.g_off[S], lds + lds_levels, sg, g, ntiles, t, cS, lo, hi, st, s_red, s_arg, 3, ty_a, ty_b, y_lo, y_hi, y_out_a, y_out_b);
}

// Filter-first collapse of levels too large for LDS (4K, skip 2; rm_front.hip front_filter): with X_l the band-passed Gaussian levels,
//     C_S = X_S - pyrUp^n(X_{L-1}),  n = L - 1 - S        (the telescoped collapse, see k_small_filter_first)
// for one 64 x 16 tile of level S per work item: the footprint of the tile at the coarsest level is staged in LDS, the pyrUp chain
// runs there exactly as in k_eval_pairs (`g` describes levels S .. L-1 as its levels 0 .. n), the last step lands in registers
// (lane = column, 16 rows) and is subtracted from the tile of X_S, requested before the chain starts.  X_S is read once, C_S
// written once, the intermediate levels U_l never exist (three k_pyr_up launches over the 2.1 GB level at 4K x 512 did 1.05 ms).
// Same per-pixel arithmetic as k_pyr_up (modes 0 and 1): bit-identical.
RM_KERNEL __launch_bounds__(64) void k_ff_collapse(const double *xS, const double *xL, ChainGeom g, int ntiles, int nitems, double *cS)
{
    HIP_DYNAMIC_SHARED(double, lds)
    const int lane = threadIdx.x;
    const int w0 = g.w[0];
    const size_t fs0 = (size_t)g.h[0] * w0, fsL = (size_t)g.h[g.S] * g.w[g.S];
    for (int c = blockIdx.x; c < nitems; c += gridDim.x) {
        const int u = c / ntiles, tile = c - u * ntiles;   // (wave-uniform)
        const Region R0 = tile_region(g, tile, 0), R1 = tile_region(g, tile, 1);
        const int x = R0.x0 + lane, rows = R0.y1 - R0.y0 + 1;
        const bool col = x <= R0.x1;
        const double *src = xS + (size_t)u * fs0 + (size_t)R0.y0 * w0 + x;
        double xs[CT_H];
#pragma unroll
        for (int j = 0; j < CT_H; ++j) xs[j] = (col && j < rows) ? src[(size_t)j * w0] : 0.0;
        chain_to_level1(g, tile, xL + (size_t)u * fsL, lds);
        if (col) {
            double v[CT_H];
            level0_rows<CT_H>(g, R0, R1, lds, x, 0, v);
            double *dst = cS + (size_t)u * fs0 + (size_t)R0.y0 * w0 + x;
#pragma unroll
            for (int j = 0; j < CT_H; ++j)
                if (j < rows) dst[(size_t)j * w0] = xs[j] - v[j];
        }
        __syncthreads();
    }
}

}  // namespace rm
