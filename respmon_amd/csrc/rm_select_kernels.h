// respmon_amd/csrc/rm_select_kernels.h -- behind the bounds: which (tile, frame) pairs need their full-resolution values, their
// evaluation, the exact min / max / top and the masked time sum over the value store (transforms.py:184-192, base.py:562), with the
// plain forms on a materialised array: kernels of rm_collapse_eval.hip, rm_collapse_sum.hip and rm_calibrate.hip.
#pragma once
#include "rm_kernels.h"

namespace rm {

// exclusive prefix sum over the 256 threads of a workgroup (thread order); s_wave: 4 words of LDS.  total = sum over all threads.
__device__ __forceinline__ unsigned long long block_excl_scan_256(unsigned long long v, unsigned long long *s_wave, unsigned long long &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const unsigned long long c = s_wave[w]; base += (w < wave) ? c : 0; tot += c; }
    total = tot;
    return base + inc - v;
}

// which pairs need their full-resolution values:
//   C: may hold raw.max() or raw.min()                        -> evaluated for the exact min/max      (list_a)
//   D: may hold a value below top (lo - margin < top_ub)      -> values kept for the masked sum       (list_b unless also C)
// Pairs are [u][tile] over the UNIQUE frames u < Th (sym_frames).  A workgroup takes SEL_TILES adjacent tiles (16 lanes = one
// 128-byte row of bounds) and a chunk of SEL_PH x SEL_U unique frames; thread (tile, phase) owns the frames phase, phase + 16, ...
// of its tile, whose bound loads are issued together (the kernel is latency bound).  Everything the workgroup hands out -- value
// store slots, list positions -- is counted in LDS (one block-wide prefix sum in (tile, phase) order over three packed 20-bit
// counts) and reserved with ONE returning atomic per counter, so a tile's kept frames get consecutive slots.
// sel_cnt[tile] counts the kept pairs of a tile among this rank's frames (zeroed by the bounds kernel that ran before); the
// chunk that adds the first ones appends the tile to heavy[]: k_masked_sum_tiles gives those tiles to its worker workgroups and
// finishes every other tile with a constant fill.
// A frame shard [t0, t1) of the T-frame buffer owns unique frame u when it holds t = u or t = T - u (sym_in_range).
constexpr int SEL_TILES = 16, SEL_PH = 16, SEL_U = 9;   // 16 x 9 = 144 unique frames per chunk: one chunk at T = 256
RM_KERNEL __launch_bounds__(256) void k_select_pairs(const double *lo, const double *hi, int ntiles, int Th, int T, int t0, int t1,
                                                      CollapseState *st, unsigned int *list_a, unsigned int *list_b, int *slot_of,
                                                      int no_prune, double thr, int *sel_cnt, unsigned int *heavy)
{
    RM_TRACE_SCOPE(4);
    __shared__ unsigned long long s_cnt[256], s_off[257], s_wave[4];
    __shared__ unsigned int s_base[3];
    const int ti = threadIdx.x & (SEL_TILES - 1), ph = threadIdx.x / SEL_TILES;
    const int tile = blockIdx.x * SEL_TILES + ti;
    const int u0 = blockIdx.y * (SEL_PH * SEL_U) + ph;
    // the pairs' bounds first: nothing below depends on them until the comparisons
    double l[SEL_U], h[SEL_U];
    bool mine[SEL_U];
#pragma unroll
    for (int k = 0; k < SEL_U; ++k) {
        const int u = u0 + SEL_PH * k;
        mine[k] = tile < ntiles && u < Th && sym_in_range(u, T, t0, t1);
        const size_t i = (size_t)u * ntiles + tile;
        l[k] = mine[k] ? lo[i] : 0.0;
        h[k] = mine[k] ? hi[i] : 0.0;
    }
    // margin and the bounds-only upper bound of top = max - (max - min) * thr (increasing in max and min
    // for 0 <= thr <= 1); every thread derives them from the reduced bounds
    const unsigned long long k_lb_max = fold_max_keys(st->lb_max_keys, st->lb_max_key), k_ub_min = fold_min_keys(st->ub_min_keys, st->ub_min_key);
    const unsigned long long k_ub_max = fold_max_keys(st->ub_max_keys, st->ub_max_key), k_lb_min = fold_min_keys(st->lb_min_keys, st->lb_min_key);
    double lb_max = f64_unkey(k_lb_max), ub_min = f64_unkey(k_ub_min);
    const double ub_max = f64_unkey(k_ub_max), lb_min = f64_unkey(k_lb_min);
    const double aa = ub_max < 0 ? -ub_max : ub_max, bb = lb_min < 0 ? -lb_min : lb_min;
    const double m = PRUNE_REL_MARGIN * (aa > bb ? aa : bb);
    {   // true raw values (lattice samples) bound raw.min() from above and raw.max() from below far better than the tile bounds
        const unsigned long long k_smn = fold_min_keys(st->smp_min_keys, ~0ull), k_smx = fold_max_keys(st->smp_max_keys, 0ull);
        if (k_smn != ~0ull) {
            const double s_mn = f64_unkey(k_smn) + 2 * m, s_mx = f64_unkey(k_smx) - 2 * m;
            ub_min = (s_mn < ub_min) ? s_mn : ub_min;
            lb_max = (s_mx > lb_max) ? s_mx : lb_max;
        }
    }
    const double mx_ = ub_max + m, mn_ = ub_min + m;
    const double top_ub = (mx_ - (mx_ - mn_) * thr) + m;
    // a threshold that is not finite (an infinite or NaN bound, or a value range that overflows float64) proves nothing: no pair is
    // pruned on it -- the call is evaluated as with RM_FLAG_NO_PRUNE.  (The bounds kernels keep their bounds finite; this is the second
    // line of defence: a bound kernel with that flaw costs speed, not correctness.)  The sums see the same verdict: a NaN top_ub and margin.
    const bool thr_finite = __builtin_isfinite(m) && __builtin_isfinite(top_ub) && __builtin_isfinite(lb_max) && __builtin_isfinite(ub_min);
    if (!thr_finite) no_prune = 1;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        st->margin = thr_finite ? m : __builtin_nan("");
        st->top_ub = thr_finite ? top_ub : __builtin_nan("");
    }
    unsigned int fC = 0, fD = 0;   // bit k: pair k is C / D
    unsigned long long cnt = 0;    // D | A << 20 | B << 40
#pragma unroll
    for (int k = 0; k < SEL_U; ++k) {
        if (!mine[k]) continue;
        const bool isC = no_prune || !(h[k] + m < lb_max - m) || !(l[k] - m > ub_min + m);
        const bool isD = no_prune || (l[k] - m < top_ub);
        fC |= (isC ? 1u : 0u) << k; fD |= (isD ? 1u : 0u) << k;
        cnt += (isD ? 1ull : 0ull) + (isC ? 1ull << 20 : 0ull) + ((isD && !isC) ? 1ull << 40 : 0ull);
    }
    // prefix sums in (tile, phase) order: thread j of the scan stands for tile j / 16, phase j % 16
    s_cnt[ti * SEL_PH + ph] = cnt;
    __syncthreads();
    unsigned long long total = 0;
    const unsigned long long ex = block_excl_scan_256(s_cnt[threadIdx.x], s_wave, total);
    s_off[threadIdx.x] = ex;
    if (threadIdx.x == 0) s_off[256] = total;
    if (threadIdx.x < 3) {   // the three reservations by three lanes: ONE round trip instead of three in a row (every thread holds `total`)
        const unsigned int tot = threadIdx.x == 0 ? (unsigned)(total & 0xfffffu) : threadIdx.x == 1 ? (unsigned)((total >> 20) & 0xfffffu) : (unsigned)(total >> 40);
        unsigned int *ctr = threadIdx.x == 0 ? &st->n_slots : threadIdx.x == 1 ? &st->n_list_a : &st->n_list_b;
        s_base[threadIdx.x] = tot ? atomicAdd(ctr, tot) : 0u;
    }
    __syncthreads();
    const unsigned long long mo = s_off[ti * SEL_PH + ph];
    unsigned int oD = s_base[0] + (unsigned)(mo & 0xfffffu), oA = s_base[1] + (unsigned)((mo >> 20) & 0xfffffu), oB = s_base[2] + (unsigned)(mo >> 40);
    bool new_heavy = false;           // this chunk adds the tile's first kept pairs
    if (ph == 0 && tile < ntiles) {   // kept pairs of this tile in this chunk
        const unsigned int tot = (unsigned)((s_off[(ti + 1) * SEL_PH] - s_off[ti * SEL_PH]) & 0xfffffu);
        new_heavy = tot && atomicAdd(&sel_cnt[tile], (int)tot) == 0;
    }
    if (threadIdx.x < 64) {   // (phase 0 = lanes 0 .. 15 of wave 0) ONE reservation on n_heavy for the workgroup's new tiles: at 4K x 512 every
                              // tile of a noisy stream is heavy, and 8 100 returning atomics on one address were most of the kernel's 58 us
        const unsigned long long mk = __ballot(new_heavy);
        if (mk) {
            const int lane = threadIdx.x, first = __builtin_ctzll(mk);
            unsigned int base = 0;
            if (lane == first) base = atomicAdd(&st->n_heavy, (unsigned)__popcll(mk));
            base = (unsigned)__shfl((int)base, first);
            if (new_heavy) heavy[base + __popcll(mk & ((1ull << lane) - 1ull))] = (unsigned)tile;
        }
    }
#pragma unroll
    for (int k = 0; k < SEL_U; ++k) {
        if (!mine[k]) continue;
        const int u = u0 + SEL_PH * k;
        const unsigned int i = (unsigned)u * (unsigned)ntiles + (unsigned)tile;
        const bool isC = (fC >> k) & 1u, isD = (fD >> k) & 1u;
        slot_of[slot_index(u, tile, Th)] = isD ? (int)oD : SLOT_PRUNED;
        if (isD) ++oD;
        if (isC) list_a[oA++] = i;
        else if (isD) list_b[oB++] = i;
    }
}

// the one evaluation pass: full-resolution values of every listed (unique frame, tile) pair, once.
// Exact raw.min()/raw.max() (transforms.py:185,187) come from here (list_a); on the sparse path the values of the pairs that can
// fall below `top` (list_a's kept pairs and all of list_b) are parked in their slot of `store` ([slot][row][lane], coalesced) for
// the masked time sum.  On the dense path (sum_is_dense) list_b is not touched and nothing is stored.
RM_KERNEL __launch_bounds__(64) void k_eval_pairs(const double *cS, ChainGeom g, int ntiles, const unsigned int *list_a, const unsigned int *list_b,
                                                   int *slot_of, CollapseState *st, double *store, SumPlan sp, int Th)
{
    RM_TRACE_SCOPE(5);
    HIP_DYNAMIC_SHARED(double, lds)
    // the first list entry is requested together with the list lengths (the list buffer is valid memory whatever they turn out
    // to be): one memory round trip less at the head of every workgroup's dependent chain
    const unsigned first_idx = list_a[blockIdx.x];
    const unsigned nA = st->n_list_a, nB = st->n_list_b;
    const bool dense = sum_is_dense(st, sp);
    const unsigned n = nA + (dense ? 0u : nB);
    const int lane = threadIdx.x;
    const double inf = __builtin_huge_val();
    const double top_ub = st->top_ub;   // upper bound of `top` from the tile bounds (k_select_pairs)
    double mn = inf, mx = -inf;
    for (unsigned c = blockIdx.x; c < n; c += gridDim.x) {
        RM_TRACE_MARK(5, 0);
        const unsigned raw_idx = c < nA ? (c == blockIdx.x ? first_idx : list_a[c]) : list_b[c - nA];
        const unsigned idx = (unsigned)uniform((int)raw_idx);   // wave-uniform: the tile geometry stays in scalar registers
        const int u = idx / ntiles, tile = idx - u * ntiles;
        const int slot = dense ? SLOT_PRUNED : uniform(slot_of[slot_index(u, tile, Th)]);   // (needed after the chain: requested now)
        const Region R0 = tile_region(g, tile, 0), R1 = tile_region(g, tile, 1);
        RM_TRACE_MARK(5, 1);
        chain_to_level1(g, tile, cS + (size_t)u * g.h[g.S] * g.w[g.S], lds);
        RM_TRACE_MARK(5, 6);
        int x = R0.x0 + lane;
        double pmn = inf;   // minimum of this pair's tile
        double v[CT_H];
        const int rows = R0.y1 - R0.y0 + 1;
        if (x <= R0.x1) {
            level0_rows<CT_H>(g, R0, R1, lds, x, 0, v);
#pragma unroll
            for (int j = 0; j < CT_H; ++j)
                if (j < rows) { pmn = (v[j] < pmn) ? v[j] : pmn; mx = (v[j] > mx) ? v[j] : mx; }
        }
        mn = (pmn < mn) ? pmn : mn;
        RM_TRACE_MARK(5, 7);
        if (slot != SLOT_PRUNED) {   // wave-uniform
            pmn = wave_min(pmn);
            // nothing of this tile can fall below top (top <= top_ub): every pixel adds `min`, exactly like a pruned pair --
            // no values to park, and the sum pass never sees the frame
            if (__builtin_isfinite(top_ub) && pmn >= top_ub) {
                if (lane == 0) slot_of[slot_index(u, tile, Th)] = SLOT_PRUNED;
            } else if (x <= R0.x1) {
                double *d = store + (size_t)slot * (CT_H * CT_W) + lane;
#pragma unroll
                for (int j = 0; j < CT_H; ++j) d[j * CT_W] = v[j];
            }
        }
        RM_TRACE_MARK(5, 8);
        __syncthreads();
    }
    mn = wave_min(mn); mx = wave_max(mx);
    RM_TRACE_MARK(5, 9);
    if (lane == 0 && blockIdx.x < n) {
        // striped, and skipped when they cannot change the result
        const unsigned long long kmn = f64_key(mn), kmx = f64_key(mx);
        const int sp_ = blockIdx.x & (NSTRIPE - 1);
        striped_min_max(st->min_keys, st->max_keys, sp_, kmn, kmx);
    }
}

// transforms.py:184-189: min, max, top = max - (max - min) * threshold
RM_KERNEL __launch_bounds__(NSTRIPE) void k_finish_minmax(CollapseState *st, double threshold)
{
    const unsigned long long kmn = fold_min_keys(st->min_keys, st->min_key), kmx = fold_max_keys(st->max_keys, st->max_key);
    if (threadIdx.x != 0) return;
    double mn = f64_unkey(kmn), mx = f64_unkey(kmx);
    st->min_val = mn; st->max_val = mx;
    st->top = mx - (mx - mn) * threshold;
}

// frame-sharded calibration: the exact extrema of this rank's frames leave as {-min, max} (one all-reduce(MAX)
// serves both) and the global pair comes back the same way
RM_KERNEL __launch_bounds__(NSTRIPE) void k_export_minmax(const CollapseState *st, double *negmin_max)
{
    const double inf = __builtin_huge_val();
    const unsigned long long kmn = fold_min_keys(st->min_keys, st->min_key), kmx = fold_max_keys(st->max_keys, st->max_key);
    if (threadIdx.x != 0) return;
    negmin_max[0] = (kmn == ~0ull) ? -inf : -f64_unkey(kmn);
    negmin_max[1] = (kmx == 0ull) ? -inf : f64_unkey(kmx);
}
RM_KERNEL __launch_bounds__(NSTRIPE) void k_import_minmax(CollapseState *st, const double *negmin_max)
{
    st->min_keys[threadIdx.x] = ~0ull; st->max_keys[threadIdx.x] = 0ull;   // the global pair replaces this rank's stripes
    if (threadIdx.x != 0) return;
    st->min_key = f64_key(-negmin_max[0]);
    st->max_key = f64_key(negmin_max[1]);
}

// pass D: heat_sum[y,x] = sum_t (raw >= top ? min : raw), sequential in t (np.average order, base.py:562).
// Pruned pairs add `min`; kept pairs read their values back from `store`.
//
// One launch of `nworkers` 256-thread workgroups:
//   * WORKER items.  Item i is (heavy[i / MS_Q], row group i % MS_Q): the tile's ordered list of kept frames is compacted by
//     ballot / popcount (every worker of the tile repeats that cheap, parallel step), then thread (wave, lane) owns pixel
//     (row MS_RQ * q + wave, column lane) and walks the kept frames in batches of MS_B loads issued one batch ahead.  The
//     longest dependent chain of the launch is therefore ceil(kept / MS_B) round trips of ONE tile row group, not
//     256 / 6 of a whole tile (the earlier form: one 256-thread workgroup per tile, 4 rows per lane, 6-frame batches --
//     its heaviest tile alone took 29 us and every empty tile 8-10 us in three rounds).
//   * FILL.  A tile without a kept pair (sel_cnt[tile] == 0: 94 % of the tiles of the synthetic 1080p stream) is one
//     constant -- T sequential additions of `min` -- computed once per workgroup and stored into every such tile of its
//     share.  The workgroups that found no worker item do the filling (they are free at once; separate fill workgroups
//     queued behind the workers' registers and started 5-14 us late); when every workgroup has items, all of them fill
//     after their items.
// Dynamic LDS: s_kt[T] and s_ks[T], the tile's kept frames in order and their value store slots.
// Frames are walked in time order t = t_first .. t_end - 1 (np.average's order); frame t's pair is that of its unique frame
// sym_frame(t, T).  On the dense path (sum_is_dense) the kernel returns at once: k_dense_sum takes the sum.
constexpr int MS_Q = 4;              // row groups (worker items) per heavy tile
constexpr int MS_RQ = CT_H / MS_Q;   // rows per worker == waves per workgroup
#ifndef RM_MS_B
#define RM_MS_B 16
#endif
constexpr int MS_B = RM_MS_B;        // kept frames per batch (32: 220 VGPRs, two waves per SIMD -- measured 32 us against 20)

RM_KERNEL __launch_bounds__(64 * MS_RQ) void k_masked_sum_tiles(int t_first, int t_end, int T, int ntiles, int W0, int H0,
                                                          const int *slot_of, const double *store,
                                                          CollapseState *st, double threshold, double *heat_sum, int avg_T,
                                                          int *tile_nkept, const int *sel_cnt, const unsigned int *heavy, int nworkers,
                                                          SumPlan sp, int *unserved_host)
{
    RM_TRACE_SCOPE(6);
    HIP_DYNAMIC_SHARED(int, s_kt)     // kept frames of the tile, in order; then their slots
    int *s_ks = s_kt + T;
    __shared__ int s_wcnt[MS_RQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (W0 + CT_W - 1) / CT_W;
    // everything that does not depend on the state is requested before it: the tile of this workgroup's first item and its
    // first slot_of column (speculatively: heavy[] and slot_of[] are valid memory whatever n_heavy turns out to be)
    const int tile0 = (int)(heavy[blockIdx.x / MS_Q] % (unsigned)ntiles);
    int slot0 = SLOT_PRUNED;
    if (t_first + tid < t_end) slot0 = slot_of[slot_index(sym_frame(t_first + tid, T), tile0, sym_frames(T))];
    const int nitems = (int)st->n_heavy * MS_Q;
    if (unserved_host && blockIdx.x == 0 && threadIdx.x == 0) unserved_host[1] = (int)st->n_slots;   // (pinned: how many pairs this call's selection kept -- rm_locate's refine_hint)
    if (sum_is_dense(st, sp)) {   // (uniform over the grid: k_dense_sum takes the sum)
        // unserved_host (pinned, nullable): no dense kernel follows on the stream -- the caller synchronises anyway and enqueues it
        // itself when it finds this word set (rm_locate: the rare value-store overflow costs the common case no launch)
        if (unserved_host && blockIdx.x == 0 && tid == 0) *unserved_host = 1;
        return;
    }
    // transforms.py:184-189: min, max, top = max - (max - min) * threshold
    const double min_val = f64_unkey(fold_min_keys(st->min_keys, st->min_key)), max_val = f64_unkey(fold_max_keys(st->max_keys, st->max_key));
    const double top = max_val - (max_val - min_val) * threshold;
    RM_TRACE_MARK(6, 0);
    if (blockIdx.x == 0 && tid == 0) {
        st->min_val = min_val; st->max_val = max_val; st->top = top;
    }
    // avg_T > 0 (the whole buffer is summed here): write np.average = sum / T (base.py:562) and reduce the
    // heatmap's min / max for the normalisation (base.py:563) on the way out
    const double cnt = (double)avg_T;
    for (int item = (int)blockIdx.x; item < nitems; item += nworkers) {
        const bool first = item == (int)blockIdx.x;
        const int tile = first ? tile0 : (int)heavy[item / MS_Q], q = item % MS_Q;
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        // frames [t_first, t_end): the whole buffer, or this rank's frame shard (partial time sums add up across ranks).
        // Ordered compaction of the frames that are not pruned (by the selection, or by the evaluation pass when the whole
        // tile turned out >= top_ub): ballot + prefix popcount, 256 frames per round.
        int nkept = 0;
        for (int c0 = t_first; c0 < t_end; c0 += 64 * MS_RQ) {
            const int t = c0 + tid;
            int slot = SLOT_PRUNED;
            if (first && c0 == t_first) slot = slot0;
            else if (t < t_end) slot = slot_of[slot_index(sym_frame(t, T), tile, sym_frames(T))];
            const bool kept = slot != SLOT_PRUNED;
            const unsigned long long m = __ballot(kept);
            if (lane == 0) s_wcnt[wave] = __popcll(m);
            __syncthreads();
            int off = nkept, tot = 0;
#pragma unroll
            for (int w = 0; w < MS_RQ; ++w) { const int c = s_wcnt[w]; off += (w < wave) ? c : 0; tot += c; }
            if (kept) { const int pos = off + __popcll(m & ((1ull << lane) - 1ull)); s_kt[pos] = t; s_ks[pos] = slot; }
            nkept += tot;
            __syncthreads();
        }
        if (tid == 0 && q == 0 && tile_nkept) tile_nkept[tile] = nkept;   // 0: every pixel of the tile ends up as the same constant
        RM_TRACE_MARK(6, 1);
        const int x = tx * CT_W + lane;
        const int row = q * MS_RQ + wave, y = ty * CT_H + row;
        const bool active = x < W0 && y < H0;
        const double *mine = store + (size_t)row * CT_W + lane;   // + slot * 1024: this pixel in the pair parked in `slot`
        double acc = 0.0;
        // a batch = MS_B kept frames: their frame numbers and (one batch ahead) values sit in registers, so the serial
        // part below touches neither LDS nor memory (per-frame LDS look-ups were 2/3 of the heaviest worker's time)
        double nxt[MS_B];
        int ktn[MS_B];
#pragma unroll
        for (int b = 0; b < MS_B; ++b) nxt[b] = 0.0;
        auto fetch = [&](int ib) __attribute__((always_inline)) {
#pragma unroll
            for (int b = 0; b < MS_B; ++b) {
                const int i = ib + b;
                const bool ok = i < nkept;
                ktn[b] = ok ? s_kt[i] : t_end;
                if (ok && active) nxt[b] = mine[(size_t)s_ks[i] * (CT_H * CT_W)];
            }
        };
        fetch(0);
        RM_TRACE_MARK(6, 2);
        int t_done = t_first;
        for (int ib = 0; ib < nkept; ib += MS_B) {
            double cur[MS_B];
            int kt[MS_B];
#pragma unroll
            for (int b = 0; b < MS_B; ++b) { cur[b] = nxt[b]; kt[b] = ktn[b]; }
            fetch(ib + MS_B);
#pragma unroll
            for (int b = 0; b < MS_B; ++b) {
                if (ib + b < nkept) {
                    const int t_stop = uniform(kt[b]);     // frames [t_done, t_stop) are pruned
                    for (int t = t_done; t < t_stop; ++t) acc = acc + min_val;
                    if (active) acc = acc + ((cur[b] >= top) ? min_val : cur[b]);
                    t_done = t_stop + 1;
                }
            }
            RM_TRACE_MARK(6, 3 + ib / MS_B);
        }
        for (int t = t_done; t < t_end; ++t) acc = acc + min_val;
        RM_TRACE_MARK(6, 12);
        double hmn = __builtin_huge_val(), hmx = -__builtin_huge_val();
        if (active) {
            const double v = avg_T > 0 ? acc / cnt : acc;
            heat_sum[(size_t)y * W0 + x] = v;
            hmn = v; hmx = v;
        }
        if (avg_T > 0) {
            block_minmax(hmn, hmx);
            if (tid == 0) {
                const unsigned long long kmn = f64_key(hmn), kmx = f64_key(hmx);
                const int sp = blockIdx.x & (NSTRIPE - 1);
                striped_min_max(st->heat_min_keys, st->heat_max_keys, sp, kmn, kmx);
            }
        }
        RM_TRACE_MARK(6, 13);
        __syncthreads();   // s_kt is rewritten by the next item
    }
    // FILL: by the workgroups without items when there are any, by every workgroup otherwise
    const int idle = nworkers - min(nitems, nworkers);
    const int nfill = idle > 0 ? idle : nworkers;
    const int fid = idle > 0 ? (int)blockIdx.x - nitems : (int)blockIdx.x;
    if (fid < 0) return;
    double lead = 0.0;
    for (int t = t_first; t < t_end; ++t) lead = lead + min_val;
    const double v = avg_T > 0 ? lead / cnt : lead;
    bool any = false;
    constexpr int FU = 4;    // tiles whose kept-pair counts are requested together
    for (int base = fid; base < ntiles; base += FU * nfill) {
        int cntk[FU];
#pragma unroll
        for (int k = 0; k < FU; ++k) { const int tile = base + k * nfill; cntk[k] = tile < ntiles ? sel_cnt[tile] : 1; }
#pragma unroll
        for (int k = 0; k < FU; ++k) {
            const int tile = base + k * nfill;
            if (cntk[k] != 0) continue;               // past the end, or a worker sums this tile
            any = true;
            const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
            const int x = tx * CT_W + lane, y0 = ty * CT_H;
            if (x < W0) {
#pragma unroll
                for (int j = 0; j < CT_H / MS_RQ; ++j) {
                    const int y = y0 + wave * (CT_H / MS_RQ) + j;
                    if (y < H0) heat_sum[(size_t)y * W0 + x] = v;
                }
            }
            if (tid == 0 && tile_nkept) tile_nkept[tile] = 0;     // 0: every pixel of the tile is the same constant
        }
    }
    if (any && tid == 0 && avg_T > 0) {
        const unsigned long long kv = f64_key(v);
        const int sp = blockIdx.x & (NSTRIPE - 1);
        striped_min_max(st->heat_min_keys, st->heat_max_keys, sp, kv, kv);
    }
}

// ----------------------------------------------------------------------------------------
// plain (materialised) forms: global min/max, mask, time sum  -- transforms.py:184-192, base.py:562
// ----------------------------------------------------------------------------------------
RM_KERNEL __launch_bounds__(256) void k_minmax_plain(const double *a, size_t n, CollapseState *st)
{
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        double v = a[i];
        mn = (v < mn) ? v : mn;
        mx = (v > mx) ? v : mx;
    }
    block_minmax(mn, mx);
    if (threadIdx.x == 0) {
        atomicMin(&st->min_key, f64_key(mn));
        atomicMax(&st->max_key, f64_key(mx));
    }
}

RM_KERNEL __launch_bounds__(256) void k_mask_plain(const double *raw, size_t n, const CollapseState *st, double *masked)
{
    const double top = st->top, mn = st->min_val;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        double v = raw[i];
        masked[i] = (v >= top) ? mn : v;
    }
}

// heat_sum[p] = sum_t (raw[t,p] >= top ? min : raw[t,p])   (sequential in t); raw holds the sym_frames(T) unique frames
RM_KERNEL __launch_bounds__(256) void k_masked_sum_plain(const double *raw, int T, size_t npix, const CollapseState *st,
                                                          double *heat_sum)
{
    size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const double top = st->top, mn = st->min_val;
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
        double v = raw[(size_t)sym_frame(t, T) * npix + p];
        acc = acc + ((v >= top) ? mn : v);
    }
    heat_sum[p] = acc;
}

// frames T/2+1 .. T-1 of a [T, npix] array from their mirror images (sym_frame): dst[t] = dst[T - t]
RM_KERNEL __launch_bounds__(256) void k_mirror_frames(double *a, int T, size_t npix)
{
    const int t = sym_frames(T) + (int)blockIdx.y;   // t in (T/2, T)
    const double *src = a + (size_t)(T - t) * npix;
    double *dst = a + (size_t)t * npix;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

}  // namespace rm
