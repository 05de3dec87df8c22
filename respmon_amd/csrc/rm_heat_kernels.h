// respmon_amd/csrc/rm_heat_kernels.h -- heatmap -> thresholded uint8 image for the ROI stage (base.py:562-566) and the sparse heatmap
// exchange between GPUs: kernels of rm_roi.hip and rm_calibrate.hip.
#pragma once
#include "rm_kernels.h"

namespace rm {

// ----------------------------------------------------------------------------------------
// base.py:562-566: avg = sum / T ; normalise ; float_to_uint8 ; threshold
// ----------------------------------------------------------------------------------------
RM_KERNEL __launch_bounds__(256) void k_heat_avg_minmax(const double *heat_sum, size_t npix, int T, double *heat,
                                                         CollapseState *st)
{
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    const double cnt = (double)T;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        double v = heat_sum[i] / cnt;
        heat[i] = v;
        mn = (v < mn) ? v : mn;
        mx = (v > mx) ? v : mx;
    }
    block_minmax(mn, mx);
    if (threadIdx.x == 0) {
        atomicMin(&st->heat_min_key, f64_key(mn));
        atomicMax(&st->heat_max_key, f64_key(mx));
    }
}

// min/max of an existing heatmap (rm_heatmap_to_roi entry point)
// reset of the heatmap extrema in the state (in front of k_heat_minmax / k_heat_avg_minmax / a sum kernel that reduces them)
RM_KERNEL __launch_bounds__(NSTRIPE) void k_heat_state_init(CollapseState *st)
{
    st->heat_min_keys[threadIdx.x] = ~0ull; st->heat_max_keys[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) { st->heat_min_key = ~0ull; st->heat_max_key = 0ull; }
}

RM_KERNEL __launch_bounds__(256) void k_heat_minmax(const double *heat, size_t npix, CollapseState *st)
{
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        double v = heat[i];
        mn = (v < mn) ? v : mn;
        mx = (v > mx) ? v : mx;
    }
    block_minmax(mn, mx);
    if (threadIdx.x == 0) {
        atomicMin(&st->heat_min_key, f64_key(mn));
        atomicMax(&st->heat_max_key, f64_key(mx));
    }
}

// `bits` receives the thresholded image bit-packed (bit p & 63 of word p >> 6 = pixel p, row-major): 1/8 of a byte per
// pixel, stored straight into pinned, device-mapped host memory.  `row_any[y]` (pinned bytes) is set for every row that holds
// foreground: the host contour stage then reads only those rows of `bits` -- the breathing region covers ~1/5 of a 1080p frame,
// and reading memory the device has just written (lines no host cache holds) was most of that stage.  The host zeroes the
// flags AND the rows it read after use, so the image is all-zero between calls and the kernel stores only the words that
// have a bit set (~12 KB instead of 259 KB over PCIe: the launch's end-of-kernel flush of host-memory writes shrinks with it).  (Tried and dropped: a sparse list of the non-zero words with a `done` word the host spins on instead of the
// runtime's completion query -- the kernel's own hand-off cost 14 us more, and a stream the runtime never sees complete
// makes the NEXT launch ~100 us slower.)
struct alignas(16) CclBox { int minx, maxx, maxy, cnt; };   // bounding box of a labelled component (rm_ccl.h), indexed by its root; cnt: 2 * pixels - cracks (rm_ccl.h ccl_piece_2n_minus_p)

// tile_const (nullable; needs W % 64 == 0): tile_nkept of the sum kernel that wrote `heat` -- 0 for a 64 x 16 tile every pixel of which
// is the same constant (96 % of the tiles of the synthetic 1080p stream): such a word takes its ONE value from a wave-uniform load
// and the 16.6 MB heatmap is read only where it varies
RM_KERNEL __launch_bounds__(256) void k_heat_to_u8(const double *heat, size_t npix, int W, const CollapseState *st,
                                                    int threshold, uint8_t *avg_u8, uint8_t *binary,
                                                    unsigned long long *bits, uint8_t *row_any,
                                                    unsigned long long *bits_dev, int *ccl_label, CclBox *ccl_box,
                                                    unsigned int *ccl_counters, const int *tile_const = nullptr)
{
    RM_TRACE_SCOPE(7);
    if (ccl_counters && blockIdx.x == 0 && threadIdx.x == 0) ccl_counters[0] = 0;   // k_ccl_bbox reserves the root list's slots there
    const int lane = threadIdx.x & 63;
    // `base` is the first pixel of this wave's 64-pixel group: the same for all lanes, so the ballot is complete.
    // HU groups per trip: their heat values are requested together and BEFORE the extrema are folded from the state
    constexpr int HU = 4;
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t first = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u);
    double hv[HU];
    const int tiles_x = (W + CT_W - 1) / CT_W;
    auto fetch = [&](size_t base0) __attribute__((always_inline)) {
        if (tile_const) {
            // the word's tile flag and its first value (both wave-uniform), then the 64 values only where the tile is not a constant
            int cst[HU];
            double h0[HU];
#pragma unroll
            for (int k = 0; k < HU; ++k) {
                const size_t base = base0 + k * stride;
                const size_t bc = base < npix ? base : 0;
                const int y = (int)(bc / (size_t)W), x = (int)(bc - (size_t)y * W);
                cst[k] = tile_const[(y / CT_H) * tiles_x + x / CT_W];
                h0[k] = heat[bc];
            }
#pragma unroll
            for (int k = 0; k < HU; ++k) {
                const size_t i = base0 + k * stride + lane;
                hv[k] = (cst[k] != 0 && i < npix) ? heat[i] : h0[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < HU; ++k) { const size_t i = base0 + k * stride + lane; hv[k] = i < npix ? heat[i] : 0.0; }
        }
    };
    fetch(first);
    const double mn = f64_unkey(fold_min_keys(st->heat_min_keys, st->heat_min_key));
    const double mx = f64_unkey(fold_max_keys(st->heat_max_keys, st->heat_max_key));
    const double range = mx - mn;
    for (size_t base0 = first; base0 < npix; base0 += HU * stride) {
        if (base0 != first) fetch(base0);
#pragma unroll
        for (int k = 0; k < HU; ++k) {
            const size_t base = base0 + k * stride, i = base + lane;
            if (base >= npix) break;                          // wave-uniform
            uint8_t b = 0;
            if (i < npix) {
                double nrm = (hv[k] - mn) / range;            // base.py:563 (NaN when the heatmap is flat)
                uint8_t u = f64_to_u8_trunc(nrm * 255);       // transforms.py:26-29
                b = (u > threshold) ? 255 : 0;                // cv2.threshold THRESH_BINARY, base.py:566
                if (avg_u8) avg_u8[i] = u;
                if (binary) binary[i] = b;
            }
            const unsigned long long m = __ballot(b != 0);
            if (bits_dev) {   // device labelling of the components (rm_ccl.h) follows: every word, and the start state of its
                              // union-find -- the ballot IS the pixel's word, so no separate pass has to read it back
                if (lane == 0) bits_dev[base >> 6] = m;
                if (b && ccl_label) {   // (null: k_ccl_tile builds the start state itself, in LDS)
                    // label = first pixel of the run of ones that ends here (inside this word, not crossing the row start).  Only
                    // such a first pixel can end up a root, and only it carries a box: that of its piece of the run
                    const unsigned long long zeros_below = ~m & ((1ull << lane) - 1ull);
                    int run0 = zeros_below ? 64 - __builtin_clzll(zeros_below) : 0;
                    const unsigned int y = (unsigned int)i / (unsigned int)W, x = (unsigned int)i - y * (unsigned int)W;
                    if (lane - run0 > (int)x) run0 = lane - (int)x;
                    ccl_label[i] = (int)i - (lane - run0);
                    if (run0 == lane) {
                        const unsigned long long zeros_above = ~(m >> lane);              // bit k: pixel i + k is background (or past the word)
                        int len = zeros_above ? __builtin_ctzll(zeros_above) : 64;        // (lane 0 of a full word: 64 ones)
                        if (len > 64 - lane) len = 64 - lane;
                        if (len > W - (int)x) len = W - (int)x;                           // the row ends inside the word
                        CclBox e; e.minx = (int)x; e.maxx = (int)x + len - 1; e.maxy = (int)y; e.cnt = 0;
                        ccl_box[i] = e;
                    }
                }
            }
            if (lane == 0 && bits && m) {   // the host keeps the image all-zero between calls: only set words travel
                bits[base >> 6] = m;
                if (row_any) {   // the group may straddle row ends: flag every row it touches (a superset is fine)
                    const size_t last = (base + 63 < npix ? base + 63 : npix - 1);
                    for (size_t y = base / (size_t)W; y <= last / (size_t)W; ++y) row_any[y] = 1;
                }
            }
        }
    }
}

// The same for images whose rows are whole 64-pixel words (W % 64 == 0: 1080p, 720p, 4K), one workgroup per image row.  Beside the
// packed image the host gets ONE 8-byte record per row that holds foreground,
//     rec[y] = first | last << 16 | min(runs, 0xffff) << 32 | 1 << 48        (first / last foreground column, runs of foreground)
// so the host's one-blob rule (rm_contour.cpp simple_shape_row_records: one run per row, neighbouring runs touching => one hole-free
// 8-connected component => the ROI is the bounding box of the runs, base.py:568-575) reads H x 8 bytes instead of hunting through
// the image rows the device has just written (lines no host cache holds: ~10 us of the 48 us the GPU idles between two synchronous
// locate() calls at 1080p).  The image words still travel for the images the rule does not settle (the host then follows the
// borders as before).  Wave w of the row takes the words w, w + 4, ...; the words meet in LDS, wave 0 folds them.
constexpr int HR_MAXW = 512;   // words per row the row kernel takes (W <= 32768)
RM_KERNEL __launch_bounds__(256) void k_heat_rows_u8(const double *heat, int H, int W, const CollapseState *st, int threshold, uint8_t *avg_u8,
                                                      uint8_t *binary, unsigned long long *bits, unsigned long long *rec, const int *tile_const)
{
    RM_TRACE_SCOPE(7);
    __shared__ unsigned long long s_words[HR_MAXW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y = blockIdx.x, nw = W >> 6;
    const int tiles_x = (W + CT_W - 1) / CT_W;
    const double *row = heat + (size_t)y * W;
    constexpr int HU = 4;
    const int trow = (y / CT_H) * tiles_x;
    double hv[HU];
    auto fetch = [&](int j0) __attribute__((always_inline)) {   // words j0, j0 + 4, .. of this wave, requested together
        if (tile_const) {
            int cst[HU];
            double h0[HU];
#pragma unroll
            for (int k = 0; k < HU; ++k) {
                const int j = j0 + 4 * k, jc = j < nw ? j : 0;
                cst[k] = tile_const[trow + (jc * 64) / CT_W];
                h0[k] = row[jc * 64];
            }
#pragma unroll
            for (int k = 0; k < HU; ++k) {
                const int j = j0 + 4 * k;
                hv[k] = (cst[k] != 0 && j < nw) ? row[j * 64 + lane] : h0[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < HU; ++k) { const int j = j0 + 4 * k; hv[k] = j < nw ? row[j * 64 + lane] : 0.0; }
        }
    };
    fetch(wave);
    const double mn = f64_unkey(fold_min_keys(st->heat_min_keys, st->heat_min_key));
    const double mx = f64_unkey(fold_max_keys(st->heat_max_keys, st->heat_max_key));
    const double range = mx - mn;
    for (int j0 = wave; j0 < nw; j0 += 4 * HU) {
        if (j0 != wave) fetch(j0);
#pragma unroll
        for (int k = 0; k < HU; ++k) {
            const int j = j0 + 4 * k;
            if (j >= nw) break;                               // wave-uniform
            const size_t i = (size_t)y * W + (size_t)j * 64 + lane;
            const double nrm = (hv[k] - mn) / range;          // base.py:563 (NaN when the heatmap is flat)
            const uint8_t u = f64_to_u8_trunc(nrm * 255);     // transforms.py:26-29
            const uint8_t b = (u > threshold) ? 255 : 0;      // cv2.threshold THRESH_BINARY, base.py:566
            if (avg_u8) avg_u8[i] = u;
            if (binary) binary[i] = b;
            const unsigned long long m = __ballot(b != 0);
            if (lane == 0) {
                s_words[j] = m;
                if (m) bits[i >> 6] = m;                      // the host keeps the image all-zero between calls: only set words travel
            }
        }
    }
    __syncthreads();
    if (wave != 0) return;
    int first = 0x7fffffff, last = -1, runs = 0;
    for (int c = 0; c < nw; c += 64) {
        const int j = c + lane;
        const unsigned long long m = j < nw ? s_words[j] : 0ull;
        const unsigned long long prev = (j > 0 && j < nw) ? (s_words[j - 1] >> 63) : 0ull;
        if (m) {
            const int a = j * 64 + __builtin_ctzll(m), b = j * 64 + 63 - __builtin_clzll(m);
            first = a < first ? a : first;
            last = b > last ? b : last;
            runs += __popcll(m & ~((m << 1) | prev));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int f2 = __shfl_xor(first, d), l2 = __shfl_xor(last, d), r2 = __shfl_xor(runs, d);
        first = f2 < first ? f2 : first; last = l2 > last ? l2 : last; runs += r2;
    }
    if (lane == 0 && runs > 0)
        rec[y] = (unsigned long long)first | ((unsigned long long)last << 16) | ((unsigned long long)(runs > 0xffff ? 0xffff : runs) << 32) | (1ull << 48);
    (void)H;
}

// ----------------------------------------------------------------------------------------
// Sparse heatmap exchange between GPUs (one stream per GPU, dist.locate_streams).  A stream's heatmap is ONE
// constant -- the time average of `min` -- in every tile none of whose frames survived the pruning (98 % of the
// tiles on the synthetic video), so instead of all-reducing 16.6 MB per GPU over xGMI each rank sends a packet
//   header { u32 count, u32 reserved, f64 background, 2 x f64 reserved } , f64 tile index [cap] , f64 values [cap][16][64]
// (0.5 MB at cap = 64) through ONE all-gather, and every rank rebuilds  sum_r heat_r  in rank order.
// count > cap (or no pruning information) makes every rank fall back to the dense all-reduce.
// ----------------------------------------------------------------------------------------
constexpr int SP_HDR = 4;  // doubles

// background constant = the heatmap value of the first tile without kept frames (header double 1); none -> overflow.
// One wave, 64 tiles per ballot (the first tile is almost always one of them).
constexpr unsigned int SP_DENSE_ONLY = 0xffffffffu;   // header count: this rank has no sparse form, use the dense exchange
RM_KERNEL __launch_bounds__(64) void k_sparse_background(const double *heat, int W, int tiles_x, int ntiles, const int *tile_nkept,
                                                          int cap, double *packet)
{
    const int lane = threadIdx.x;
    int first = ntiles;
    for (int base = 0; base < ntiles && first == ntiles; base += 64) {
        const int i = base + lane;
        const unsigned long long m = __ballot(i < ntiles && tile_nkept[i] == 0);
        if (m) first = base + __builtin_ctzll(m);
    }
    if (lane != 0) return;
    packet[0] = 0.0; packet[1] = 0.0; packet[2] = 0.0; packet[3] = 0.0;   // header: count = 0 before k_sparse_pack counts
    if (first >= ntiles) { *reinterpret_cast<unsigned int *>(packet) = SP_DENSE_ONLY; return; }
    const int ty = first / tiles_x, tx = first - ty * tiles_x;
    packet[1] = heat[(size_t)ty * CT_H * W + (size_t)tx * CT_W];
}

// a tile travels only if one of its pixels differs from the background (a tile with kept frames whose values were
// all masked ends up as the same constant, bit for bit: the same sequence of additions of `min`)
RM_KERNEL __launch_bounds__(256) void k_sparse_pack(const double *heat, int H, int W, int tiles_x, const int *tile_nkept, int cap,
                                                     double *packet)
{
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * CT_H, x0 = tx * CT_W;
    if (tile_nkept[tile] == 0) return;
    unsigned int *count = reinterpret_cast<unsigned int *>(packet);
    if (*(volatile unsigned int *)count == SP_DENSE_ONLY) return;
    const double c = packet[1];
    double v[CT_H * CT_W / 256];
    bool differs = false;
#pragma unroll
    for (int k = 0; k < CT_H * CT_W / 256; ++k) {
        const int i = threadIdx.x + 256 * k;
        const int y = y0 + i / CT_W, x = x0 + (i & (CT_W - 1));
        const bool in = y < H && x < W;
        v[k] = in ? heat[(size_t)y * W + x] : c;
        differs = differs || (in && v[k] != c);
    }
    __shared__ unsigned int s_slot;
    __shared__ int s_any;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    if (__ballot(differs) != 0ull && (threadIdx.x & 63) == 0) s_any = 1;
    __syncthreads();
    if (!s_any) return;
    if (threadIdx.x == 0) s_slot = atomicAdd(count, 1u);
    __syncthreads();
    const unsigned int slot = s_slot;
    if (slot >= (unsigned)cap) return;   // overflow: count says so, the receiver falls back
    if (threadIdx.x == 0) packet[SP_HDR + slot] = (double)tile;
    double *dst = packet + SP_HDR + cap + (size_t)slot * (CT_H * CT_W);
#pragma unroll
    for (int k = 0; k < CT_H * CT_W / 256; ++k) dst[threadIdx.x + 256 * k] = v[k];
}

// ONE workgroup prepares the merge: map[r][tile] = slot of `tile` in rank r's packet or -1, any[tile] = 1 when some rank
// sent the tile, flag_host[0] = 1 when some rank overflowed, flag_host[1] = the largest tile count a rank needed
// (pinned host words: the caller reads them after the ROI stage's synchronisation), and the stripes the merge
// kernel reduces the fused heatmap's extrema into
RM_KERNEL __launch_bounds__(256) void k_sparse_index(const double *packets, size_t packet_doubles, int world, int cap, int ntiles,
                                                      int *map, int *any, int *flag_host, CollapseState *st, int avg_T)
{
    for (int i = threadIdx.x; i < world * ntiles; i += 256) map[i] = -1;
    for (int i = threadIdx.x; i < ntiles; i += 256) any[i] = 0;
    if (threadIdx.x < NSTRIPE) { st->heat_min_keys[threadIdx.x] = ~0ull; st->heat_max_keys[threadIdx.x] = 0ull; }
    if (threadIdx.x == 0) { st->heat_min_key = ~0ull; st->heat_max_key = 0ull; }
    __syncthreads();
    int over = 0;
    unsigned int need = 0;
    for (int r = 0; r < world; ++r) {
        const double *pk = packets + (size_t)r * packet_doubles;
        const unsigned int count = *reinterpret_cast<const unsigned int *>(pk);
        if (count != SP_DENSE_ONLY && count > need) need = count;
        if (count > (unsigned)cap) { over = 1; continue; }
        for (unsigned int j = threadIdx.x; j < count; j += 256) {
            const int tile = (int)pk[SP_HDR + j];
            if (tile >= 0 && tile < ntiles) { map[(size_t)r * ntiles + tile] = (int)j; any[tile] = 1; }
        }
    }
    if (threadIdx.x == 0) { flag_host[0] = over; flag_host[1] = (int)need; }
    // the tiles nobody sent are one constant: the backgrounds summed in rank order (the per-pixel arithmetic, done once)
    double bg = 0.0;
    for (int r = 0; r < world; ++r) {
        const double v = packets[(size_t)r * packet_doubles + 1];
        bg = (r == 0) ? v : bg + v;
    }
    if (avg_T > 0) bg = bg / (double)avg_T;
    __shared__ int s_const;
    if (threadIdx.x == 0) s_const = 0;
    __syncthreads();   // also orders the any[] writes above before the reads below
    int mine = 0;
    for (int i = threadIdx.x; i < ntiles; i += 256) mine |= (any[i] == 0);
    if (mine) s_const = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        st->sp_bg = bg;
        if (s_const) { st->heat_min_keys[0] = f64_key(bg); st->heat_max_keys[0] = f64_key(bg); }
    }
}

// fused[p] = sum over ranks (in rank order) of heat_r[p]; also the fused heatmap's min / max (striped)
// avg_T > 0: the packets hold partial time SUMS of a frame-sharded buffer; the fused value is their sum / avg_T.
// A tile no rank sent is the constant k_sparse_index prepared (already in the extrema), stored 16 bytes per lane.
RM_KERNEL __launch_bounds__(256) void k_sparse_merge(const double *packets, size_t packet_doubles, int world, int cap, int H, int W,
                                                      int tiles_x, int ntiles, const int *map, const int *any, double *fused,
                                                      CollapseState *st, int avg_T)
{
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * CT_H, x0 = tx * CT_W;
    if (!any[tile]) {   // workgroup-uniform
        const double acc = st->sp_bg;
        const int x = x0 + 2 * (threadIdx.x & 31);
        const bool pair = ((W & 1) == 0) && x + 1 < W;   // even W: every row starts 16-byte aligned (x is even)
#pragma unroll
        for (int k = 0; k < CT_H / 8; ++k) {
            const int y = y0 + (threadIdx.x >> 5) + 8 * k;
            if (y >= H) continue;
            double *dst = fused + (size_t)y * W + x;
            if (pair) {
                *reinterpret_cast<F64Pair *>(dst) = F64Pair{acc, acc};
            } else {
                if (x < W) dst[0] = acc;
                if (x + 1 < W) dst[1] = acc;
            }
        }
        return;
    }
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    for (int i = threadIdx.x; i < CT_H * CT_W; i += 256) {
        const int y = y0 + i / CT_W, x = x0 + (i & (CT_W - 1));
        if (y >= H || x >= W) continue;
        double acc = 0.0;
        for (int r = 0; r < world; ++r) {
            const double *pk = packets + (size_t)r * packet_doubles;
            const int slot = map[(size_t)r * ntiles + tile];
            const double v = slot >= 0 ? pk[SP_HDR + cap + (size_t)slot * (CT_H * CT_W) + i] : pk[1];
            acc = (r == 0) ? v : acc + v;
        }
        if (avg_T > 0) acc = acc / (double)avg_T;   // np.average = sum / T (base.py:562)
        fused[(size_t)y * W + x] = acc;
        mn = (acc < mn) ? acc : mn;
        mx = (acc > mx) ? acc : mx;
    }
    block_minmax(mn, mx);
    if (threadIdx.x == 0) {
        const unsigned long long kmn = f64_key(mn), kmx = f64_key(mx);
        const int sp = blockIdx.x & (NSTRIPE - 1);
        striped_min_max(st->heat_min_keys, st->heat_max_keys, sp, kmn, kmx);
    }
}

}  // namespace rm
