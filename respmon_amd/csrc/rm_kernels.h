// respmon_amd/csrc/rm_kernels.h -- what the gfx950 HIP kernels of more than one stage share: the kernel macros, the host waits, the
// trace hooks, pixel loads and border rules, the float64 keys and wave reductions, the geometry of the small pyramid and of the tile
// chain with its walk through LDS, the reduction state of the collapse passes (CollapseState, k_state_init) and the SumPlan.
// The kernels themselves live in one header per stage, included by the units that launch them:
//   rm_pyr_kernels.h       pyrDown / pyrUp on whole levels                      rm_pyramid.hip
//   rm_temporal_kernels.h  temporal band-pass, lfilter                          rm_temporal.hip
//   rm_small_kernels.h     small pyramid in LDS, tile bounds, filter-first      rm_front.hip, rm_collapse_eval.hip
//   rm_select_kernels.h    selection, evaluation, min / max, masked sum         rm_collapse_eval.hip, rm_collapse_sum.hip, rm_calibrate.hip
//   rm_rate_kernels.h      spectral peak per pixel column (rate map)            rm_rate.hip
//   rm_heat_kernels.h      heatmap -> uint8 image, sparse heatmap packets       rm_roi.hip, rm_calibrate.hip
//   rm_roi_kernels.h       dtype conversions, time average, ROI mean / crop     rm_ctx.hip, rm_temporal.hip, rm_motion.hip
//
// All arithmetic that decides the ROI is float64 with the operation order of the reference's
// numpy / OpenCV-scalar path (no FMA contraction: the library is built with -ffp-contract=off),
// so results are reproducible op-for-op against the CPU oracle.
//
// Reference functions restated (paths relative to the reference root):
//   pyramid.py:9-28   Gaussian / Laplacian image pyramid (cv2.pyrDown / cv2.pyrUp)
//   pyramid.py:51-69  collapse
//   transforms.py:82-102  temporal FFT band-pass (as the explicit linear operator M)
//   transforms.py:184-192 global min/max mask
//   base.py:562-566   time average, normalise, float_to_uint8, threshold
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <chrono>

// Non-template kernels are function templates with one defaulted parameter (launched as k_name<>): a unit generates device code only
// for the kernels it launches, and each kernel is launched from ONE unit (tools/check_resources.py fails the build on a second copy).
// A host function that launches a kernel is therefore never defined in a header that several units include.
#define RM_KERNEL template <int RM_UNIT_ = 0> __global__
// N-element vector type (clang spells it ext_vector_type, the g++ of the tests' host emulation vector_size): MFMA accumulators, 16-byte loads
#ifdef RM_HIPEMU
#define RM_VEC(T, N) T __attribute__((vector_size(sizeof(T) * (N))))
#else
#define RM_VEC(T, N) T __attribute__((ext_vector_type(N)))
#endif
#define RM_WAVES_PER_EU(n) __attribute__((amdgpu_waves_per_eu(n, n)))   // register budget of 512 / n per lane
#ifndef RM_HIPEMU
#define RM_WAVES_PER_EU_IF(cond, a, b) __attribute__((amdgpu_waves_per_eu((cond) ? (a) : (b), (cond) ? (a) : (b))))   // ... chosen by a template parameter
#else
#define RM_WAVES_PER_EU_IF(cond, a, b)   // (g++ does not parse an expression inside an attribute it does not know)
#endif

namespace rm {

// Host wait for a result on `s`.  hipStreamSynchronize sleeps on an interrupt (tens of microseconds to wake up);
// the calls that return host results are latency-critical (one per locate(), one per measured frame), so poll
// first and only fall back to the blocking wait when the stream is still busy after a few milliseconds.
inline hipError_t stream_wait(hipStream_t s)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(4)) return hipStreamSynchronize(s);
    }
}

// ... for the work in front of an event (rm_locate_result: the stream already carries the next submission)
inline hipError_t event_wait(hipEvent_t ev)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(4)) return hipEventSynchronize(ev);
    }
}


// ----------------------------------------------------------------------------------------
// Workgroup timeline tracing -- DEVELOPER BUILD ONLY (make librespmon_hip_trace.so, tools/trace_tail.py).  In the product
// library RM_TRACE is undefined and both macros expand to nothing.  A traced workgroup records the 100 MHz wall clock at
// entry and exit plus the CU it ran on, so launch ramps, imbalance and per-workgroup latency can be read off per kernel.
// ----------------------------------------------------------------------------------------
#ifdef RM_TRACE
struct TraceRec { unsigned long long t0, t1, c0, c1; unsigned int hwid, xcc; };   // t: 100 MHz wall clock, c: shader clock (s_memtime)
constexpr int TRACE_KERNELS = 16, TRACE_BLOCKS = 20480;
__device__ TraceRec *g_trace_buf = nullptr;
__device__ __forceinline__ void trace_end(int kid, unsigned long long t0, unsigned long long c0)
{
    if (threadIdx.x != 0 || !g_trace_buf) return;
    const unsigned b = blockIdx.x + blockIdx.y * gridDim.x;
    if (b >= (unsigned)TRACE_BLOCKS) return;
    TraceRec &r = g_trace_buf[(size_t)kid * TRACE_BLOCKS + b];
    r.t0 = t0; r.t1 = wall_clock64(); r.c0 = c0; r.c1 = clock64();
    r.hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
    r.xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);    // HW_REG_XCC_ID
}
struct TraceScope {
    int kid; unsigned long long t0, c0;
    __device__ __forceinline__ TraceScope(int k) : kid(k), t0(wall_clock64()), c0(clock64()) {}
    __device__ __forceinline__ ~TraceScope() { trace_end(kid, t0, c0); }
};
#define RM_TRACE_SCOPE(KID) TraceScope rm_trace_scope_(KID)
// phase marks inside ONE workgroup (block 5) of a kernel: mark i = wall clock when thread 0 passes the call; they live in
// the records of the last pseudo-kernel (TRACE_KERNELS - 1), field t0 of record kid * TRACE_MARKS + i
constexpr int TRACE_MARKS = 16;
__device__ __forceinline__ void trace_mark(int kid, int i)
{
    if (threadIdx.x == 0 && blockIdx.x == 5 && blockIdx.y == 0 && g_trace_buf)
        g_trace_buf[(size_t)(TRACE_KERNELS - 1) * TRACE_BLOCKS + kid * TRACE_MARKS + i].t0 = wall_clock64();
}
#define RM_TRACE_MARK(KID, I) trace_mark(KID, I)
#else
#define RM_TRACE_SCOPE(KID)
#define RM_TRACE_MARK(KID, I)
#endif

// ----------------------------------------------------------------------------------------
// small helpers
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = (p < 0) ? -p : 2 * len - 2 - p;
    return p;
}

// The band-passed video is EVEN in time.  transforms.py:98 takes Re(ifft(.)) of a REAL (packed-rfft) array, so the filter output
// satisfies out[s] == out[n - s] for 0 < s < n -- bit for bit in the reference (scipy's ifft of a real sequence is exactly
// Hermitian) and here (the stage-2 operator is evaluated for s <= n / 2 only, rm_temporal.hip get_operator).  Every per-frame stage
// after the filter is a function of the frame alone, so C_S, the tile bounds and raw inherit the symmetry: the library computes and
// stores the T / 2 + 1 UNIQUE frames and the time-ordered consumers (the masked sum) read frame t through sym_frame().
__host__ __device__ __forceinline__ int sym_frames(int T) { return T / 2 + 1; }
__host__ __device__ __forceinline__ int sym_frame(int t, int T) { return 2 * t <= T ? t : T - t; }
// does the frame range [t0, t1) of a T-frame buffer hold a frame whose unique frame is u?
__host__ __device__ __forceinline__ bool sym_in_range(int u, int T, int t0, int t1)
{
    return (u >= t0 && u < t1) || (u > 0 && T - u >= t0 && T - u < t1);
}

// slot_of[] (which pairs the masked time sum keeps, k_select_pairs) is TILE-major -- [tile][unique frame] -- so that the sum kernels,
// which walk the frames of one tile, find them in a few cache lines (frame-major: one line per frame, 129 scattered lines per tile
// and reader at 1080p x 256); the pair index of the lists and bounds stays u * ntiles + tile
__host__ __device__ __forceinline__ size_t slot_index(int u, int tile, int Th) { return (size_t)tile * Th + u; }

// widening loads; uint8 applies uint8_to_float's  k * (1./255)  (transforms.py:20-23)
__device__ __forceinline__ double load_px(const uint8_t *p, size_t i) { return (double)p[i] * (1.0 / 255); }
// uint16 (RM_U16): uint16_to_float's  k * (1./65535), one float64 multiplication.  Never through a float: 65 534 of the 65 536 values
// are not float32 numbers
__device__ __forceinline__ double u16_to_f64(unsigned k) { return (double)k * (1.0 / 65535); }
__device__ __forceinline__ double load_px(const uint16_t *p, size_t i) { return u16_to_f64(p[i]); }
__device__ __forceinline__ double load_px(const __half *p, size_t i) { return (double)__half2float(p[i]); }
__device__ __forceinline__ double load_px(const float *p, size_t i) { return (double)p[i]; }
__device__ __forceinline__ double load_px(const double *p, size_t i) { return p[i]; }

// order-preserving map double -> uint64 so that atomicMin/atomicMax on the key orders doubles
__device__ __forceinline__ unsigned long long f64_key(double d)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double f64_unkey(unsigned long long k)
{
    unsigned long long b = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// float_to_uint8 (transforms.py:26-29): v*255 then C cast (truncate toward zero, low byte;
// NaN / |v| >= 2^31 -> 0, the x86 cvttsd2si result numpy produces)
__device__ __forceinline__ uint8_t f64_to_u8_trunc(double v255)
{
    if (!(v255 == v255) || v255 >= 2147483648.0 || v255 <= -2147483649.0) return 0;
    return (uint8_t)((int)v255 & 255);
}
// float_to_uint16: the same rule on v * 65535, low 16 bits
__device__ __forceinline__ uint16_t f64_to_u16_trunc(double v65535)
{
    if (!(v65535 == v65535) || v65535 >= 2147483648.0 || v65535 <= -2147483649.0) return 0;
    return (uint16_t)((int)v65535 & 65535);
}

// Wave (64-lane) reductions; the result is valid in every lane.
// On the GPU they run on DPP row shifts / broadcasts (VALU speed): a __shfl_xor butterfly compiles to ds_bpermute, i.e. six
// dependent LDS round trips per 32-bit word -- the latency-bound tail kernels spent 1-3 us each in their folds and extrema.
//   row_shr:1,2,4,8 leave the reduction of each 16-lane row in its last lane (a lane without a source keeps its own value:
//   harmless for min / max), row_bcast:15 folds rows 0->1 and 2->3, row_bcast:31 folds the lower half into lane 63.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int dpp_i32(int v)
{
    return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xF, false);
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v)
{
    const int lo = dpp_i32<CTRL, ROW_MASK>((int)(unsigned)v), hi = dpp_i32<CTRL, ROW_MASK>((int)(unsigned)(v >> 32));
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ unsigned long long bits_of(double d) { return (unsigned long long)__double_as_longlong(d); }
__device__ __forceinline__ unsigned long long bits_of(unsigned long long d) { return d; }
__device__ __forceinline__ void from_bits(unsigned long long b, double &d) { d = __longlong_as_double((long long)b); }
__device__ __forceinline__ void from_bits(unsigned long long b, unsigned long long &d) { d = b; }
template <int CTRL, int ROW_MASK, typename T> __device__ __forceinline__ T dpp_get(T v)
{
    T o;
    from_bits(dpp_u64<CTRL, ROW_MASK>(bits_of(v)), o);
    return o;
}
template <typename T, typename Op> __device__ __forceinline__ T wave_reduce(T v, Op op)   // T: double or unsigned long long
{
    v = op(dpp_get<0x111, 0xF>(v), v);   // row_shr:1
    v = op(dpp_get<0x112, 0xF>(v), v);   // row_shr:2
    v = op(dpp_get<0x114, 0xF>(v), v);   // row_shr:4
    v = op(dpp_get<0x118, 0xF>(v), v);   // row_shr:8
    v = op(dpp_get<0x142, 0xA>(v), v);   // row_bcast:15 into rows 1 and 3
    v = op(dpp_get<0x143, 0xC>(v), v);   // row_bcast:31 into rows 2 and 3
    const unsigned long long b = bits_of(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 63);
    T r;
    from_bits(((unsigned long long)hi << 32) | lo, r);
    return r;
}
// arg-reduction: the value and the position that holds it travel together
template <typename Less> __device__ __forceinline__ void wave_arg_reduce(double &v, int &idx, Less less)
{
#define RM_ARG_STEP(CTRL, MASK)                                                  \
    {                                                                            \
        const double ov = dpp_get<CTRL, MASK>(v);                                \
        const int oi = dpp_i32<CTRL, MASK>(idx);                                 \
        if (less(ov, v)) { v = ov; idx = oi; }                                   \
    }
    RM_ARG_STEP(0x111, 0xF) RM_ARG_STEP(0x112, 0xF) RM_ARG_STEP(0x114, 0xF) RM_ARG_STEP(0x118, 0xF)
    RM_ARG_STEP(0x142, 0xA) RM_ARG_STEP(0x143, 0xC)
#undef RM_ARG_STEP
    const unsigned long long b = bits_of(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 63);
    from_bits(((unsigned long long)hi << 32) | lo, v);
    idx = __builtin_amdgcn_readlane(idx, 63);
}
// min / max of two doubles as ONE instruction.  __builtin_fmin / fmax put a canonicalising v_max_f64 x, x, x in front of every operand
// the compiler cannot prove quiet (loads, DPP moves, loop-carried values): three instructions instead of one in kernels that do
// little else (rm_bounds_l1.h).  The operands here are never signalling NaNs (arithmetic results and loaded image data); a quiet NaN
// operand yields the other operand, as fmin / fmax do.
__device__ __forceinline__ double f64_min(double a, double b)
{
#ifndef RM_HIPEMU
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    return __builtin_fmin(a, b);
#endif
}
__device__ __forceinline__ double f64_max(double a, double b)
{
#ifndef RM_HIPEMU
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    return __builtin_fmax(a, b);
#endif
}

__device__ __forceinline__ double wave_min(double v) { return wave_reduce(v, [](double o, double w) { return (o < w) ? o : w; }); }
__device__ __forceinline__ double wave_max(double v) { return wave_reduce(v, [](double o, double w) { return (o > w) ? o : w; }); }

// ----------------------------------------------------------------------------------------
// Geometry of the small pyramid (rm_small_kernels.h): levels S .. L-1 of one frame, side by side in LDS and in a [NP] row
// ----------------------------------------------------------------------------------------
constexpr int SMALL_MAX_LEVELS = 16;
constexpr int SMALL_NT = 1024;     // one workgroup per frame and per CU: 16 waves hide the LDS / global latencies
struct SmallGeom {
    int S, L;                        // levels S .. L-1 take part
    int h[SMALL_MAX_LEVELS], w[SMALL_MAX_LEVELS];
    int g_off[SMALL_MAX_LEVELS];     // LDS offset (doubles) of Gaussian level l
    int np_off[SMALL_MAX_LEVELS];    // offset of level l inside a [NP] frame of lap_all / bp_all
    int NP;
};

// ---- pyrUp inside LDS, separable and branch-free -------------------------------------------------------------
// up_h() (rm_pyr_kernels.h) chooses between five differently shaped expressions per column (interior / left / right border,
// even / odd), which on a wavefront means divergent branches and every shape executed.  The same values, bit for
// bit, come out of ONE shape with per-column operands and weights fixed once per level:
//     h(x) = (A*wa + B*wb) + C*wc
//   even interior  A=s[j-1] B=s[j] C=s[j+1]  w = 1,6,1    == s[j-1] + s[j]*6 + s[j+1]
//   even left      B=s[0]   C=s[1]           w = 0,6,2    == s[0]*6 + s[1]*2          (0 + x is exact)
//   even right     A=s[j-1] B=s[j]           w = 1,7,0    == s[j-1] + s[j]*7          (x + 0 is exact)
//   odd  interior  B=s[j]   C=s[j+1]         w = 0,4,4    == (s[j] + s[j+1])*4        (scaling by 4 commutes with rounding)
//   odd  right / single column  B=C=s[j]     w = 0,4,4    == s[j]*8
// (only the sign of an exact zero can differ, which no later operation observes).  The vertical pass needs no such
// trick: OpenCV's border rules are index clamps there, and row parity is uniform across a wavefront.
struct HTap { int ia, ib, ic; double wa, wb, wc; };

__device__ __forceinline__ HTap make_htap(int x, int sw)   // destination column x of a pyrUp from a source row of width sw
{
    HTap t;
    const int j = x >> 1;
    const bool odd = (x & 1) != 0, single = sw == 1, left = j == 0, right = j == sw - 1;
    const bool four = odd || single;                      // the (B + C) * 4 shapes
    t.ib = j;
    t.ia = (four || left) ? j : j - 1;                   // unused (weight 0) in those shapes: any valid index
    t.ic = (single || right) ? j : j + 1;
    t.wa = (four || left) ? 0.0 : 1.0;
    t.wb = four ? 4.0 : (right ? 7.0 : 6.0);
    t.wc = four ? 4.0 : (left ? 2.0 : (right ? 0.0 : 1.0));
    return t;
}

// ----------------------------------------------------------------------------------------
// Fused collapse from level S to full resolution (pyramid.py:51-69 for the levels below
// skip_levels_at_top, which are all-zero in the band-passed pyramid: transforms.py:150-160).
//
// One single-wave workgroup owns a CT_W x CT_H tile of the full-resolution frame.  For a frame
// t it stages the level-S footprint of the tile in LDS, runs the pyrUp chain S..1 inside LDS
// and evaluates level 0 in registers (thread = column, marching down CT_H rows so every
// horizontal value is computed once).  No [T,H,W] array is ever written.
// ----------------------------------------------------------------------------------------
constexpr int CT_W = 64, CT_H = 16;
constexpr int MAX_CHAIN = 8;

struct ChainGeom {
    int S;                       // number of pyrUp steps (== skip_levels_at_top), 1..MAX_CHAIN-1
    int h[MAX_CHAIN], w[MAX_CHAIN];  // level sizes, index 0 = full resolution
    int lds_off[MAX_CHAIN];      // offset (doubles) of level k's tile buffer in LDS, k = 1..S
    int lds_hb[MAX_CHAIN];       // offset of the scratch buffer of the horizontal pass of step k -> k-1 (chain_step), k = 2..S
    int lds_total;               // doubles
    int tiles_x, tiles_y;
    double lat_a, lat_b;         // raw[t, y << S, x << S] == lat_a * (c[y-1] + c[y+1]) + lat_b * c[y] per axis (lattice_sample)
};

struct Region { int y0, y1, x0, x1; };  // inclusive

__host__ __device__ __forceinline__ int floordiv2(int a) { return a >> 1; }  // arithmetic shift == floor for negatives

// footprint of `tile` at level k (0 = the tile itself): scalars only, so nothing lands in scratch
__host__ __device__ __forceinline__ Region tile_region(const ChainGeom &g, int tile, int k)
{
    int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    Region R;
    R.y0 = ty * CT_H; R.y1 = min(R.y0 + CT_H, g.h[0]) - 1;
    R.x0 = tx * CT_W; R.x1 = min(R.x0 + CT_W, g.w[0]) - 1;
    for (int i = 1; i <= k; ++i) {
        R.y0 = max(0, floordiv2(R.y0) - 1);
        R.y1 = min(g.h[i] - 1, floordiv2(R.y1) + 1);
        R.x0 = max(0, floordiv2(R.x0) - 1);
        R.x1 = min(g.w[i] - 1, floordiv2(R.x1) + 1);
    }
    return R;
}

// worst-case tile-buffer extent of level k (host + device agree on the LDS layout)
__host__ __device__ inline int chain_extent(int base, int k)
{
    int lo = 0, hi = base - 1;  // worst case is an interior tile starting at a multiple of `base`
    for (int i = 0; i < k; ++i) { lo = (lo >> 1) - 1; hi = (hi >> 1) + 1; }
    return hi - lo + 1;
}

struct LdsImg {  // a level's tile buffer: absolute coordinates -> LDS
    const double *p; int y0, x0, pitch;
    __device__ __forceinline__ double operator()(int r, int c) const { return p[(r - y0) * pitch + (c - x0)]; }
};

// block-wide min / max: wave shuffles, then one LDS hop across the block's waves (blockDim.x <= 256)
__device__ __forceinline__ void block_minmax(double &mn, double &mx)
{
    __shared__ double s_mn[4], s_mx[4];
    mn = wave_min(mn); mx = wave_max(mx);
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { s_mn[wave] = mn; s_mx[wave] = mx; }
    __syncthreads();
    mn = s_mn[0]; mx = s_mx[0];
    for (int i = 1; i < nw; ++i) { mn = (s_mn[i] < mn) ? s_mn[i] : mn; mx = (s_mx[i] > mx) ? s_mx[i] : mx; }
    __syncthreads();
}

// i -> (i / nw, i % nw) for the small element counts of a tile buffer (i < 2^16, 1 <= nw <= 2^10): one multiply
// by the reciprocal instead of the ~35-instruction integer division; (i + 0.5) / nw is at least 0.5 / nw away
// from an integer, far more than the float rounding error at these magnitudes, so the floor is exact
__device__ __forceinline__ void split_rc(int i, int nw, float inv_nw, int &r, int &c)
{
    r = (int)(((float)i + 0.5f) * inv_nw);
    c = i - r * nw;
}

// LDS hand-off between the lanes of ONE wave: the LDS executes a wave's DS instructions in order, so a
// read issued after a write sees it; only the compiler must be kept from reordering them.  (The host
// emulation models lanes as fibers and needs a real barrier.)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// wave-uniform value into a scalar register (index math derived from it then runs on the scalar unit)
__device__ __forceinline__ int uniform(int v)
{
    return __builtin_amdgcn_readfirstlane(v);
}

// device-side scalars shared by the collapse passes
// Thousands of workgroups finish at about the same time and all want to fold their extremum into ONE word:
// same-address atomics serialise at ~5-12 ns each (100+ us for the evaluation pass).  Each reduction target is
// therefore striped over NSTRIPE words (workgroup b uses stripe b % NSTRIPE); readers fold the stripes with one
// load per lane and a wave reduction.
constexpr int NSTRIPE = 64;

struct CollapseState {
    unsigned long long lb_max_key;  // max over pairs of lo  (lower bound of raw.max())
    unsigned long long ub_min_key;  // min over pairs of hi  (upper bound of raw.min())
    unsigned long long ub_max_key;  // max over pairs of hi  (upper bound of raw.max())
    unsigned long long lb_min_key;  // min over pairs of lo  (lower bound of raw.min())
    unsigned long long min_key, max_key;  // exact raw.min() / raw.max()
    unsigned long long lb_max_keys[NSTRIPE], ub_min_keys[NSTRIPE], ub_max_keys[NSTRIPE], lb_min_keys[NSTRIPE];
    unsigned long long min_keys[NSTRIPE], max_keys[NSTRIPE];  // stripes of the six words above
    unsigned long long heat_min_keys[NSTRIPE], heat_max_keys[NSTRIPE];  // stripes of heat_min_key / heat_max_key
    unsigned long long smp_min_keys[NSTRIPE], smp_max_keys[NSTRIPE];    // extrema of the lattice samples (true raw values)
    unsigned int n_list_a;          // (frame, tile) pairs that may hold raw.min() / raw.max(): always evaluated (k_select_pairs -> list_a)
    unsigned int n_list_b;          // pairs kept for the masked time sum that are not in list_a: evaluated on the sparse path only
    unsigned int n_slots;           // pairs whose values are kept for the masked time sum = slots of the value store handed out
    unsigned int n_heavy;           // tiles with at least one such pair among this rank's frames (k_select_pairs -> heavy[])
    double margin;                  // absolute safety margin of the bounds
    double top_ub;                  // upper bound of `top`, from the bounds alone
    double min_val, max_val, top;   // transforms.py:185-189, decoded by k_finish_minmax
    unsigned long long heat_min_key, heat_max_key;
    double sp_bg;                   // sparse merge: rank-ordered sum of the packets' backgrounds (k_sparse_index)
};

__device__ void state_init_lane(CollapseState *st, int i)   // lanes 0 .. NSTRIPE-1 of one wavefront
{
    if (i >= NSTRIPE) return;
    st->lb_max_keys[i] = 0ull; st->ub_min_keys[i] = ~0ull; st->ub_max_keys[i] = 0ull; st->lb_min_keys[i] = ~0ull;
    st->min_keys[i] = ~0ull; st->max_keys[i] = 0ull;
    st->heat_min_keys[i] = ~0ull; st->heat_max_keys[i] = 0ull;
    st->smp_min_keys[i] = ~0ull; st->smp_max_keys[i] = 0ull;
    if (i != 0) return;
    st->lb_max_key = 0ull; st->ub_min_key = ~0ull; st->ub_max_key = 0ull; st->lb_min_key = ~0ull;
    st->min_key = ~0ull; st->max_key = 0ull; st->n_list_a = 0; st->n_list_b = 0; st->n_slots = 0; st->n_heavy = 0;
    st->margin = 0; st->top_ub = 0; st->min_val = 0; st->max_val = 0; st->top = 0;
    st->heat_min_key = ~0ull; st->heat_max_key = 0ull;
}

RM_KERNEL __launch_bounds__(NSTRIPE) void k_state_init(CollapseState *st) { state_init_lane(st, (int)threadIdx.x); }

// min / max of a pair of striped targets: skipped when they cannot change the result.  Both current words are requested before either is
// compared -- a load-compare-atomic at a time is a round trip per target at the end of a wave's life (rm_bounds_l1.h)
__device__ __forceinline__ void striped_min_max(unsigned long long *mins, unsigned long long *maxs, int sp, unsigned long long kmn, unsigned long long kmx)
{
    const unsigned long long cmn = *(volatile unsigned long long *)&mins[sp], cmx = *(volatile unsigned long long *)&maxs[sp];
    if (kmn < cmn) atomicMin(&mins[sp], kmn);
    if (kmx > cmx) atomicMax(&maxs[sp], kmx);
}

// fold the stripes of one target (plus its unstriped word); every lane of the wave gets the result
__device__ __forceinline__ unsigned long long fold_min_keys(const unsigned long long *stripes, unsigned long long word)
{
    unsigned long long v = stripes[threadIdx.x & (NSTRIPE - 1)];
    v = wave_reduce(v, [](unsigned long long o, unsigned long long w) { return (o < w) ? o : w; });
    return (word < v) ? word : v;
}
__device__ __forceinline__ unsigned long long fold_max_keys(const unsigned long long *stripes, unsigned long long word)
{
    unsigned long long v = stripes[threadIdx.x & (NSTRIPE - 1)];
    v = wave_reduce(v, [](unsigned long long o, unsigned long long w) { return (o > w) ? o : w; });
    return (word > v) ? word : v;
}

// stage the level-S footprint of `tile` for frame t
__device__ __forceinline__ Region chain_stage(const ChainGeom &g, int tile, const double *cS_t, double *lds)
{
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int S = g.S;
    const Region Rk = tile_region(g, tile, S);
    double *d = lds + g.lds_off[S];
    const int nw = Rk.x1 - Rk.x0 + 1, n = (Rk.y1 - Rk.y0 + 1) * nw, wS = g.w[S];
    const float inv_nw = 1.0f / (float)nw;
    for (int i = tid; i < n; i += nthr) {
        int r, c;
        split_rc(i, nw, inv_nw, r, c);
        d[i] = cS_t[(size_t)(Rk.y0 + r) * wS + Rk.x0 + c];
    }
    __syncthreads();
    return Rk;
}

// one pyrUp step inside LDS, level k (footprint Rk) -> level k-1: horizontal pass into the scratch buffer (every
// source row at the destination columns), then the vertical pass.  Wave w takes rows w, w + nwaves, ...; lane = column.
__device__ __forceinline__ Region chain_step(const ChainGeom &g, int tile, double *lds, int k, const Region &Rk)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
    const Region Rd = tile_region(g, tile, k - 1);
    const double *src = lds + g.lds_off[k];
    double *hb = lds + g.lds_hb[k], *dst = lds + g.lds_off[k - 1];
    const int sp = Rk.x1 - Rk.x0 + 1, srows = Rk.y1 - Rk.y0 + 1;      // source pitch / rows
    const int dw = Rd.x1 - Rd.x0 + 1, drows = Rd.y1 - Rd.y0 + 1;
    const int sh = g.h[k], sw = g.w[k];
    for (int c = lane; c < dw; c += 64) {
        const HTap t = make_htap(Rd.x0 + c, sw);
        const int oa = t.ia - Rk.x0, ob = t.ib - Rk.x0, oc = t.ic - Rk.x0;
        for (int r = wave; r < srows; r += nwaves) {
            const double *row = src + r * sp;
            hb[r * dw + c] = (row[oa] * t.wa + row[ob] * t.wb) + row[oc] * t.wc;
        }
    }
    __syncthreads();
    for (int r = wave; r < drows; r += nwaves) {
        const int y = Rd.y0 + r, i = y >> 1;                          // uniform per wave: no divergence
        const int r2 = ((i == sh - 1) ? i : i + 1) - Rk.y0;
        const int r1 = i - Rk.y0;
        if (y & 1) {
            for (int c = lane; c < dw; c += 64) dst[r * dw + c] = ((hb[r1 * dw + c] + hb[r2 * dw + c]) * 4) * (1.0 / 64);
        } else {
            const int r0 = ((i == 0) ? (sh > 1 ? 1 : 0) : i - 1) - Rk.y0;
            for (int c = lane; c < dw; c += 64)
                dst[r * dw + c] = (hb[r0 * dw + c] + hb[r1 * dw + c] * 6 + hb[r2 * dw + c]) * (1.0 / 64);
        }
    }
    __syncthreads();
    return Rd;
}

// stage the level-S footprint of `tile` for frame t, then run the chain S -> 1 inside LDS
__device__ __forceinline__ void chain_to_level1(const ChainGeom &g, int tile, const double *cS_t, double *lds)
{
    Region Rk = chain_stage(g, tile, cS_t, lds);
    RM_TRACE_MARK(5, 2);
    for (int k = g.S; k >= 2; --k) { Rk = chain_step(g, tile, lds, k, Rk); RM_TRACE_MARK(5, 3 + (g.S - k)); }
}

// level 1 (LDS) -> level 0 for this lane's column: out[j] = raw[t, y0 + j0 + j, x], j < NR (j0, NR even)
template <int NR>
__device__ __forceinline__ void level0_rows(const ChainGeom &g, const Region &R0, const Region &R1, const double *lds, int x, int j0,
                                            double (&out)[NR])
{
    const double *src = lds + g.lds_off[1];
    const int sp = R1.x1 - R1.x0 + 1;
    const int sh = g.h[1], sw = g.w[1];
    const HTap t = make_htap(x, sw);
    const int oa = t.ia - R1.x0, ob = t.ib - R1.x0, oc = t.ic - R1.x0;
    // horizontal values of source rows i0-1 .. i0+NR/2 (border rules applied by row index)
    const int i0 = (R0.y0 + j0) >> 1;  // R0.y0 is a multiple of CT_H, j0 is even
    double hv[NR / 2 + 2];
#pragma unroll
    for (int k = 0; k < NR / 2 + 2; ++k) {
        int i = i0 - 1 + k;
        int r = (i < 0) ? (sh > 1 ? 1 : 0) : (i > sh - 1 ? sh - 1 : i);
        const double *row = src + (r - R1.y0) * sp;
        hv[k] = (row[oa] * t.wa + row[ob] * t.wb) + row[oc] * t.wc;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        int k = (j >> 1) + 1;  // hv index of source row i = (y0+j0+j)/2
        if (j & 1) out[j] = ((hv[k] + hv[k + 1]) * 4) * (1.0 / 64);
        else out[j] = (hv[k - 1] + hv[k] * 6 + hv[k + 1]) * (1.0 / 64);
    }
}

constexpr double PRUNE_REL_MARGIN = 1e-12;  // >> the ~1e-14 relative rounding of the S-level chain

constexpr int SLOT_PRUNED = -1;    // every value of the pair is provably >= top: contributes `min`
// slot >= 0: the pair's 16 x 64 values are parked in slot `slot` of the value store for the masked time sum.  k_select_pairs hands
// the slots out so that the kept frames of a tile are NEIGHBOURS in the store (one contiguous run per tile and frame chunk): the
// sum pass walks a tile's frames, and slots scattered over the store cost it a TLB / DRAM-page miss per frame.
//
// Sparse or dense sum?  (rm_dense_sum.h)  Decided ON THE DEVICE from what this call's own selection kept -- every kernel that
// cares evaluates sum_is_dense() on the counters k_select_pairs left in the state, so the first call of a geometry behaves like
// the hundredth and nothing is remembered between calls:
//   * more kept pairs than the value store has slots -> dense (the store is capped: rm_collapse_eval.hip collapse_eval);
//   * skip <= 2 and more than one pair in DENSE_ONE_IN kept -> dense (measured per pair of the geometry on MI355X: sparse 3.7-4.8 ns
//     per KEPT pair; dense 1.6 ns at 4K x 512 skip 2, 3.6 ns at 720p x 128 skip 2, 4.6 ns at 1080p x 256 skip 4 -- slower than
//     sparse even with everything kept, so deeper chains go dense only on overflow);
//   * RM_FLAG_DENSE_SUM / RM_FLAG_SPARSE_SUM force it (an overflowing store still goes dense).
constexpr unsigned long long DENSE_ONE_IN = 2;
struct SumPlan {
    int mode;                  // 0 automatic, 1 dense, 2 sparse
    unsigned int cap_slots;    // slots of the value store
    unsigned int npairs_mine;  // unique (tile, frame) pairs among this rank's frames
    int auto_dense_ok;         // the automatic rule may choose the dense kernel (skip <= 2)
};
__device__ __forceinline__ bool sum_is_dense(const CollapseState *st, const SumPlan &sp)
{
    const unsigned int kept = st->n_slots;
    if (sp.mode == 1 || kept > sp.cap_slots) return true;
    if (sp.mode == 2) return false;
    return sp.auto_dense_ok && (unsigned long long)kept * DENSE_ONE_IN > (unsigned long long)sp.npairs_mine;
}

constexpr int MAX_T = 4096;   // frames of one buffer: the sum kernels keep a tile's list of kept frames in LDS (k_masked_sum_tiles, k_dense_sum_t)
struct alignas(16) F64Pair { double a, b; };   // two values in one 16-byte store or load

// cv2.cvtColor(BGR2GRAY), base.py:230: Y = (B*1868 + G*9617 + R*4899 + 8192) >> 14 (k_bgr_to_gray, rm_roi_kernels.h).  What follows is
// shared by k_bgr_to_gray_quads there and the frame-buffer kernel of RM_BGR8 buffers (rm_down_chain_u8.h).
// The same sum on whole words.  The weights do not fit a byte, so it is two v_dot4_u32_u8 (low and high bytes of the weights; the
// fourth byte of the word meets a zero weight) joined by one v_lshl_add_u32; a pixel whose three bytes straddle two words is brought
// together by v_alignbyte_b32 first.
constexpr unsigned BGR_W_LO = 0x0023914Cu, BGR_W_HI = 0x00132507u;   // 1868 = 0x074C, 9617 = 0x2591, 4899 = 0x1323: byte 0 = B, 1 = G, 2 = R

// gray value of the pixel whose B sits in byte SH of word d0 (its G / R may continue in d1), times 8: the byte offset into the table
template <int SH> __device__ __forceinline__ unsigned bgr_gray_x8(unsigned d0, unsigned d1)
{
    unsigned x = d0, wlo = BGR_W_LO, whi = BGR_W_HI;
    if constexpr (SH == 1) { wlo = BGR_W_LO << 8; whi = BGR_W_HI << 8; }        // bytes 1..3 of d0: move the weights, not the pixel
    else if constexpr (SH >= 2) x = __builtin_amdgcn_alignbyte(d1, d0, SH);     // {d1, d0} >> 8 SH
    const unsigned lo = __builtin_amdgcn_udot4(x, wlo, 8192u, false), hi = __builtin_amdgcn_udot4(x, whi, 0u, false);
    return (((hi << 8) + lo) >> 11) & 0x7f8u;                                  // (sum >> 14) << 3
}

}  // namespace rm
