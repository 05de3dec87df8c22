// respmon_amd/csrc/rm_magnify.h -- the magnified video in one pass (rm_magnify)
//
//   m[t] = f[t] + raw[t]        f: the frame as the calibration reads it (uint8: k * (1./255), transforms.py:20-23; BGR: base.py:230 first)
//                               raw[t] = pyrUp^S(C_S[t]): raw_bandpassed_data of rm_eulerian_magnification_bandpass, bit for bit
//
// The reference adds the band-passed levels into the video's own Laplacian pyramid (transforms.py:170) and leaves the collapse of that
// pyramid commented out (transforms.py:181): collapse(vid_pyramid) is this video in exact arithmetic, because the Laplacian pyramid of
// a frame telescopes back to the frame.  Here the sum is formed at full resolution, one float64 addition per pixel.
//
// Output: RM_F64 m; RM_F32 (float)m, round to nearest; RM_U8 m clamped to [0, 1] and then rm_float_to_uint8's rule (transforms.py:26-29,
// the C truncation of m * 255; NaN -> 0 as there).  THE CLAMP IS OURS: the reference has no writer for this video, and a magnified pixel
// leaves [0, 1] wherever the amplified motion is larger than the head room of the frame -- without the clamp such a pixel would wrap
// around modulo 256.  RM_U16: the same clamp, then rm_float_to_uint16's rule (the C truncation of m * 65535).
//
//   * k_magnify<S, Tin, Tout>: a wave owns a 64 x 16 tile and MAG_FC consecutive UNIQUE frames u (the band-passed signal is even in time,
//     rm_kernels.h sym_frame: raw[T - u] is raw[u] again).  Per u it stages the tile's level-S footprint of C_S[u], evaluates raw with
//     TileEval (rm_tile_eval.h: every pair, no pruning), parks the 1024 values in the wave's LDS slice and reads them back in the
//     order of the frame's memory -- V = 16 / max(sizeof input pixel, sizeof output pixel) consecutive pixels per lane, the lanes of a
//     pass side by side -- then, for t = u and t = T - u: load, add, convert, store.  Frame tiles are read once and the output written
//     once (non-temporal, 16 bytes per lane on the wider side where the rows are 16-byte aligned: W a multiple of V); nothing else
//     of size [T, H, W] exists.  The frame tiles are requested before the evaluation starts, so they travel while it runs.
//   * k_magnify_plain<Tin, Tout>: the same sum behind a materialised raw (skip 0, skip 5 and deeper, images too small for TileEval),
//     and the conversion alone where nothing is filtered (raw == 0).
//
// In colour (rm_magnify_bgr: Tin = Tout = bgr8_t, BGR frames in, BGR video out), for every channel c of pixel p:
//
//   out[t, p, c] = u8(clamp01((double)frames[t, p, c] * (1./255) + raw[t, p]))      clamp01, u8: mag_out<uint8_t> below
//
// raw is the band-passed motion of the gray image cvtColor makes of the frame, as everywhere else, and the SAME raw goes onto all three
// channels: cvtColor's weights (0.114, 0.587, 0.299) are the Y row of YIQ, and in the YIQ -> RGB matrix the Y column is (1, 1, 1), so
// adding raw to B, G and R is the classical magnification of luma with chroma left alone.  One float64 multiplication, one addition
// and one multiplication per channel, each rounded once.  Both kernels have that instance: k_magnify keeps a lane's 16 pixels packed
// as loaded (three 16-byte pieces per served frame, 2 x 48 bytes in flight) and widens a byte only when the raw values are at hand.
//   - three equal channels in give three equal channels out, each the RM_U8 output of rm_magnify on that buffer bit for bit (the
//     integer cvtColor of (k, k, k) is k);
//   - where nothing is filtered (skip >= levels - 1) raw is zero and a byte k becomes u8(k * (1./255)): the reference's
//     float_to_uint8(uint8_to_float(k)), which is k - 1 on 24 of the 256 levels.  NOT an identity copy: the rule of the gray path, kept.
#pragma once
#include "rm_down_chain_u8.h"   // bgr8_t
#include "rm_tile_eval.h"

namespace rm {

#ifdef RM_HIPEMU
template <typename T> inline void mag_nt_store(T v, T *p) { *p = v; }
#else
template <typename T> __device__ __forceinline__ void mag_nt_store(T v, T *p) { __builtin_nontemporal_store(v, p); }
#endif

// a pixel of a frame buffer: its storage element E, elements per pixel, and the widening the calibration applies (load_px)
template <typename T> struct MagPx;
template <> struct MagPx<uint8_t> {
    using E = uint8_t; static constexpr int C = 1;
    static __device__ __forceinline__ double widen(const E *e) { return (double)e[0] * (1.0 / 255); }
};
template <> struct MagPx<uint16_t> {   // RM_U16: uint16_to_float's k * (1./65535)
    using E = uint16_t; static constexpr int C = 1;
    static __device__ __forceinline__ double widen(const E *e) { return u16_to_f64(e[0]); }
};
template <> struct MagPx<__half> {
    using E = uint16_t; static constexpr int C = 1;
    static __device__ __forceinline__ double widen(const E *e)
    {
        __half h;
        __builtin_memcpy(&h, e, 2);
        return (double)__half2float(h);
    }
};
template <> struct MagPx<float> {
    using E = float; static constexpr int C = 1;
    static __device__ __forceinline__ double widen(const E *e) { return (double)e[0]; }
};
template <> struct MagPx<double> {
    using E = double; static constexpr int C = 1;
    static __device__ __forceinline__ double widen(const E *e) { return e[0]; }
};
template <> struct MagPx<bgr8_t> {   // cv2.cvtColor(BGR2GRAY), base.py:230 (k_bgr_to_gray), then uint8_to_float
    using E = uint8_t; static constexpr int C = 3;
    static __device__ __forceinline__ double widen(const E *e)
    {
        const int b = e[0], g = e[1], r = e[2];
        return (double)(uint8_t)((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14) * (1.0 / 255);
    }
};

template <typename Tout> __device__ __forceinline__ Tout mag_out(double m);
template <> __device__ __forceinline__ double mag_out<double>(double m) { return m; }
template <> __device__ __forceinline__ float mag_out<float>(double m) { return (float)m; }
template <> __device__ __forceinline__ uint8_t mag_out<uint8_t>(double m)
{
    const double c = m < 0.0 ? 0.0 : (m > 1.0 ? 1.0 : m);   // (NaN passes through: f64_to_u8_trunc maps it to 0)
    return f64_to_u8_trunc(c * 255);
}
template <> __device__ __forceinline__ uint16_t mag_out<uint16_t>(double m)   // the same clamp, for the same reason, then float_to_uint16's rule
{
    const double c = m < 0.0 ? 0.0 : (m > 1.0 ? 1.0 : m);
    return f64_to_u16_trunc(c * 65535);
}

constexpr int MAG_FC = 8;                      // unique frames per work item
constexpr int MAG_LDS_DOUBLES = CT_H * CT_W;   // the wave's slice: the footprints of TileEval, then the tile's 1024 values

template <typename Tin, typename Tout> struct MagGeom {
    using E = typename MagPx<Tin>::E;
    static constexpr int C = MagPx<Tin>::C;
    static constexpr int WIDE = (int)(sizeof(E) > sizeof(Tout) ? sizeof(E) : sizeof(Tout));
    static constexpr int V = 16 / WIDE;                    // pixels per lane and pass
    static constexpr int NP = CT_H * CT_W / (64 * V);      // passes per tile
    static constexpr int NE = V * C;                       // storage elements of a lane's pixels
};

template <> struct MagGeom<bgr8_t, bgr8_t> {   // colour: 16 pixels = 48 bytes per lane on both sides, one pass per tile
    using E = uint8_t;
    static constexpr int C = 3, V = 16, NP = CT_H * CT_W / (64 * V), NE = V * C;
};
template <typename Tin, typename Tout> constexpr bool mag_colour = false;
template <> inline constexpr bool mag_colour<bgr8_t, bgr8_t> = true;   // (inline: rm_phase_kernels.h includes this header for mag_out, a second unit)

// the V pixels of one lane and pass, as stored
template <typename Tin, typename Tout> struct MagIn { typename MagGeom<Tin, Tout>::E e[MagGeom<Tin, Tout>::NE]; };
template <> struct MagIn<bgr8_t, bgr8_t> { uint32_t w[MagGeom<bgr8_t, bgr8_t>::NE / 4]; };   // ... kept packed: byte j is bits 8 (j % 4) .. of w[j / 4]
typedef RM_VEC(uint32_t, 4) MagU32x4;

// the colour form of the two functions below: the lane's 48 bytes as 12 dwords
template <bool VEC>
__device__ __forceinline__ void mag_load_bgr(const uint8_t *pe, int nvalid, MagIn<bgr8_t, bgr8_t> &in)
{
    constexpr int NE = MagGeom<bgr8_t, bgr8_t>::NE;
    if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < NE / 16; ++k) {
            const MagU32x4 v = __builtin_nontemporal_load(reinterpret_cast<const MagU32x4 *>(pe) + k);
#pragma unroll
            for (int i = 0; i < 4; ++i) in.w[4 * k + i] = v[i];
        }
    } else {
#pragma unroll
        for (int k = 0; k < NE / 4; ++k) in.w[k] = 0;
#pragma unroll
        for (int j = 0; j < NE; ++j) if (j / 3 < nvalid) in.w[j >> 2] |= (uint32_t)pe[j] << (8 * (j & 3));
    }
}

template <bool VEC>
__device__ __forceinline__ void mag_store_bgr(uint8_t *po, int nvalid, const MagIn<bgr8_t, bgr8_t> &in, const double *raw)
{
    constexpr int NE = MagGeom<bgr8_t, bgr8_t>::NE;
    uint32_t o[NE / 4];
#pragma unroll
    for (int k = 0; k < NE / 4; ++k) o[k] = 0;
#pragma unroll
    for (int j = 0; j < NE; ++j) {   // byte j: channel j % 3 of pixel j / 3
        const uint8_t k = (uint8_t)(in.w[j >> 2] >> (8 * (j & 3)));
        o[j >> 2] |= (uint32_t)mag_out<uint8_t>(MagPx<uint8_t>::widen(&k) + raw[j / 3]) << (8 * (j & 3));
    }
    if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < NE / 16; ++k)
            mag_nt_store(MagU32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]}, reinterpret_cast<MagU32x4 *>(po) + k);
    } else {
#pragma unroll
        for (int j = 0; j < NE; ++j) if (j / 3 < nvalid) po[j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
    }
}

// p: the lane's first pixel; VEC: the chunk is whole and aligned to its size; otherwise `nvalid` pixels exist (the rest read as zero)
template <typename Tin, typename Tout, bool VEC>
__device__ __forceinline__ void mag_load(const Tin *p, int nvalid, MagIn<Tin, Tout> &in)
{
    using G = MagGeom<Tin, Tout>;
    using E = typename G::E;
    const E *pe = reinterpret_cast<const E *>(p);
    if constexpr (mag_colour<Tin, Tout>) {
        mag_load_bgr<VEC>(pe, nvalid, in);
    } else if constexpr (VEC && G::C == 1) {
        typedef RM_VEC(E, G::NE) Vec;
        const Vec v = __builtin_nontemporal_load(reinterpret_cast<const Vec *>(pe));
#pragma unroll
        for (int i = 0; i < G::NE; ++i) in.e[i] = v[i];
    } else if constexpr (VEC && (G::NE * sizeof(E)) % 16 == 0) {   // BGR, 16 pixels: three 16-byte pieces
        typedef RM_VEC(E, 16 / sizeof(E)) Vec;
        constexpr int PER = 16 / sizeof(E);
#pragma unroll
        for (int k = 0; k < G::NE / PER; ++k) {
            const Vec v = __builtin_nontemporal_load(reinterpret_cast<const Vec *>(pe) + k);
#pragma unroll
            for (int i = 0; i < PER; ++i) in.e[k * PER + i] = v[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < G::NE; ++i) in.e[i] = (i / G::C < nvalid) ? pe[i] : E(0);
    }
}

template <typename Tin, typename Tout, bool VEC>
__device__ __forceinline__ void mag_store(Tout *p, int nvalid, const MagIn<Tin, Tout> &in, const double *raw)
{
    using G = MagGeom<Tin, Tout>;
    if constexpr (mag_colour<Tin, Tout>) {
        mag_store_bgr<VEC>(reinterpret_cast<uint8_t *>(p), nvalid, in, raw);
    } else {
        Tout o[G::V];
#pragma unroll
        for (int i = 0; i < G::V; ++i) o[i] = mag_out<Tout>(MagPx<Tin>::widen(in.e + i * G::C) + raw[i]);
        if constexpr (VEC) {
            typedef RM_VEC(Tout, G::V) Vec;
            Vec v;
#pragma unroll
            for (int i = 0; i < G::V; ++i) v[i] = o[i];
            mag_nt_store(v, reinterpret_cast<Vec *>(p));
        } else {
#pragma unroll
            for (int i = 0; i < G::V; ++i) if (i < nvalid) p[i] = o[i];
        }
    }
}

// grid: ntiles * ceil(Th / MAG_FC) single-wave workgroups, block = chunk * ntiles + tile (neighbours in the grid work on neighbouring
// tiles of the same frames); dynamic LDS: MAG_LDS_DOUBLES doubles.  vec: rows and base addresses allow the aligned whole-chunk accesses.
// SYM = 1: the band-passed signal is even in time (the FFT operator of rm_magnify), C_S holds the unique frames.  SYM = 0: every frame
// owns its row of C_S (Th = T; the causal filter of rm_stream_push): no second served frame, one frame tile in flight instead of two.
template <int S, typename Tin, typename Tout, int SYM = 1>
__global__ __launch_bounds__(64) void k_magnify(const double *cS, ChainGeom g, int T, int ntiles, const Tin *frames, Tout *out, int vec)
{
    using F = TileFoot<S>;
    using G = MagGeom<Tin, Tout>;
    static_assert(F::TOTAL <= MAG_LDS_DOUBLES, "the footprint slice must fit under the tile's values");
    HIP_DYNAMIC_SHARED(double, lds)
    const int lane = threadIdx.x;
    const int tile = (int)blockIdx.x % ntiles, chunk = (int)blockIdx.x / ntiles;
    const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    const int Th = SYM ? sym_frames(T) : T;
    const int u0 = chunk * MAG_FC, u1 = min(Th, u0 + MAG_FC);
    const int H0 = g.h[0], W0 = g.w[0];
    const size_t fs = (size_t)g.h[S] * g.w[S], npix = (size_t)H0 * W0;
    TileSetup<S> ts;
    tile_setup<S>(g, tx, ty, lane, ts);
    // where this lane's pixels of pass p lie: element e = (64 p + lane) V of the tile's 64 x 16 values, row e / 64, column e % 64
    size_t px_off[G::NP];
    int nvalid[G::NP];
#pragma unroll
    for (int p = 0; p < G::NP; ++p) {
        const int e = (64 * p + lane) * G::V;
        const int y = CT_H * ty + (e >> 6), x = CT_W * tx + (e & 63);
        nvalid[p] = y < H0 ? min(max(W0 - x, 0), G::V) : 0;
        px_off[p] = (size_t)min(y, H0 - 1) * W0 + min(x, W0 - 1);
    }
    for (int u = u0; u < u1; ++u) {
        const int t2 = (SYM && u >= 1 && 2 * u != T) ? T - u : -1;   // (uniform) the second frame this evaluation serves
        const double *src = cS + (size_t)u * fs;
        double stg[F::PF];
#pragma unroll
        for (int p = 0; p < F::PF; ++p) stg[p] = src[ts.off_g[p]];
        // the frame tiles travel while the evaluation runs
        MagIn<Tin, Tout> in_a[G::NP], in_b[SYM ? G::NP : 1];
        const Tin *fa = frames + (size_t)u * npix, *fb = frames + (size_t)(t2 >= 0 ? t2 : u) * npix;
#pragma unroll
        for (int p = 0; p < G::NP; ++p) {
            if (vec) {
                if (nvalid[p] > 0) {
                    mag_load<Tin, Tout, true>(fa + px_off[p], G::V, in_a[p]);
                    if constexpr (SYM) if (t2 >= 0) mag_load<Tin, Tout, true>(fb + px_off[p], G::V, in_b[p]);
                }
            } else {
                mag_load<Tin, Tout, false>(fa + px_off[p], nvalid[p], in_a[p]);
                if constexpr (SYM) if (t2 >= 0) mag_load<Tin, Tout, false>(fb + px_off[p], nvalid[p], in_b[p]);
            }
        }
        wave_sync();   // the previous frame's reads of the slice are behind us
#pragma unroll
        for (int p = 0; p < F::PF; ++p) if (lane + 64 * p < F::NST) lds[F::off(S) + lane + 64 * p] = stg[p];
        wave_sync();
        double v[16];
        tile_eval<S>(ts, lds, lane, v);
        wave_sync();   // every lane has its values: the slice may be overwritten
        {   // lane (column pair cp, row half rg) holds rows 8 rg .. 8 rg + 7 of columns 2 cp, 2 cp + 1 (tile_setup)
            double *d = lds + (size_t)(8 * (lane >> 5)) * CT_W + 2 * (lane & 31);
#pragma unroll
            for (int r = 0; r < 8; ++r) *reinterpret_cast<F64Pair *>(d + r * CT_W) = F64Pair{v[r], v[8 + r]};
        }
        wave_sync();
#pragma unroll
        for (int p = 0; p < G::NP; ++p) {
            double raw[G::V];
            const double *rp = lds + (64 * p + lane) * G::V;
#pragma unroll
            for (int i = 0; i < G::V; ++i) raw[i] = rp[i];
            if (nvalid[p] > 0) {
                if (vec) {
                    mag_store<Tin, Tout, true>(out + (size_t)u * npix + px_off[p], G::V, in_a[p], raw);
                    if constexpr (SYM) if (t2 >= 0) mag_store<Tin, Tout, true>(out + (size_t)t2 * npix + px_off[p], G::V, in_b[p], raw);
                } else {
                    mag_store<Tin, Tout, false>(out + (size_t)u * npix + px_off[p], nvalid[p], in_a[p], raw);
                    if constexpr (SYM) if (t2 >= 0) mag_store<Tin, Tout, false>(out + (size_t)t2 * npix + px_off[p], nvalid[p], in_b[p], raw);
                }
            }
        }
    }
}

// out[t, p] = convert(f[t, p] + raw[sym_frame(t), p]) (colour: per channel of f[t, p], the header of this file); raw: the unique frames [T / 2 + 1][npix], or null where nothing is filtered (raw == 0).
// SYM = 0: raw is [T][npix], a row per frame.  blockIdx.y = t.
template <typename Tin, typename Tout, int SYM = 1>
__global__ __launch_bounds__(256) void k_magnify_plain(const Tin *frames, const double *raw, int T, size_t npix, Tout *out)
{
    const int t = (int)blockIdx.y;
    const Tin *f = frames + (size_t)t * npix;
    const double *r = raw ? raw + (size_t)(SYM ? sym_frame(t, T) : t) * npix : nullptr;
    Tout *o = out + (size_t)t * npix;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
        const typename MagPx<Tin>::E *e = reinterpret_cast<const typename MagPx<Tin>::E *>(f + p);
        const double rv = r ? r[p] : 0.0;
        if constexpr (mag_colour<Tin, Tout>)
            o[p] = bgr8_t{mag_out<uint8_t>(MagPx<uint8_t>::widen(e) + rv), mag_out<uint8_t>(MagPx<uint8_t>::widen(e + 1) + rv),
                          mag_out<uint8_t>(MagPx<uint8_t>::widen(e + 2) + rv)};
        else
            o[p] = mag_out<Tout>(MagPx<Tin>::widen(e) + rv);
    }
}

}  // namespace rm
