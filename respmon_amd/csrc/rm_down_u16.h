// respmon_amd/csrc/rm_down_u16.h -- uint16 frame buffers (RM_U16) in the fused Gaussian chains: the traits and the unpack of a pixel
//
// A 16-bit gray plane per frame is what infrared, thermal and depth cameras deliver (Y16, or Y10 / Y12 / Y14 in 16-bit words).  The rule
// is  uint16_to_float(k) = (double)k * (1./65535)  -- ONE float64 multiplication by the rounded constant, the shape of uint8_to_float
// (transforms.py:20-23) -- and every kernel applies it as it reads the buffer, so the results are bit-identical to the float64 buffer
// that holds k * (1./65535) (include/respmon_hip.h RM_U16).
//
// The chains are the ones of rm_down_chain_u8.h (all-register, W % 16 == 0) and rm_down_chain.h (LDS front end: ragged widths and
// whatever the register geometry refuses), instantiated for uint16_t in a unit of their own (rm_down_u16.hip).  The geometry is the
// float16 one -- a lane owns 16 adjacent pixels in two 16-byte loads per row -- and prefetch depth, row ring and hot blocks start from
// the float16 settings.  These declarations sit in a header of their own, outside the sources hashed into
// rm_debug_kernel_source_stamp (Makefile STAMP_SRCS): no existing instantiation changes, and the committed PMC figures keep their stamp.
//
// The unpack is the new instruction work: a 16-bit extract from the loaded word, an EXACT integer -> float64 conversion and one
// v_mul_f64 per pixel, in place of the half chain's two converts.
//   - No table as the uint8 chain has (RM_U8_LUT): 65 536 doubles are 512 KB.
//   - Nothing through a float or a half: 65 534 of the 65 536 values k * (1./65535) are not float32 numbers.
#pragma once
#include "rm_down_chain_u8.h"

namespace rm {

template <> struct VecTraits<uint16_t> { static constexpr int V = 8; };

// The conversion is v_cvt_f64_u32.  The other exact form -- k or-ed into the mantissa of 2^52, then 2^52 subtracted, which trades the
// convert for a v_add_f64 and a constant register pair -- was built and measured beside it and is no faster (it lives on
// as u16_magic_t in bench_micro/dc16_bench.hip, where the two are timed in one process).
template <> __device__ __forceinline__ double unpack_px<uint16_t>(const Raw16 &r, int e)
{
    const unsigned int wd = (e >> 1) == 0 ? r.x : (e >> 1) == 1 ? r.y : (e >> 1) == 2 ? r.z : r.w;
    const unsigned int k = (e & 1) ? (wd >> 16) : (wd & 0xffffu);
    return (double)k * (1.0 / 65535);
}

template <> struct RegTraits<uint16_t> { static constexpr int NLD = 2, PF = RM_F16_PREFETCH, RD = RM_F16_RING; static constexpr bool HOT = RM_F16_HOT != 0, DMA = RM_NARROW_DMA_ON != 0; };

}  // namespace rm
