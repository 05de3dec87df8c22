/*
 * include/respmon_hip.h -- C-ABI of librespmon_hip.so, the MI355X (gfx950) implementation of
 * respmon's Eulerian-magnification calibration and ROI motion-extraction hot path.
 *
 * The reference (kevroy314/respmon) is pure Python and has no FFI layer; the "interface each
 * entry point replaces" is therefore the Python function (and the cv2 / scipy / numpy calls
 * under it) cited next to each declaration, paths relative to the reference root.
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *  - plain C types only; every pointer named *_dev is a DEVICE pointer (HBM) unless the
 *    comment says host; images are row-major, videos are [T,H,W] with frame stride H*W.
 *  - every function returns int: RM_OK (0) or a negative RM_E_* code; rm_last_error_string()
 *    gives the text for the calling thread's last failure.  RM_NO_CONTOUR (+1) is the
 *    reference's `return None` (base.py:569-570).
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls enqueue work on
 *    it; functions that return host results synchronise that stream before returning.
 *  - a context is not thread-safe; use one per stream / GPU.
 *  - developer switches, hooks for the tests and diagnostics counters are NOT part of this interface: include/respmon_hip_debug.h.
 */
#ifndef RESPMON_HIP_H
#define RESPMON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RM_OK 0
#define RM_NO_CONTOUR 1
#define RM_SPARSE_FALLBACK 2 /* rm_heat_sparse_merge_roi: a packet overflowed, use the dense all-reduce instead */
#define RM_E_BADARG (-1)
#define RM_E_HIP (-2)
#define RM_E_NOMEM (-3)
#define RM_E_UNSUPPORTED (-4)
#define RM_E_INTERNAL (-5)
#define RM_E_COMM (-6)     /* RCCL: library missing, communicator or collective failed */
#define RM_E_BUSY (-7)     /* rm_locate_submit: every ticket of the context is waiting for its rm_locate_result */

/* element type of a frame buffer handed to the library */
#define RM_U8 0  /* gray uint8; the kernels apply uint8_to_float's  k * (1./255)  (transforms.py:20-23) */
#define RM_F16 1 /* IEEE half, widened exactly */
#define RM_F32 2 /* float, widened exactly */
#define RM_F64 3 /* double: the reference's calibration_buffer dtype (base.py:119-120) */
/* Frame BUFFERS only -- the `frames` argument of rm_calibrate, rm_locate, rm_locate_submit, rm_locate_streams, rm_locate_sharded,
 * rm_shard_pyramid, rm_eulerian_magnification_bandpass and rm_magnify: [T,H,W,3] uint8 in cv2.VideoCapture's channel order.  The kernels apply
 * base.py:230-231 (cv2.cvtColor(BGR2GRAY), then uint8_to_float) as they read the buffer: results are bit-identical to the same call on
 * the RM_U8 buffer that rm_bgr_to_gray makes of it.  Every other entry point takes gray frames and answers RM_E_BADARG. */
#define RM_BGR8 4
/* gray uint16: one 16-bit plane per frame, as infrared, thermal and depth cameras deliver it (Y16, or Y10 / Y12 / Y14 in 16-bit words).
 * The kernels apply  uint16_to_float(k) = (double)k * (1./65535)  -- ONE float64 multiplication by the rounded constant, the shape of
 * uint8_to_float -- as they read the buffer.  Every entry point that takes a gray dtype takes it, and returns bit for bit what the
 * same call returns on the RM_F64 buffer that holds k * (1./65535) (the contract RM_F16 / RM_F32 have: "widened exactly").
 *   - The low byte matters: 65 534 of the 65 536 values k * (1./65535) are not representable in float32, so nothing on this path
 *     converts through a float or a half.
 *   - Left-shifted samples: a 10 / 12 / 14-bit camera may store its samples shifted left by n bits or not.  Scaling every input by
 *     2^n scales every float64 on the path exactly: the heat map comes out scaled by 2^n bit for bit, and the ROI, the normalised
 *     uint8 heat map and the peaks of the mean signal are identical.  There is no white-level argument.  The optical-flow path alone
 *     cares: rm_roi_to_uint8 makes trunc(x * 255) of a frame, so flow wants white at 65535 (shift such samples up first).
 *   - (257 k) * (1./65535) is NOT k * (1./255) for 24 of the 256 k: an 8-bit stream widened to 16 bits does not reproduce the RM_U8
 *     results bit for bit (the ROI normally agrees, the heat map does not).
 * (The codes 5 and 7 stay unassigned.) */
#define RM_U16 6

/* rm_calibrate flags */
#define RM_FLAG_NO_PRUNE 1u      /* evaluate every (tile, frame) of the collapse passes (A/B + verification) */
#define RM_FLAG_UNFUSED_DOWN 2u  /* build the Gaussian levels one pyrDown launch per level */
#define RM_FLAG_UNFUSED_SMALL 16u /* build / collapse the small pyramid with one launch per level (A/B + fallback path) */
#define RM_FLAG_CONTOUR_CLIP_FRAME 32u /* rm_locate: cv2.findContours as OpenCV <= 3.1 did it (see rm_set_contour_clip_frame) */
#define RM_FLAG_FILTER_LAPLACIANS 64u /* build the small pyramid in the reference's order -- Laplacians first, filter them, collapse (bit for bit equal to the per-level
                                         path) -- instead of the filter-first form (filter G_S, then Laplacians + collapse in one kernel; equal to ~1e-15).
                                         Frames whose level skip_levels_at_top is a single pixel: the Laplacians (zero but for rounding there) are
                                         taken from G_S before the filter in either form; what a window or rm_shard_pyramid stores does not change. */
#define RM_FLAG_DENSE_SUM 128u    /* take the masked time sum with the dense kernel (recomputes every value, no value store) ... */
#define RM_FLAG_SPARSE_SUM 256u   /* ... or with the sparse path (evaluate + store the pairs that can fall below `top`).  Neither: decided on
                                     the device from what THIS call's selection kept (nothing is remembered between calls): dense when the
                                     kept pairs outnumber the value store's slots, or at skip <= 2 when more than half are kept.
                                     Bit-identical results. */

typedef struct rm_ctx rm_ctx;

/* ---- context -------------------------------------------------------------------------- */
int rm_ctx_create(int device, rm_ctx **out);
int rm_ctx_destroy(rm_ctx *ctx);
const char *rm_last_error_string(void);
int rm_abi_version(void);
/* bytes of device workspace currently held by the context */
size_t rm_ctx_workspace_bytes(const rm_ctx *ctx);

/* ---- measurement hook for bench.py: mode 1 brackets only the frame-buffer kernel with hipEvents on the
 *      caller's stream (cheap enough for the timed region), mode 2 brackets every phase of rm_calibrate /
 *      rm_heatmap_to_roi (each bracket costs ~10 us of stream idle time), mode 0 turns it off.  rm_profile_read waits for them and returns the summed
 *      milliseconds since the last read: ms_host[0] = the kernel that reads the [T,H,W] frame buffer
 *      (the roofline kernel), [1] = remaining pyramid + temporal kernels, [2] = collapse passes,
 *      [3] = heatmap -> ROI (device part + host contour stage); *n_host = rm_calibrate calls the sums cover
 *      (mode 2: every call; mode 1: every 8th call is bracketed, the others run without the two event records). */
#define RM_PROFILE_PHASES 4
int rm_profile_enable(rm_ctx *ctx, int mode);
int rm_profile_read(rm_ctx *ctx, double *ms_host, int *n_host);

/* ---- dtype helpers: transforms.py:20-23 uint8_to_float, transforms.py:26-29 float_to_uint8 */
int rm_uint8_to_float(rm_ctx *ctx, const uint8_t *src_dev, double *dst_dev, size_t n, void *stream);
int rm_float_to_uint8(rm_ctx *ctx, const double *src_dev, uint8_t *dst_dev, size_t n, void *stream);
/* ... and the 16-bit pair (RM_U16 above): dst = (double)k * (1./65535);  dst = the low 16 bits of the C truncation of v * 65535,
 * NaN and products outside int32 -> 0 (the rule of rm_float_to_uint8 with 65535 for 255) */
int rm_uint16_to_float(rm_ctx *ctx, const uint16_t *src_dev, double *dst_dev, size_t n, void *stream);
int rm_float_to_uint16(rm_ctx *ctx, const double *src_dev, uint16_t *dst_dev, size_t n, void *stream);

/* ---- pyramid.py building blocks (materialising forms, API parity + tests) ------------- */
/* cv2.pyrDown on every frame of src[T,h,w] -> dst[T,(h+1)/2,(w+1)/2] float64.  pyramid.py:14 */
int rm_pyr_down(rm_ctx *ctx, const void *src_dev, int src_dtype, int T, int h, int w,
                double *dst_dev, void *stream);
/* cv2.pyrUp(src, dstsize=(dw,dh)) on every frame, fused with the reference's add/subtract:
 *   mode 0: dst = up(src)                      pyramid.py:55 with a zero level
 *   mode 1: dst = other - up(src)              pyramid.py:24-26  (Laplacian level)
 *   mode 2: dst = up(src) + other              pyramid.py:55     (collapse step)
 * `other_dev` is [T,dh,dw] (ignored for mode 0); dst may alias other. */
int rm_pyr_up(rm_ctx *ctx, const double *src_dev, int T, int sh, int sw, double *dst_dev, int dh, int dw,
              int mode, const double *other_dev, void *stream);
/* pyramid.py:31-48 create_laplacian_video_pyramid: level_ptrs_host[l] -> device [T,h_l,w_l] float64,
 * h_0=H, h_{l+1}=(h_l+1)/2.  All `levels` arrays are written. */
int rm_create_laplacian_video_pyramid(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W,
                                      int levels, double *const *level_ptrs_host, void *stream);
/* pyramid.py:60-69 collapse_laplacian_video_pyramid: result into out_dev[T,H,W] (may be level 0). */
int rm_collapse_laplacian_video_pyramid(rm_ctx *ctx, const double *const *level_ptrs_host, int T, int H, int W,
                                        int levels, double *out_dev, void *stream);

/* ---- transforms.py:82-102 temporal_bandpass_filter_fft -------------------------------- */
/* out[s,p] = amplification * sum_t M[s,t] data[t,p], M = the reference's packed-rfft / mask /
 * Re(ifft) operator (quirk kept).  data/out: [T, npix] float64. */
int rm_temporal_bandpass_filter_fft(rm_ctx *ctx, const double *data_dev, int T, size_t npix, double fps,
                                    double freq_min, double freq_max, double amplification,
                                    double *out_dev, void *stream);
/* the operator itself (host, row-major [T,T], without the amplification) and the band bounds */
int rm_temporal_operator(int T, double fps, double freq_min, double freq_max, double *M_host,
                         int *bound_low, int *bound_high);

/* ---- np.average(video, axis=0) (base.py:562, 579, 587, 589: heatmap and the panels of the calibration image):
 *      out_dev[npix] float64 = (sum over t, in t order, of data[t, :]) / T for a [T, npix] array of any frame dtype. */
int rm_time_average(rm_ctx *ctx, const void *data_dev, int dtype, int T, size_t npix, double *out_dev, void *stream);

/* ---- transforms.py:72-79 temporal_bandpass_filter, transforms.py:53-55 butter_bandpass_filter_fast:
 *      out = scipy.signal.lfilter(b, a, data, axis=0) * scale on data[T, npix] float64 (transposed direct form II,
 *      the operation order of scipy's C loop).  b_host / a_host: ncoef coefficients each (ncoef <= 16; the
 *      reference's order-6 Butterworth band-pass has 13), designed on the host with scipy.signal.butter exactly
 *      as transforms.py:38-44 does.  SURVEY 8f row f4. */
int rm_lfilter(rm_ctx *ctx, const double *data_dev, int T, size_t npix, const double *b_host, const double *a_host,
               int ncoef, double scale, double *out_dev, void *stream);

/* ---- the same band-pass design as a cascade of second-order sections (scipy.signal.butter(..., output='sos')):
 *      out = scipy.signal.sosfilt(sos, data, axis=0[, zi]) * scale on data[T, npix] float64, in the operation order of scipy's loop:
 *          cur = x[t];  for every section s = (b0, b1, b2, a0 == 1, a1, a2), in order:
 *              new = b0*cur + z[s][0];  z[s][0] = (b1*cur - a1*new) + z[s][1];  z[s][1] = b2*cur - a2*new;  cur = new
 *          y[t] = cur * scale                                       every operation rounded once
 *      sos_host[nsec][6], 1 <= nsec <= 8.  zi_host NULL: every element starts at rest (z = 0).  zi_host[nsec][2] (the table of
 *      scipy.signal.sosfilt_zi): element p starts at z[s][k] = zi[s][k] * data[0, p], the steady state of a constant input data[0, p]
 *      -- scipy's sosfilt(sos, data, axis=0, zi=zi[:, :, None] * data[0]).
 *      Why this exists beside rm_lfilter: in `ba` form the order-6 band-pass of transforms.py:72-79 has poles outside the unit circle
 *      at camera rates in float64 (fps 30, 0.1-0.5 Hz: largest pole 1.056, the output of noise in [0, 1] reaches 1.7e19 within 2 000
 *      samples); as sections its largest pole is 0.9963 and the output stays below 0.3.
 *      RM_E_UNSUPPORTED: nsec > 8;  RM_E_BADARG: nsec < 1, a section with a0 != 1, data_dev == out_dev, NULL pointers, T < 1. */
int rm_sosfilt(rm_ctx *ctx, const double *data_dev, int T, size_t npix, const double *sos_host, int nsec, const double *zi_host,
               double scale, double *out_dev, void *stream);

/* ---- transforms.py:184-192 on a materialised array: minmax_host = {raw.min(), raw.max()} (may be NULL);
 *      masked_dev (may be NULL) = raw with every value >= max - (max - min) * threshold replaced by min.
 *      Lets eulerian_magnification_bandpass run with ANY temporal_filter_function (transforms.py:146). */
int rm_threshold_mask(rm_ctx *ctx, const double *raw_dev, size_t n, double threshold, double *masked_dev,
                      double *minmax_host, void *stream);

/* ---- transforms.py:144-198 eulerian_magnification_bandpass (materialised outputs) ------ */
/* masked_dev / raw_dev: [T,H,W] float64 (either may be NULL); minmax_host[2] = {min, max} of raw. */
int rm_eulerian_magnification_bandpass(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W,
                                       double fps, double freq_min, double freq_max, double amplification,
                                       int pyramid_levels, int skip_levels_at_top, double threshold,
                                       double *masked_dev, double *raw_dev, double *minmax_host, void *stream);

/* ---- the magnified video: original frames plus the amplified band-passed motion ------- */
/* transforms.py:170 adds the band-passed levels into the video's Laplacian pyramid; the collapse of that pyramid is the commented
 * line transforms.py:181.  In exact arithmetic that collapse is frame + raw (a frame's Laplacian pyramid telescopes back to the
 * frame); this entry forms
 *     m[t] = f[t] + raw[t]                 one float64 addition per pixel
 * with f[t] the frame as the calibration reads it (RM_U8: k * (1./255); RM_BGR8: cvtColor first) and raw[t] the raw_dev of
 * rm_eulerian_magnification_bandpass for the same arguments, bit for bit -- in one pass over the frame buffer, without a [T,H,W]
 * float64 intermediate (1 <= skip_levels_at_top <= 4; other depths materialise raw's unique frames in the workspace first).
 * out_dev[T,H,W] of out_dtype:  RM_F64: m;  RM_F32: (float)m, round to nearest;  RM_U8: m clamped to [0, 1], then
 * rm_float_to_uint8's rule (transforms.py:26-29: the C truncation of m * 255; NaN -> 0).  The clamp is this library's: the
 * reference has no writer for this video, and without it a pixel pushed outside [0, 1] would wrap around modulo 256.
 * RM_U16: the same clamp, then rm_float_to_uint16's rule (the C truncation of m * 65535).
 * skip_levels_at_top >= pyramid_levels - 1 (nothing is filtered): raw is zero and the output is f converted (an RM_U16 buffer
 * magnified to RM_U16 comes back as u16(k * (1./65535) * 65535) per level: the rule, not an identity copy).
 * RM_E_BADARG: any other out_dtype, out_dev overlapping the frame buffer, NULL pointers, T < 1;  RM_E_UNSUPPORTED: T > 4096 as
 * in rm_calibrate.  Asynchronous on `stream`. */
int rm_magnify(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W,
               double fps, double freq_min, double freq_max, double amplification,
               int pyramid_levels, int skip_levels_at_top,
               void *out_dev, int out_dtype, void *stream);

/* ---- the magnified video in colour: BGR frames in, BGR video out ------------------------ */
/* For every frame t, pixel p and channel c of an RM_BGR8 frame buffer
 *     out[t,p,c] = u8( clamp01( (double)frames[t,p,c] * (1./255)  +  raw[t,p] ) )
 * with raw the raw_dev of rm_eulerian_magnification_bandpass on the same RM_BGR8 buffer with the same arguments, bit for bit (the
 * band-passed motion of the gray image cvtColor makes of the frame, as everywhere else), and clamp01 / u8 those of rm_magnify's
 * RM_U8 output: the clamp to [0, 1], then rm_float_to_uint8's C truncation of m * 255.  One float64 multiplication, one addition
 * and one multiplication per channel, each rounded once.
 * The same raw goes onto all three channels: cvtColor's weights (0.114, 0.587, 0.299) are the Y row of YIQ, and in the YIQ -> RGB
 * matrix the Y column is (1, 1, 1), so adding raw to B, G and R is the classical magnification of luma with chroma left alone.
 *   - A buffer whose three channels are equal yields three equal output channels, each equal to rm_magnify(..., RM_U8) on that
 *     buffer bit for bit (the gray value of (k, k, k) under the integer cvtColor is k).
 *   - skip_levels_at_top >= pyramid_levels - 1 (nothing is filtered): raw is zero and every byte k becomes u8(k * (1./255)), the
 *     reference's float_to_uint8(uint8_to_float(k)): one level below k on 24 of the 256 levels.  This is the rule of the gray
 *     path, kept for consistency; it is NOT an identity copy.
 * One pass over the frame buffer as rm_magnify (no [T,H,W] or [T,H,W,3] float64 array for 1 <= skip_levels_at_top <= 4).
 * RM_E_BADARG: NULL pointers, T, H or W < 1, pyramid_levels < 1, skip_levels_at_top < 0, fps not > 0, out_dev overlapping the
 * frame buffer (3*T*H*W bytes on both sides);  RM_E_UNSUPPORTED: T > 4096.  Asynchronous on `stream`. */
int rm_magnify_bgr(rm_ctx *ctx, const uint8_t *frames_dev /* [T,H,W,3] BGR */, int T, int H, int W,
                   double fps, double freq_min, double freq_max, double amplification,
                   int pyramid_levels, int skip_levels_at_top,
                   uint8_t *out_dev /* [T,H,W,3] BGR */, void *stream);

/* ---- the fused calibration path: base.py:555-562 (eulerian ... np.average(op, axis=0)) -- */
/* Reads the frame buffer once; never materialises a [T,H,W] intermediate.  heatmap_dev[H*W]
 * receives np.average(masked, axis=0) (sequential-in-t float64 sum / T).  minmax_host (may be
 * NULL) receives {raw.min(), raw.max()}.  Asynchronous unless minmax_host != NULL. */
int rm_calibrate(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W,
                 double fps, double freq_min, double freq_max, double amplification,
                 int pyramid_levels, int skip_levels_at_top, double temporal_threshold,
                 unsigned flags, double *heatmap_dev, double *minmax_host, void *stream);

/* ---- base.py:563-575: normalise, float_to_uint8, threshold, findContours(EXTERNAL,SIMPLE),
 *      max contourArea, boundingRect.  avg_u8_dev / binary_dev (device, H*W, may be NULL) receive
 *      the uint8 heatmap and the thresholded image.  Returns RM_OK + xywh_host[4], or RM_NO_CONTOUR. */
int rm_heatmap_to_roi(rm_ctx *ctx, const double *heatmap_dev, int H, int W, int threshold,
                      int32_t *xywh_host, uint8_t *avg_u8_dev, uint8_t *binary_dev, void *stream);

/* ---- sparse exchange of per-stream heatmaps between GPUs (one stream per GPU, respmon_amd/dist.py::locate_streams).
 *      Not a reference function: it replaces the dense all-reduce(sum) of the [H,W] float64 heatmaps (16.6 MB per GPU
 *      at 1080p) by ONE all-gather of small packets.  The heatmap rm_calibrate leaves behind is a single constant (the
 *      time average of `min`, transforms.py:190-192 + base.py:562) in every 64x16 tile whose frames were all masked,
 *      so a packet holds that constant plus the values of the tiles that differ from it (cap_tiles of them at most).
 *        rm_heat_sparse_packet_doubles(cap)  packet length in doubles
 *        rm_heat_sparse_pack      packet_dev <- heatmap of the LAST rm_calibrate on this context
 *          -- all-gather the packets: packets_dev[world][packet] --
 *        rm_heat_sparse_merge_roi fused_dev[H*W] = sum over ranks, in rank order, of the per-rank heatmaps (avg_T = 0),
 *                                 or of the partial heat sums of a frame-sharded buffer divided by avg_T (rm_shard_heat
 *                                 outputs: the sparse form of the heat-sum all-reduce + rm_shard_finish), then
 *                                 base.py:563-575 on it -> xywh_host.  Returns RM_OK / RM_NO_CONTOUR, or
 *                                 RM_SPARSE_FALLBACK when some rank needed more than cap_tiles tiles (every rank sees
 *                                 the same packets, so every rank falls back to the dense all-reduce together).
 *        rm_heat_sparse_tiles_needed  the largest tile count any rank needed in the LAST rm_heat_sparse_merge_roi on this
 *                                 context (also when it overflowed): identical on every rank, so the ranks can size the
 *                                 next exchange's packets from it without talking to each other. */
size_t rm_heat_sparse_packet_doubles(int cap_tiles);
int rm_heat_sparse_pack(rm_ctx *ctx, const double *heat_dev, int H, int W, int cap_tiles, double *packet_dev, void *stream);
int rm_heat_sparse_merge_roi(rm_ctx *ctx, const double *packets_dev, int world, int H, int W, int cap_tiles, int threshold,
                             int avg_T, double *fused_dev, int32_t *xywh_host, void *stream);
int rm_heat_sparse_tiles_needed(rm_ctx *ctx, int *tiles_host);

/* ---- base.py:547-601 RespiratoryMonitor.locate = rm_calibrate + rm_heatmap_to_roi ------- */
int rm_locate(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W, double fps,
              double freq_min, double freq_max, double amplification, int pyramid_levels,
              int skip_levels_at_top, double temporal_threshold, int threshold, unsigned flags,
              int32_t *xywh_host, void *stream);

/* ---- the same in two calls, for back-to-back calibration buffers (base.py:547-601 called once per buffer: the streams of
 *      BASELINE config 4, the state machine's recalibrations).  rm_locate_submit enqueues the device work of rm_locate on `stream`
 *      and returns a ticket without waiting; rm_locate_result(ticket) waits for it, runs the host contour stage (base.py:568-575)
 *      and fills xywh_host -- same return values and bit-identical ROI as rm_locate.  A context holds up to RM_LOCATE_TICKETS
 *      submissions (RM_E_BUSY beyond), all on ONE stream; results may be fetched in any order.  Submitting buffer k+1 before
 *      fetching buffer k puts the frame-buffer kernel of k+1 where the synchronous call leaves the GPU idle (host wait + contour
 *      stage + launch latency of the next call).  frames_dev must stay valid and unchanged until the ticket's rm_locate_result
 *      (a selection that overflows the value store is taken again synchronously there); between a submit and its result the
 *      context takes no other calls than rm_locate_submit / rm_locate_result / rm_locate on the same stream. */
#define RM_LOCATE_TICKETS 2
int rm_locate_submit(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W, double fps,
                     double freq_min, double freq_max, double amplification, int pyramid_levels,
                     int skip_levels_at_top, double temporal_threshold, int threshold, unsigned flags,
                     void *stream, int *ticket_host);
int rm_locate_result(rm_ctx *ctx, int ticket, int32_t *xywh_host);

/* ---- several subjects in one frame: the K largest contours instead of the largest one.  Not a reference function: base.py:571 keeps
 *      max(contours, key=cv2.contourArea) and drops the rest.  On the image base.py:563-566 builds from the heatmap,
 *        contours = cv2.findContours(thresh, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)
 *        keep those with cv2.contourArea(c) >= min_area
 *        order them by decreasing area; equal areas keep the order of the list findContours returned (the earlier one ranks first:
 *        a stable sort on -area -- at one entry that is what Python's max() keeps)
 *      and the first min(max_rois, count) are returned as cv2.boundingRect (xywh_host[i][4]) and area (area_host[i], may be NULL);
 *      *n_host = how many.  Contours of area 0 (single pixels, one-pixel lines) are contours and are listed when min_area == 0.
 *      With min_area == 0 entry 0 is the ROI of rm_heatmap_to_roi / rm_locate on the same input; rm_locate_multi with max_rois == 1
 *      is rm_locate.  rm_set_contour_clip_frame and RM_FLAG_CONTOUR_CLIP_FRAME act as they do there.
 *      Returns RM_OK (*n_host >= 1) or RM_NO_CONTOUR (*n_host == 0: nothing survives);  RM_E_BADARG: max_rois outside
 *      1..RM_MAX_ROIS, min_area negative or NaN, NULL xywh_host / n_host, H or W < 1.
 *      The calls leave the state of the single-ROI stage alone (its pinned result areas, the contour-labelling rule's counters,
 *      rm_contour_stats): an rm_locate after them behaves as if they had not happened.  One stream wait per call; every external
 *      border is followed on the host. */
#define RM_MAX_ROIS 64
int rm_heatmap_to_rois(rm_ctx *ctx, const double *heatmap_dev, int H, int W, int threshold, int max_rois, double min_area,
                       int32_t *xywh_host /* [max_rois][4] */, double *area_host /* [max_rois], may be NULL */, int *n_host, void *stream);
int rm_locate_multi(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W, double fps,
                    double freq_min, double freq_max, double amplification, int pyramid_levels,
                    int skip_levels_at_top, double temporal_threshold, int threshold, unsigned flags,
                    int max_rois, double min_area, int32_t *xywh_host, double *area_host, int *n_host, void *stream);

/* ---- frame-sharded calibration (one [T,H,W] buffer split by frame index over the GPUs of a node; SURVEY 8e
 *      "Mode A", BASELINE north_star).  Same arithmetic as rm_calibrate (transforms.py:144-198, base.py:562),
 *      cut at the three points where frames meet; the caller runs a collective at each cut
 *      (respmon_amd/dist.py::locate_sharded uses torch.distributed / RCCL):
 *        rm_shard_pyramid   frames[t0:t1] -> lap_local[(t1-t0), NP]   the Gaussian level `skip` of every frame (filter-first form, the
 *                           default where it fits LDS) or the Laplacian levels skip..L-2 (pyramid.py:20-48): see rm_shard_layout_flags
 *          -- all-gather lap_local -> lap_all[T, NP] --
 *        rm_shard_collapse  temporal band-pass + collapse of every frame (cheap, identical on every rank),
 *                           full-resolution evaluation of this rank's frames [t0,t1) only;
 *                           negmin_max_dev[2] (DEVICE) = { -min, max } of raw over those frames
 *          -- all-reduce(MAX) of negmin_max_dev --
 *        rm_shard_heat      heat_sum_dev[H*W] = sum_{t in [t0,t1)} (raw >= top ? min : raw)   (transforms.py:184-192)
 *          -- all-reduce(SUM) of heat_sum_dev: the single [H,W] heatmap collective --
 *        rm_shard_finish    heatmap = heat_sum / T (base.py:562), then base.py:563-575 -> xywh_host (may be NULL).
 *      With one rank (t0 = 0, t1 = T) the result equals rm_calibrate / rm_locate bit for bit; with several
 *      ranks the time sum is associated per shard (<= 1e-15 relative on the heatmap).
 *      rm_shard_layout returns NP (0 when no level is filtered).  Requires skip_levels_at_top >= 1. */
int rm_shard_layout(int H, int W, int pyramid_levels, int skip_levels_at_top, size_t *np_out);
/* ... for the `flags` the other stages will be given (RM_FLAG_FILTER_LAPLACIANS / RM_FLAG_UNFUSED_SMALL change what travels between the
 * stages: the Laplacian levels S .. L-2, NP = their pixel count, instead of the Gaussian level S, NP = h_S * w_S); rm_shard_layout = flags 0 */
int rm_shard_layout_flags(int H, int W, int pyramid_levels, int skip_levels_at_top, unsigned flags, size_t *np_out);
int rm_shard_pyramid(rm_ctx *ctx, const void *frames_local_dev, int dtype, int T_local, int H, int W, int pyramid_levels,
                     int skip_levels_at_top, unsigned flags, double *lap_local_dev, void *stream);
int rm_shard_collapse(rm_ctx *ctx, const double *lap_all_dev, int T, int t0, int t1, int H, int W, double fps,
                      double freq_min, double freq_max, double amplification, int pyramid_levels, int skip_levels_at_top,
                      double temporal_threshold, unsigned flags, double *negmin_max_dev, void *stream);
int rm_shard_heat(rm_ctx *ctx, const double *negmin_max_dev, double temporal_threshold, double *heat_sum_dev, void *stream);
int rm_shard_finish(rm_ctx *ctx, const double *heat_sum_dev, int T, int H, int W, int threshold, double *heatmap_dev,
                    int32_t *xywh_host, void *stream);

/* ---- the calibration on a SLIDING window (base.py:409-513 without the refill).  The default path filters in time before it builds
 *      the Laplacians, so all the tail of rm_locate needs from a frame is the row rm_shard_pyramid writes for it.  An rm_window keeps
 *      the rows of the last T frames in a ring, takes camera frames as they come, and relocates from the ring at any moment: every
 *      frame goes through the frame-buffer kernel once in its life, a relocation costs the tail only, and after a reset of the
 *      monitor the next ROI needs no refill.
 *      Ring: T rows of NP doubles, NP = rm_shard_layout_flags(H, W, levels, skip, flags), allocated once by rm_window_create on the
 *        context's device -- its own allocation, not the context's workspace, so it survives every other call on the context.  A
 *        row holds what rm_shard_pyramid writes for one frame (G_S; the Laplacian levels S .. L-2 under RM_FLAG_FILTER_LAPLACIANS /
 *        RM_FLAG_UNFUSED_SMALL), float64 whatever the frame dtype: successive pushes may differ in dtype.  Requires
 *        skip_levels_at_top >= 1 like the rm_shard calls (RM_E_BADARG); T > 4096 is RM_E_UNSUPPORTED.  NP == 0 (nothing is filtered:
 *        skip >= levels - 1): there is no ring, the heatmap is zero and the ROI stage runs on it, as in rm_shard_collapse.
 *      rm_window_push: n >= 1 frames [n,H,W] of `dtype` (RM_BGR8: [n,H,W,3]), asynchronous on `stream`.  While the ring fills,
 *        frame i of the call goes to row (head + count + i) mod T; once it is full a frame overwrites the oldest row and advances
 *        head.  A call that crosses the ring's end is two launches of the frame-buffer kernel; a call with n > T reduces its last T
 *        frames only.  The ring after a sequence of pushes depends on the frames, not on how they were grouped into calls.
 *      rm_window_reset: count = 0, head = 0; the ring memory is kept.
 *      rm_window_info: frames held, row of the oldest one, NP and the ring's size in bytes (any pointer may be NULL).
 *      rm_window_calibrate / rm_window_locate / rm_window_locate_multi act on the m = min(count, T) frames held, in chronological
 *        order, and give bit for bit what rm_calibrate / rm_locate / rm_locate_multi give on a contiguous [m,H,W] buffer of the same
 *        frames with the window's geometry and flags: same arguments otherwise, same return codes (RM_NO_CONTOUR included).  Before
 *        the ring is full the temporal operator is the one of T = m frames (head is 0 there); count == 0 is RM_E_BADARG.  The
 *        window is never un-rotated or copied: the temporal kernels read frame t from row (t + head) mod T in place, in the product
 *        order of the contiguous call, and write their output in chronological order.  The stages behind them are those of
 *        rm_shard_collapse / rm_shard_heat with one rank; the time average and the heatmap extrema ride the sum kernel as in
 *        rm_calibrate.  A selection that overflows the value store is summed by the dense stand-in on the stream, as in
 *        rm_locate_multi.  rm_window_locate_multi leaves the state of the single-ROI stage alone, as rm_locate_multi does.
 *      The three calls use the context's workspace and the plan rm_shard_collapse leaves for rm_shard_heat: they may not come
 *        between an rm_shard_collapse and its rm_shard_heat, nor between an rm_locate_submit and its rm_locate_result on another
 *        stream (RM_E_BUSY).  Pushes and relocations of one window belong on one stream (or on streams the caller orders): stream
 *        order is what keeps a push off the rows a relocation still reads.  Any other call on the context may come between them.
 *      rm_window_destroy waits for the device work that uses the ring. */
typedef struct rm_window rm_window;
int rm_window_create(rm_ctx *ctx, int T, int H, int W, int pyramid_levels, int skip_levels_at_top, unsigned flags, rm_window **out);
int rm_window_destroy(rm_window *win);
int rm_window_reset(rm_ctx *ctx, rm_window *win);
int rm_window_push(rm_ctx *ctx, rm_window *win, const void *frames_dev, int dtype, int n, void *stream);
int rm_window_info(const rm_window *win, int *count, int *head, size_t *np, size_t *ring_bytes);
int rm_window_calibrate(rm_ctx *ctx, rm_window *win, double fps, double freq_min, double freq_max, double amplification,
                        double temporal_threshold, double *heatmap_dev, void *stream);
int rm_window_locate(rm_ctx *ctx, rm_window *win, double fps, double freq_min, double freq_max, double amplification,
                     double temporal_threshold, int threshold, int32_t *xywh_host, void *stream);
int rm_window_locate_multi(rm_ctx *ctx, rm_window *win, double fps, double freq_min, double freq_max, double amplification,
                           double temporal_threshold, int threshold, int max_rois, double min_area, int32_t *xywh_host,
                           double *area_host, int *n_host, void *stream);

/* ---- the RATE MAP: for every pixel column the dominant frequency inside a band and the share of the band's power in that peak --
 *      the estimator of prototypes/temporal_analysis.py (Blackman-Harris window, spectrum, argmax, parabolic(log .)) on a fine
 *      frequency grid instead of the FFT bins, for every pixel of a pyramid level instead of one ROI signal.
 *      Definition, x[T, NP] float64, 2 <= T <= 4096, 0 < freq_min < freq_max <= fps / 2, 3 <= nfreq = F <= 64:
 *        step = (freq_max - freq_min) / (F - 1), f_j = freq_min + j * step;  w = scipy.signal.blackmanharris(T) (symmetric);
 *        E[2j, t] = w[t] cos(2 pi f_j t / fps), E[2j+1, t] = -w[t] sin(2 pi f_j t / fps), A[r, t] = E[r, t] - mean_u E[r, u]
 *        (sig - sig.mean() folded into the operator), built on the host in long double and rounded once;
 *        y[t, p] = x[t, p] - x[0, p] (a column that never changes gives y == 0 exactly);
 *        c_j = sum_t A[2j, t] y[t, p], s_j = sum_t A[2j+1, t] y[t, p] on v_mfma_f64_16x16x4_f64, P_j = c_j c_j + s_j s_j; the order
 *        of the sums is the kernel's own and fixed for a given (T, NP, F);
 *        total = sum_j P_j added in ascending j, index = the first j at which max_j P_j is reached, power = P_index;
 *        total == 0: index = -1, freq = NaN, power = total = 0;
 *        otherwise freq = f_index + delta * step, where for 0 < index < F - 1 and three positive powers a = log P_(index-1),
 *        b = log P_index, c = log P_(index+1), num = a - c, den = (a - 2 b) + c, delta = den < 0 ? clamp((0.5 num) / den, -0.5, 0.5)
 *        : 0, and delta = 0 elsewhere.
 *      rm_spectral_operator (host only): A_host[2F][T] row major and freqs_host[F]; either may be NULL.
 *      rm_spectral_peak: x_dev[T, NP]; outputs [NP] each, any may be NULL (not all).  Asynchronous on `stream`.
 *      rm_rate_map: x = the Gaussian level `level` (1 <= level <= 5) of every frame of a frame buffer of any buffer dtype (RM_BGR8
 *        included) -- what rm_pyr_down applied `level` times gives, bit for bit, written by the frame-buffer kernel in one pass over
 *        the frames; outputs [h_level * w_level].  The level array lives in the context's workspace.
 *      rm_window_rate_map: the same on the m = min(count, T) frames a window holds, read from the ring in place (the oldest frame is
 *        x[0]); level = the window's skip_levels_at_top.  Bit for bit rm_rate_map on the contiguous buffer of those frames.
 *      RM_E_BADARG: T < 2 (a window with count < 2), nfreq outside 3..64, a band that violates 0 < freq_min < freq_max <= fps / 2
 *        (NaN included), all outputs NULL, NULL input, level < 1.  RM_E_UNSUPPORTED: T > 4096, level >= 6, a window whose rows are not
 *        G_skip (RM_FLAG_FILTER_LAPLACIANS / RM_FLAG_UNFUSED_SMALL, or a geometry whose small pyramid is filtered level by level).
 *        Nothing is written on a refusal.  rm_rate_map and rm_window_rate_map follow the RM_E_BUSY rule of rm_window_locate.
 *      The operator is cached in the context per (T, fps, freq_min, freq_max, nfreq). */
int rm_spectral_operator(int T, double fps, double freq_min, double freq_max, int nfreq, double *A_host, double *freqs_host);
int rm_spectral_peak(rm_ctx *ctx, const double *x_dev, int T, size_t NP, double fps, double freq_min, double freq_max, int nfreq,
                     double *freq_dev, double *power_dev, double *total_dev, int32_t *index_dev, void *stream);
int rm_rate_map(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W, int level, double fps, double freq_min,
                double freq_max, int nfreq, double *freq_dev, double *power_dev, double *total_dev, int32_t *index_dev, void *stream);
int rm_window_rate_map(rm_ctx *ctx, rm_window *win, double fps, double freq_min, double freq_max, int nfreq, double *freq_dev,
                       double *power_dev, double *total_dev, int32_t *index_dev, void *stream);

/* ---- the pulse beside the breath: POS ("plane orthogonal to skin": Wang, den Brinker, Stuijk, de Haan, Algorithmic Principles of
 *      Remote PPG, IEEE TBME 2017) on the three channels of an RM_BGR8 buffer.  Everything above measures luma; the pulse is a
 *      sub-level colour change of skin, and POS projects the temporally normalised colour onto the plane orthogonal to (1, 1, 1), so
 *      an intensity change common to the channels (a lamp, auto-exposure, a moving shadow) vanishes.  Per block of the frame it gives
 *      a pulse map (skin is where the map is periodic), per rectangle a pulse signal for the subjects of rm_locate_multi.  Gray and
 *      16-bit buffers carry no chroma: there is no entry point for them.
 *      rm_bgr_block_sums: frames_dev [N,H,W,3] uint8 (channel 0, 1, 2 = B, G, R), block one of 4, 8, 16, 32, 64, Hb = ceil(H / block),
 *        Wb = ceil(W / block); sums_dev[n][by][bx][c] (uint32) = the sum of channel c over the pixels of frame n that lie in block
 *        (by, bx).  Edge blocks are partial and sum what is there.  The sums are exact integers (at most 64 * 64 * 255), so no order
 *        of summation is part of the interface.  One pass over the 3 N H W bytes in one launch whatever N; any W and any byte
 *        alignment of frames_dev are taken (16-byte loads where W % 16 == 0 and the buffer is 16-byte aligned, byte loads elsewhere).
 *        RM_E_BADARG: NULL pointers, N, H or W < 1, a block not in the list.  RM_E_UNSUPPORTED: N * Hb >= 2^31.
 *      rm_bgr_roi_sums: the same for K rectangles rois_host[k] = x, y, w, h (1 <= K <= RM_MAX_ROIS) of every frame, sums_dev[n][k][c],
 *        in one launch whatever N and K.  Rectangles may overlap, repeat, be 1 x 1 or the whole frame.  rois_host is read before the
 *        call returns.  RM_E_BADARG -- nothing is launched, nothing written -- for a rectangle that does not lie inside the frame, K
 *        out of range, N < 1, NULL pointers.  RM_E_UNSUPPORTED: a rectangle with w * h * 255 >= 2^32, N * K >= 2^31.
 *      rm_pulse_pos: sums_dev [N][NP][3] uint32 (NP columns: blocks or rectangles) -> h_dev [N][NP] float64, 2 <= window = l <= N <=
 *        4096.  Everything is float64, every operation rounds once (no contraction).  For column p and every window start
 *        n = 0 .. N - l:
 *          S_c   = sum_{k<l} s[n+k][p][c]                  integer, exact (uint64); any S_c == 0: the window contributes nothing
 *          x_c,k = ((double)s[n+k][p][c] * (double)l) / (double)S_c      (the product is exact: x is the correctly rounded ratio)
 *          S1_k  = x_G,k - x_B,k           S2_k = (x_G,k + x_B,k) - 2.0 * x_R,k
 *          v1    = sum_k S1_k * S1_k       v2   = sum_k S2_k * S2_k       ascending k, from 0.0
 *          a     = v2 > 0 ? sqrt(v1 / v2) : 0
 *          h_n,k = S1_k + a * S2_k
 *          H[t][p] = sum_n h_n,(t-n)  over n = max(0, t - l + 1) .. min(t, N - l), ascending n, from 0.0
 *        This is the published algorithm; the time mean of each normalised channel over its window is exactly 1, so the means of S1,
 *        S2 and h are 0 in exact arithmetic and the published mean subtractions are left out (the textbook form agrees to ~1e-14
 *        relative).  The per-window S_c and a live in the context's workspace: RM_E_BUSY as rm_rate_map.  RM_E_BADARG: NULL pointers,
 *        N < 2, window outside 2..N.  RM_E_UNSUPPORTED: N > 4096.  NP == 0 is an empty call.
 *      rm_pulse_map: rm_bgr_block_sums, then rm_pulse_pos on [N][Hb * Wb][3], then the estimator of rm_spectral_peak on H[N][Hb * Wb];
 *        outputs [Hb * Wb] each, any may be NULL (not all).  Bit for bit what the three calls give one after the other.  The
 *        intermediates live in the context's workspace: RM_E_BUSY as rm_rate_map.  Band, nfreq and N refusals are rm_spectral_peak's
 *        (T = N); RM_E_BADARG also for a block not in the list and a window outside 2..N.  Nothing is written on a refusal.
 *      All four are asynchronous on `stream`. */
int rm_bgr_block_sums(rm_ctx *ctx, const uint8_t *frames_dev, int N, int H, int W, int block, uint32_t *sums_dev, void *stream);
int rm_bgr_roi_sums(rm_ctx *ctx, const uint8_t *frames_dev, int N, int H, int W, const int32_t *rois_host, int K, uint32_t *sums_dev,
                    void *stream);
int rm_pulse_pos(rm_ctx *ctx, const uint32_t *sums_dev, int N, size_t NP, int window, double *h_dev, void *stream);
int rm_pulse_map(rm_ctx *ctx, const uint8_t *frames_dev, int N, int H, int W, int block, int window, double fps, double freq_min,
                 double freq_max, int nfreq, double *freq_dev, double *power_dev, double *total_dev, int32_t *index_dev, void *stream);

/* ---- a LIVE stream magnified chunk by chunk: the causal band-pass of rm_sosfilt with carried state.  rm_magnify's band-pass is
 *      the reference's FFT operator, which is even in time: its newest frame mixes in motion of the oldest frame of the buffer.  An
 *      rm_stream holds the filter state of every filtered pyramid element instead of a [T,H,W] buffer: each pushed chunk comes back
 *      magnified, at O(1) per frame, and the result does not depend on how the stream was cut into chunks.
 *      Definition.  For the frames f[0], f[1], ... pushed since rm_stream_create or rm_stream_reset, in any chunking,
 *          out[t] = convert(f[t] + raw[t])
 *        with f the frame as the calibration reads it (rm_magnify) and raw what the reference's sequence gives with this filter as its
 *        temporal_filter_function (transforms.py:146): the Laplacian video pyramid (transforms.py:148), sosfilt * amplification
 *        along time on every element of levels skip .. levels-2 (transforms.py:156-170), the collapse (transforms.py:182) -- in THAT
 *        operation order, bit for bit: raw equals the second result of eulerian_magnification_bandpass(...,
 *        temporal_filter_function=temporal_bandpass_filter_sos) of respmon_amd.transforms on the whole sequence.
 *      rm_stream_create: sos_host[nsec][6] / zi_host[nsec][2] or NULL as rm_sosfilt (refusals included).  zi_host given: the first
 *        frame of the stream sets the state to zi * (its pyramid element), the steady start -- a band-pass has no DC gain, so the
 *        stream does not begin with seconds of ringing from the step 0 -> first frame; NULL: from rest.  The state is
 *        2 * nsec * NP doubles, NP = the elements of levels skip .. levels-2 of one frame (rm_shard_layout_flags with
 *        RM_FLAG_FILTER_LAPLACIANS), allocated here on the context's device -- its own allocation, not the context's workspace, so
 *        it survives every other call on the context.  skip_levels_at_top >= pyramid_levels - 1: nothing is filtered, there is no
 *        state and a push is the conversion alone.
 *      rm_stream_push: n >= 1 frames [n,H,W] of `dtype` (any buffer dtype; RM_BGR8: [n,H,W,3]) -> out_dev[n,H,W] of out_dtype RM_U8 /
 *        RM_F32 / RM_F64 with rm_magnify's conversions (clamp included), or RM_BGR8 ([n,H,W,3], RM_BGR8 frames only) with
 *        rm_magnify_bgr's per-channel rule.  Asynchronous on `stream`; n is unbounded (large calls are split internally).  Pushes of
 *        one stream belong on one stream (or on streams the caller orders).  Uses the context's workspace: RM_E_BUSY while an
 *        rm_locate_submit of the context is in flight on another stream.  RM_E_BADARG: n < 1, NULL pointers, out_dev overlapping
 *        the frames, RM_BGR8 output from gray frames, any other out_dtype, a stream created on another device.
 *      rm_stream_reset: the next push starts a new stream.  rm_stream_info: frames pushed since creation / reset, NP, bytes of state
 *        (any pointer may be NULL).  rm_stream_destroy waits for the device work that uses the state. */
typedef struct rm_stream rm_stream;
int rm_stream_create(rm_ctx *ctx, int H, int W, int pyramid_levels, int skip_levels_at_top, const double *sos_host, int nsec,
                     const double *zi_host, double amplification, rm_stream **out);
int rm_stream_destroy(rm_stream *st);
int rm_stream_reset(rm_ctx *ctx, rm_stream *st);
int rm_stream_info(const rm_stream *st, long long *frames_seen, size_t *np, size_t *state_bytes);
int rm_stream_push(rm_ctx *ctx, rm_stream *st, const void *frames_dev, int dtype, int n, void *out_dev, int out_dtype, void *stream);

/* ---- PHASE-BASED motion magnification on the Riesz pyramid (Wadhwa, Rubinstein, Durand, Freeman, "Riesz Pyramids for Fast Phase-Based
 *      Video Magnification", ICCP 2014), a stream object like rm_stream.  The linear method (rm_magnify, rm_stream_*) adds
 *      amplification * band-passed intensity: it holds only while amplification * displacement is small against the spatial
 *      wavelength, amplifies sensor noise by the same factor and leaves [0, 1].  Here the local PHASE of every processed Laplacian
 *      level is band-passed and the level is shifted by amplification * that phase: larger motions, no intensity overshoot, and no
 *      start-up ringing, because the filtered quantity (the accumulated phase difference) starts at zero.
 *      Definition.  THE ORDER OF OPERATIONS IS PART OF THE INTERFACE.  Everything is float64 and every operation rounds once.  Let
 *      L_l[t] be level l of the Laplacian pyramid of frame t, exactly what rm_create_laplacian_video_pyramid produces (levels
 *      0 .. pyramid_levels-1).  Processed levels are skip_levels_at_top <= l <= pyramid_levels - 2; all other levels, the low-pass
 *      residual included, pass through unchanged.  For a processed level, frame t counted since create or reset, pixel (y, x), I = L_l[t]:
 *          R1 = 0.5*(I[y][x+1] - I[y][x-1])      R2 = 0.5*(I[y+1][x] - I[y-1][x])
 *                  neighbour indices by BORDER_REFLECT_101; an axis of length 1 gives 0
 *          first frame after create/reset:  dc = ds = 0
 *          otherwise, with (Ip, R1p, R2p) of the previous frame:
 *              re  = (I*Ip + R1*R1p) + R2*R2p
 *              qx  = Ip*R1 - I*R1p          qy = Ip*R2 - I*R2p
 *              hyp = sqrt(qx*qx + qy*qy)    d  = atan2(hyp, re)
 *              dc  = hyp > 0 ? d*(qx/hyp) : 0       ds = hyp > 0 ? d*(qy/hyp) : 0
 *          Pc += dc;  Ps += ds                         (both start at 0)
 *          A   = sqrt((I*I + R1*R1) + R2*R2)
 *          Fc  = sosfilt step of Pc,  Fs = sosfilt step of Ps
 *                  rm_sosfilt's operation order, from rest, scale 1
 *          den = B(A)    nc = B(A*Fc)    ns = B(A*Fs)
 *                  B is the separable 9-tap binomial (1,8,28,56,70,56,28,8,1)/256:
 *                  along x first, then along y; each pass is the left-to-right sum of k[i]*v[i];
 *                  indices reflected 101 repeatedly (period 2(n-1)); an axis of length 1 reads index 0
 *          bc  = den > 0 ? nc/den : 0       bs = den > 0 ? ns/den : 0
 *                  with RM_PHASE_NO_BLUR: bc = Fc, bs = Fs
 *          m   = sqrt(bc*bc + bs*bs)   am = amplification*m   c = cos(am)   s = sin(am)
 *          ux  = m > 0 ? bc/m : 0      uy = m > 0 ? bs/m : 0
 *          L'_l[t] = I*c - (R1*ux + R2*uy)*s
 *      Then
 *          out[t] = convert( rm_collapse_laplacian_video_pyramid's rule applied to L' )
 *      atan2(hyp, re) stands where the paper writes acos(re/|q|): the same value, well conditioned near zero phase.  Consequences:
 *      the first frame comes back as the collapse of its own pyramid; the result for a sequence does not depend on how it was cut
 *      into pushes (on one device bit for bit); skip_levels_at_top >= pyramid_levels - 1 processes nothing (no state; a push is
 *      pyramid, collapse, conversion).
 *      Known limits: the three-tap Riesz pair (R1, R2) is exact only near spatial frequency pi/2; the phase blur averages across
 *      orientations.  A numpy prototype delivers 0.74-0.85 of the nominal (1 + amplification) on oriented structure, about 0.65 on
 *      isotropic texture with the blur and about 0.85 without (prototype figures).
 *      rm_phase_create: sos_host[nsec][6], 1 <= nsec <= 8, checked as rm_sosfilt checks them (RM_E_BADARG: nsec < 1, a section with
 *        a0 != 1, NULL pointers, H, W or pyramid_levels < 1, skip_levels_at_top < 0, unknown flags; RM_E_UNSUPPORTED: nsec > 8, more than
 *        16 processed levels).  The state is (5 + 4 * nsec) * NP doubles -- Ip, R1p, R2p, Pc, Ps and the two filters' states --, NP the
 *        pixels of the processed levels of one frame, its own allocation on the context's device.
 *      rm_phase_push: n >= 1 gray frames [n,H,W] of dtype RM_U8 / RM_U16 / RM_F16 / RM_F32 / RM_F64 -> out_dev[n,H,W] of out_dtype RM_F64 /
 *        RM_F32 / RM_U8 / RM_U16 with rm_magnify's conversions (the clamp to [0, 1] and the truncation of the integer outputs included).
 *        RM_BGR8 frames: RM_E_UNSUPPORTED (colour is out of scope).  RM_E_BADARG: n < 1, NULL pointers, any other dtype or out_dtype,
 *        out_dev overlapping the frames, an object created on another device; nothing is written on a refusal.  Asynchronous on
 *        `stream`; n is unbounded (a call whose workspace would pass 2 GiB is split internally; the number of launches of one such
 *        piece depends on the pyramid alone, not on its frames).  Pushes of one object belong on one stream.  Uses the context's
 *        workspace: RM_E_BUSY as rm_stream_push.
 *      rm_phase_reset: the next push starts a new sequence.  rm_phase_info: frames pushed since creation / reset, NP, bytes of state
 *        (any pointer may be NULL).  rm_phase_destroy waits for the device work that uses the state. */
typedef struct rm_phase rm_phase;
#define RM_PHASE_NO_BLUR 1u
int rm_phase_create(rm_ctx *ctx, int H, int W, int pyramid_levels, int skip_levels_at_top, const double *sos_host, int nsec,
                    double amplification, unsigned flags, rm_phase **out);
int rm_phase_destroy(rm_phase *ph);
int rm_phase_reset(rm_ctx *ctx, rm_phase *ph);
int rm_phase_info(const rm_phase *ph, long long *frames_seen, size_t *np, size_t *state_bytes);
int rm_phase_push(rm_ctx *ctx, rm_phase *ph, const void *frames_dev, int dtype, int n, void *out_dev, int out_dtype, void *stream);

/* ---- the 'PHASE' motion signal of extract_motion: the amplitude-weighted mean phase velocity of an ROI.  The ROI mean ('average')
 *      sees brightness changes, the Lucas-Kanade tracks ('flow') need corners; a chest under a blanket, on an infrared or depth
 *      camera, moves a fraction of a pixel at constant brightness and offers texture only.  The quaternionic phase difference of a
 *      Riesz-pyramid level between consecutive frames -- the quantity rm_phase_* shifts a level by -- measures exactly that.
 *      Definition.  THE ORDER OF OPERATIONS IS PART OF THE INTERFACE.  Everything is float64 and every operation rounds once.  A
 *      session rm_phase_motion belongs to one rectangle size (w, h) and one pyramid level l, 0 <= l <= 8.  For frame t, counted since
 *      create or reset, and the rectangle (x, y, w, h):
 *          C  = the float64 crop frame[y:y+h, x:x+w], converted from the buffer dtype as the pyramid entry points convert it
 *               (RM_U8: k*(1./255), RM_U16: k*(1./65535), RM_F16 / RM_F32 widened, RM_F64 as it is)
 *          I  = level l of rm_create_laplacian_video_pyramid applied to C as a [1,h,w] clip with pyramid_levels = l + 2:
 *               G_0 = C, G_k+1 = pyrDown(G_k), I = G_l - pyrUp(G_l+1).  The crop is an image of its own: borders reflect at the
 *               crop's edge, as in the flow path.  I is lh x lw, lh = h and lw = w halved l times, rounding up.
 *          R1 = 0.5*(I[y][x+1] - I[y][x-1])      R2 = 0.5*(I[y+1][x] - I[y-1][x])
 *                  neighbour indices by BORDER_REFLECT_101; an axis of length 1 gives 0
 *          A  = sqrt((I*I + R1*R1) + R2*R2)
 *          t == 0:  Sw = Sc = Ss = 0
 *          otherwise, with (Ip, R1p, R2p, Ap) of the previous frame, per pixel:
 *              re  = (I*Ip + R1*R1p) + R2*R2p
 *              qx  = Ip*R1 - I*R1p          qy = Ip*R2 - I*R2p
 *              hyp = sqrt(qx*qx + qy*qy)    d  = atan2(hyp, re)
 *              dc  = hyp > 0 ? d*(qx/hyp) : 0       ds = hyp > 0 ? d*(qy/hyp) : 0
 *              wgt = A*Ap
 *          Sw = sum wgt     Sc = sum wgt*dc     Ss = sum wgt*ds      over the pixels of the level
 *      The order of the three sums is the implementation's; it is a function of (lh, lw) alone, never of N, K, the chunking, the
 *      frame's position in a call or the other subjects (here: 64 x 4 tiles, a DPP wave reduction per row, the four rows in order,
 *      the tiles in order).  Outputs per frame: the three sums.  The caller forms v = (Sc/Sw, Ss/Sw) when Sw > 0: the mean phase
 *      velocity in radians per frame at level l, positive for content moving toward +x / +y.  It is not pixels: a numpy prototype
 *      measures 0.2-0.4 rad per frame and pixel on broadband texture, depending on level and content; the nominal pi/2 / 2^l holds
 *      only at spatial frequency pi/2.
 *      rm_phase_motion_create: the state is 2 * lh * lw doubles -- the previous frame's I (R1p, R2p, Ap are recomputed from it) in two
 *        planes that the internal chunks alternate between --, its own allocation on the context's device (rm_phase_motion_info reports
 *        frames seen, lh, lw, bytes; any pointer may be NULL).  RM_E_BADARG: NULL pointers, w or h < 1, level < 0; RM_E_UNSUPPORTED:
 *        level > 8.
 *      rm_phase_motion_clip: N >= 1 gray frames [N,H,W] resident on the device, the rectangle at (x, y) with the state's size ->
 *        sums_host[N][3] = Sw, Sc, Ss per frame.  N == 1 is the per-frame step; there is no separate begin: the first frame after
 *        create or reset returns zeros and becomes the state.  A clip may be cut anywhere, bit for bit.  It is the K == 1 case of
 *      rm_phase_motion_multi_clip: K subjects, subject k on states_host[k] with rectangle rois_host[k] (x, y, w, h; levels may differ)
 *        -> sums_host[N][K][3]; exactly K rm_phase_motion_clip calls, bit for bit, in outputs and in the states it leaves, so single and
 *        multi calls may be mixed on a state.  Rectangles may overlap or repeat (each with its own state).  The subjects share every
 *        launch: the front (crop with its conversion, the pyrDown chain to G_l+1, the level) runs over (pixel block, frame, subject);
 *        in the reduction a lane owns a level pixel and walks the frames of a chunk with the previous frame in registers.  The
 *        launches of a chunk grow with the level only; a call makes one table upload, one result copy and one stream wait.  The
 *        workspace holds crop-sized planes only, 256 MiB at most summed over the subjects (longer clips are chunked internally),
 *        and belongs to the context: RM_E_BUSY as rm_stream_push.
 *        Refusal is all or nothing -- nothing is enqueued, no state is touched, no output is written; the error text names the first
 *        offending subject.  RM_E_BADARG: K outside 1..RM_MAX_ROIS, N < 1, NULL pointers (a NULL entry of states_host included), a
 *        dtype that is no gray frame dtype, a rectangle outside the frame or of another size than its state, a state of another
 *        device, the same state twice.  RM_E_UNSUPPORTED: RM_BGR8 frames.
 *      rm_phase_motion_reset: the next frame starts a new sequence.  rm_phase_motion_destroy waits for the device work that uses the
 *        state. */
typedef struct rm_phase_motion rm_phase_motion;
int rm_phase_motion_create(rm_ctx *ctx, int w, int h, int level, rm_phase_motion **out);
int rm_phase_motion_destroy(rm_phase_motion *st);
int rm_phase_motion_reset(rm_ctx *ctx, rm_phase_motion *st);
int rm_phase_motion_info(const rm_phase_motion *st, long long *frames_seen, int *lh, int *lw, size_t *state_bytes);
int rm_phase_motion_clip(rm_ctx *ctx, rm_phase_motion *st, const void *frames_dev, int dtype, int N, int H, int W, int x, int y,
                         double *sums_host /* [N][3]: Sw, Sc, Ss */, void *stream);
int rm_phase_motion_multi_clip(rm_ctx *ctx, rm_phase_motion *const *states_host /* [K] */, const void *frames_dev, int dtype, int N, int H, int W,
                               const int32_t *rois_host /* [K][4] x,y,w,h */, int K, double *sums_host /* [N][K][3] */, void *stream);

/* ---- rm_stab_*, rm_warp_shift: a shaky camera taken out of the frames (no counterpart in the reference: every method there and here
 *      assumes a camera that stands still).  Per frame the global shift against a fixed reference frame, and the warp by it.
 *      THE ORDER OF OPERATIONS IS PART OF THE INTERFACE.  Everything is float64, every operation rounds once (-ffp-contract=off).
 *
 *      Session.  rm_stab belongs to one frame size (H, W).  level_coarse >= level_fine >= 0, both <= 8; iterations >= 1; max_shift > 0
 *        in level-0 pixels, at most 64.  The reference frame is the first frame after create or reset, or the frame given to
 *        rm_stab_set_reference; it stays fixed for the session and shifts are relative to it, so a frame's result does not depend on
 *        the other frames of a call, nor on how a sequence is cut into calls.
 *      Gray value f of a frame, as the pyramid entry points convert it: RM_U8 k * (1./255), RM_U16 k * (1./65535), RM_F16 / RM_F32
 *        widened, RM_F64 as it is, RM_BGR8 the integer cvtColor of rm_bgr_to_gray, then * (1./255).
 *      Pyramid.  G_0 = f, G_l+1 = pyrDown(G_l) (rm_pyr_down).  R_l, F_l: the levels of the reference and of the frame, h_l x w_l.
 *      Estimate.  d = (0, 0).  For l = level_coarse down to level_fine:
 *          b = ceil(max_shift / 2^l) + 2; Omega = the pixels at least b from every edge (b <= x <= w_l - 1 - b, the same in y).
 *          Omega empty: the level is skipped, flag bit 0.
 *          Rx = 0.5 * (R[y][x+1] - R[y][x-1]), Ry = 0.5 * (R[y+1][x] - R[y-1][x]);
 *          over Omega: a = sum Rx * Rx, bb = sum Rx * Ry, c = sum Ry * Ry; det = a * c - bb * bb.
 *          det not finite or not > 0: the level is skipped, flag bit 0.
 *          s = d / 2^l (exact).  `iterations` times:
 *              e = bilinear(F_l, x + s.x, y + s.y) - R[y][x] over Omega; gx = sum Rx * e, gy = sum Ry * e;
 *              s.x = s.x - (c * gx - bb * gy) / det; s.y = s.y - (a * gy - bb * gx) / det;
 *              each component clamped to +- max_shift / 2^l.
 *          d = s * 2^l.
 *        Flag bit 1: the clamp changed a component in the last iteration of level_fine -- the frame has probably moved further than
 *        max_shift.  d is the displacement of the frame's content against the reference, positive toward +x / +y.  The iteration count
 *        is fixed; nothing terminates on data.
 *      bilinear(F, fx, fy): x0 = floor(fx), ax = fx - x0, likewise y; i0 = clamp(x0, 0, w-1), i1 = clamp(x0 + 1, 0, w-1), j0, j1
 *        likewise; ((1-ax) * F[j0][i0] + ax * F[j0][i1]) * (1-ay) + ((1-ax) * F[j1][i0] + ax * F[j1][i1]) * ay.
 *      Order of the five sums: the implementation's, a function of (h_l, w_l, b) alone -- never of N, of the chunking or of the
 *        frame's position in a call.  (Here: 64 x 16 tiles of the level, a lane four rows of one column top down, the 64 lanes of a
 *        wave on DPP, the four waves in order; then one wave over the tiles, lane k tiles k, k + 64, ..., and its lanes on DPP.)  No
 *        floating-point atomics.
 *      Warp.  out[y][x] = bilinear(f, x + d.x, y + d.y) on the full-resolution frame, converted to out_dtype by rm_magnify's output
 *        rules: RM_F64 as it is, RM_F32 rounded to nearest, RM_U8 / RM_U16 clamped to [0, 1], then the C truncation of * 255 / * 65535.
 *        RM_BGR8 frames are warped channel by channel, k * (1./255) per channel, and go out as RM_BGR8 only; gray in means gray out.
 *        So a zero shift returns the frame through its conversion rule, and an integer shift is an exact translation with a
 *        replicated border.
 *
 *      rm_stab_create: the state holds R_l for l = level_fine .. level_coarse and (a, bb, c, det) per level, its own allocation on the
 *        context's device (rm_stab_info: frames seen, whether a reference is set, bytes).
 *      rm_stab_set_reference: the frame [H,W] (or [H,W,3] RM_BGR8) becomes the reference; asynchronous.
 *      rm_stab_push: N >= 1 frames resident on the device -> shifts_host[N][2] (d.x, d.y), flags_host[N], and, unless out_dev is NULL
 *        (estimate only), the N warped frames.  With no reference set the first frame becomes the reference and comes back with shift
 *        (0, 0).  The frames' pyramids live in the context's workspace; long clips are chunked internally under a cap of 256 MiB.  The
 *        launches of a chunk grow with the levels and iterations, never with N; the 2 x 2 update is done on the device; a call makes
 *        one result copy and one stream wait.  RM_E_BUSY as for rm_stream_push.
 *      rm_warp_shift: the warp alone with the caller's shifts; no session, asynchronous.  Shifts must be finite and at most 2^20 in
 *        magnitude.
 *      Refusal is all or nothing -- nothing is enqueued, nothing is written.  RM_E_BADARG: NULL pointers, sizes < 1, levels out of order
 *        or negative, iterations < 1, a max_shift that is not finite or not > 0, an out dtype outside the rule, out_dev overlapping the
 *        frames, a state of another device, a shift rm_warp_shift does not take.  RM_E_UNSUPPORTED: a level > 8, max_shift > 64.
 *      Out of scope: rotation, zoom, rolling shutter, a drifting reference, a smoothed camera path, cropping the replicated border. */
typedef struct rm_stab rm_stab;
int rm_stab_create(rm_ctx *ctx, int H, int W, int level_coarse, int level_fine, int iterations, double max_shift, rm_stab **out);
int rm_stab_destroy(rm_stab *st);
int rm_stab_reset(rm_ctx *ctx, rm_stab *st);
int rm_stab_info(const rm_stab *st, long long *frames_seen, int *has_reference, size_t *state_bytes);
int rm_stab_set_reference(rm_ctx *ctx, rm_stab *st, const void *frame_dev, int dtype, void *stream);
int rm_stab_push(rm_ctx *ctx, rm_stab *st, const void *frames_dev, int dtype, int N, void *out_dev /* nullable */, int out_dtype,
                 double *shifts_host /* [N][2] */, int32_t *flags_host /* [N] */, void *stream);
int rm_warp_shift(rm_ctx *ctx, const void *frames_dev, int dtype, int N, int H, int W, const double *shifts_host /* [N][2] */, void *out_dev,
                  int out_dtype, void *stream);

/* ---- rm_stab_sim_*, rm_warp_similarity: a hand-held camera taken out of the frames -- rotation about the optical axis, zoom and
 *      shift, a second model beside rm_stab, which stays as it is.  One degree of roll moves the corners of a 1080p frame by 19 px.
 *      THE ORDER OF OPERATIONS IS PART OF THE INTERFACE.  Everything is float64, every operation rounds once (-ffp-contract=off).
 *
 *      Session.  rm_stab_sim belongs to one frame size (H, W).  level_coarse >= level_fine >= 0, both <= 8; level_linear in
 *        -1 .. level_coarse; iterations >= 1; max_shift in (0, 64] level-0 pixels; max_linear in (0, 0.25].  The reference frame, the
 *        gray value f, the pyramid G_l and bilinear() are rm_stab's.
 *      Transform.  p = (p0, p1, tx, ty), p0 = s cos(theta) - 1, p1 = s sin(theta): a similarity is linear in p.  With
 *        cx = (W - 1) * 0.5, cy = (H - 1) * 0.5, u = x - cx, v = y - cy, m = 1 + p0:
 *            fx = (cx + (m * u - p1 * v)) + tx;  fy = (cy + (p1 * u + m * v)) + ty
 *        is the position in the frame of reference pixel (x, y).  At level l, inv = 1 / 2^l (exact): the same formula with cx * inv,
 *        cy * inv, (tx, ty) * inv and level-pixel coordinates; p0 and p1 do not scale.
 *      Estimate.  p = 0.  For l = level_coarse down to level_fine:
 *        l > level_linear: the level step of rm_stab, unchanged -- its b, its five sums, its 2 x 2 update and its clamp on (tx, ty);
 *          p0 = p1 = 0 still holds there, so the sample positions are rm_stab's bit for bit.
 *        l <= level_linear:
 *          b = ceil((max_shift + max_linear * (cx + cy)) * inv) + 2 (cx, cy of level 0); Omega, Rx, Ry as in rm_stab; Omega empty: the
 *            level is skipped, flag bit 0.
 *          J0 = Rx * u + Ry * v, J1 = Ry * u - Rx * v, J2 = Rx, J3 = Ry (u, v in level pixels against cx * inv, cy * inv).
 *          H_ij = sum over Omega of J_i * J_j for i >= j: ten sums, once per reference and level.
 *          H = L D L^T, row by row, no square root:
 *            D_j = H_jj - sum_{k<j} (L_jk * L_jk) * D_k;  L_ij = (H_ij - sum_{k<j} (L_ik * L_jk) * D_k) / D_j,
 *            each inner sum left to right (D_0 = H_00, L_i0 = H_i0 / D_0).
 *          A D_j not finite or not > 0: the level is skipped, flag bit 0.
 *          s = (tx, ty) * inv.  `iterations` times:
 *            e = bilinear(F_l, fx, fy) - R[y][x] over Omega; g_i = sum (J_i) * e (J_i formed as above, then one product);
 *            L z = g:    z0 = g0; z1 = g1 - L10 * z0; z2 = g2 - (L20 * z0 + L21 * z1); z3 = g3 - ((L30 * z0 + L31 * z1) + L32 * z2);
 *            y_i = z_i / D_i;
 *            L^T x = y:  x3 = y3; x2 = y2 - L32 * x3; x1 = y1 - (L21 * x2 + L31 * x3); x0 = y0 - ((L10 * x1 + L20 * x2) + L30 * x3);
 *            p0 = p0 - x0; p1 = p1 - x1; s.x = s.x - x2; s.y = s.y - x3;
 *            p0, p1 clamped to +- max_linear; s.x, s.y clamped to +- max_shift * inv.
 *          (tx, ty) = s * 2^l.
 *        Flags.  Bit 0: a level was skipped.  Bit 1: the shift clamp changed a component in the last iteration of level_fine, as in
 *        rm_stab.  Bit 2: the linear clamp did.
 *        level_linear exists because the region of a very coarse level is a few pixels, and four parameters are not determined there:
 *        keep it at 1 or 2.  level_linear < level_fine estimates no linear part, and the session then is rm_stab: (0, 0, d).
 *      Order of the sums: the implementation's, a function of (h_l, w_l, b) alone, as in rm_stab -- the same 64 x 16 tiles, DPP fold,
 *        wave order and one-wave fold over the tiles.  No floating-point atomics.
 *      Warp.  out[y][x] = bilinear(f, fx, fy) with the level-0 formula, converted by rm_magnify's output rules; RM_BGR8 channel by
 *        channel, out as RM_BGR8 only; gray in means gray out.  With p0 = p1 = 0 the position is x + tx exactly: rm_warp_shift.
 *
 *      rm_stab_sim_create / _destroy / _reset / _info / _set_reference: as rm_stab's.  The state holds R_l and, per level, (a, bb, c,
 *        det) or the factors L, D and a validity word.
 *      rm_stab_sim_push: N >= 1 frames resident on the device -> params_host[N][4] (p0, p1, tx, ty), flags_host[N] and, unless out_dev
 *        is NULL, the warped frames.  Chunked under the 256 MiB workspace cap; the launches of a chunk do not grow with N; the update is
 *        done on the device; one result copy and one stream wait per call.  RM_E_BUSY as for rm_stream_push.
 *      rm_warp_similarity: the warp alone with the caller's parameters; no session, asynchronous.
 *      Refusal is all or nothing.  RM_E_BADARG: what rm_stab refuses, a level_linear outside -1 .. level_coarse, a max_linear that is not
 *        finite or not > 0, and in rm_warp_similarity parameters that are not finite, |p0| or |p1| > 1, |tx| or |ty| > 2^20.
 *        RM_E_UNSUPPORTED: a level > 8, max_shift > 64, max_linear > 0.25.
 *      Out of scope: shear, perspective, rolling shutter, a camera that pans on purpose, a drifting reference. */
typedef struct rm_stab_sim rm_stab_sim;
int rm_stab_sim_create(rm_ctx *ctx, int H, int W, int level_coarse, int level_fine, int level_linear, int iterations, double max_shift,
                       double max_linear, rm_stab_sim **out);
int rm_stab_sim_destroy(rm_stab_sim *st);
int rm_stab_sim_reset(rm_ctx *ctx, rm_stab_sim *st);
int rm_stab_sim_info(const rm_stab_sim *st, long long *frames_seen, int *has_reference, size_t *state_bytes);
int rm_stab_sim_set_reference(rm_ctx *ctx, rm_stab_sim *st, const void *frame_dev, int dtype, void *stream);
int rm_stab_sim_push(rm_ctx *ctx, rm_stab_sim *st, const void *frames_dev, int dtype, int N, void *out_dev /* nullable */, int out_dtype,
                     double *params_host /* [N][4] */, int32_t *flags_host /* [N] */, void *stream);
int rm_warp_similarity(rm_ctx *ctx, const void *frames_dev, int dtype, int N, int H, int W, const double *params_host /* [N][4] */, void *out_dev,
                       int out_dtype, void *stream);

/* ---- base.py:355-358 + 471: extract_motion('average') = np.average(frame[y:y+h, x:x+w]) -- */
int rm_roi_mean(rm_ctx *ctx, const void *frame_dev, int dtype, int H, int W, int x, int y, int w, int h,
                double *out_host, void *stream);
/* ROI crop + float_to_uint8 (base.py:364, 371, 381): dst_dev[h*w] uint8 */
int rm_roi_to_uint8(rm_ctx *ctx, const void *frame_dev, int dtype, int H, int W, int x, int y, int w, int h,
                    uint8_t *dst_dev, void *stream);

/* ---- base.py:365-366 cv2.goodFeaturesToTrack(img_u8, mask=None, maxCorners, qualityLevel,
 *      minDistance, blockSize).  pts_host: float32 (x,y) pairs, capacity max_corners, or h * w when max_corners <= 0 (no
 *      limit, as in OpenCV); *n_host = count (0 <=> cv2 returns None; always 0 when h < 3 or w < 3). */
int rm_good_features_to_track(rm_ctx *ctx, const uint8_t *img_dev, int h, int w, int max_corners,
                              double quality_level, double min_distance, int block_size,
                              float *pts_host, int *n_host, void *stream);

/* ---- base.py:371-372 cv2.calcOpticalFlowPyrLK(prev, next, pts, None, winSize, maxLevel,
 *      criteria=(EPS|COUNT, max_count, epsilon)).  pts in/out: host float32 (x,y) pairs; status host u8.
 *      RM_E_UNSUPPORTED when win_w * win_h > 1024 or the pyramid, after OpenCV's clamping of maxLevel, needs more than
 *      8 levels (also from rm_flow_step). */
int rm_calc_optical_flow_pyr_lk(rm_ctx *ctx, const uint8_t *prev_dev, const uint8_t *next_dev, int h, int w,
                                const float *pts_in_host, int npts, int win_w, int win_h, int max_level,
                                int max_count, double epsilon, float *pts_out_host, uint8_t *status_host,
                                void *stream);

/* ---- base.py:388: np.mean(good_old - good_new, axis=0) (float32, sequential over points) and
 *      base.py:396-405: np.cov -> np.linalg.eig -> argsort desc -> ROW unpack -> projection[-1].
 *      motion_host: float32 [n,2] (the motion_data deque); *out_host = the value extract_motion returns. */
int rm_mean_flow(rm_ctx *ctx, const float *old_host, const float *new_host, const uint8_t *status_host,
                 int npts, float *mean_xy_host, int *n_good_host, void *stream);
int rm_pca_reduce(rm_ctx *ctx, const float *motion_host, int n, double *out_host, void *stream);

/* ---- base.py:363-388 as ONE call per frame (SURVEY 8b "rm_flow_step"): the ROI crop, its pyramids, the tracked points and
 *      their status never leave the device between two frames.
 *      rm_flow_begin = base.py:364-366: crop + float_to_uint8 of the ROI, cv2.goodFeaturesToTrack on it; the corners are
 *        returned (pts_host, capacity max_corners float32 pairs, or w * h when max_corners <= 0: no limit; *n_host = 0 <=> cv2
 *        returns None) and kept on the device.
 *      rm_flow_step  = base.py:371-388: crop of the new frame, cv2.calcOpticalFlowPyrLK from the previous crop and the kept
 *        points, np.mean(good_old - good_new, axis=0) over status == 1 (float32, point order) -> mean_xy_host[2], *n_good_host;
 *        the new crop and p1[st == 1] become the state the next call starts from (base.py:381-382).  With no points left the
 *        call only advances the previous image (mean 0, n_good 0: the caller returns NaN, base.py:385-386).
 *      rm_flow_points: the points the next step will track (what the reference holds in self.motion_key_points).
 *      Bit-identical to rm_roi_to_uint8 + rm_calc_optical_flow_pyr_lk + rm_mean_flow called in turn. */
/*      The session's state -- previous crop, its LK pyramid and derivatives, the tracked points -- lives in an rm_flow_state the
 *      caller owns (one per RespiratoryMonitor: self.previous_cropped_image / self.motion_key_points of base.py:111-112 are
 *      per object), so several monitors share a GPU and an rm_ctx without seeing each other's tracking.  What a step builds for
 *      the new crop is kept for the next step, which tracks FROM it: one pyramid and one set of derivatives per frame. */
typedef struct rm_flow_state rm_flow_state;
int rm_flow_state_create(rm_ctx *ctx, rm_flow_state **out);
int rm_flow_state_destroy(rm_flow_state *state);
int rm_flow_begin(rm_ctx *ctx, rm_flow_state *state, const void *frame_dev, int dtype, int H, int W, int x, int y, int w, int h, int max_corners,
                  double quality_level, double min_distance, int block_size, float *pts_host, int *n_host, void *stream);
int rm_flow_step(rm_ctx *ctx, rm_flow_state *state, const void *frame_dev, int dtype, int H, int W, int x, int y, int w, int h, int win_w, int win_h,
                 int max_level, int max_count, double epsilon, float *mean_xy_host, int *n_good_host, void *stream);
int rm_flow_points(rm_ctx *ctx, rm_flow_state *state, float *pts_host, int cap, int *n_host, void *stream);

/* ---- extract_motion() over a whole clip that is resident on the device: frames_dev is [N,H,W], contiguous, of a frame dtype.
 *      Each call waits for the stream once; the number of launches does not grow with N.
 *      rm_roi_mean_clip: out_host[i] = rm_roi_mean of frame i, bit for bit.
 *      rm_flow_clip = N successive rm_flow_step calls on a state rm_flow_begin has begun: mean_xy_host[N][2] and n_good_host[N] per
 *        frame, the same error codes for the same arguments (with nothing launched), and the same state afterwards -- the last
 *        crop, the surviving points packed in point order -- so rm_flow_step and rm_flow_clip calls may be mixed and a clip may be
 *        split anywhere.  A state with no points left only advances its previous image (mean 0, n_good 0 for every frame).
 *        Crops, pyramids and derivatives of all frames are built frame-parallel, one wavefront per point then walks the frames in
 *        order; the clip is worked through in chunks whose workspace (about 6.7 bytes per ROI pixel and frame) stays under 256 MiB.
 *        It is the K == 1 entry of rm_flow_multi_clip's driver: the chunk workspace (images, derivatives, positions, carry buffers)
 *        belongs to the context, shared by every state used with it -- a context is not thread-safe, use one per stream / GPU --
 *        while the state keeps the last crop with its pyramid, its points and its counters.
 *      rm_pca_reduce_windows: for every j in [first, n), out_host[j - first] = rm_pca_reduce of rows max(0, j + 1 - window) .. j of
 *        motion_host[n][2] (0.0 below two rows): the values extract_motion returns while the motion_data deque of base.py:473-475
 *        holds at most `window` rows.  The K == 1 case of rm_pca_reduce_windows_multi. */
int rm_roi_mean_clip(rm_ctx *ctx, const void *frames_dev, int dtype, int N, int H, int W, int x, int y, int w, int h,
                     double *out_host, void *stream);
int rm_flow_clip(rm_ctx *ctx, rm_flow_state *state, const void *frames_dev, int dtype, int N, int H, int W, int x, int y, int w, int h,
                 int win_w, int win_h, int max_level, int max_count, double epsilon, float *mean_xy_host, int *n_good_host, void *stream);
int rm_pca_reduce_windows(rm_ctx *ctx, const float *motion_host, int n, int first, int window, double *out_host, void *stream);
/*      rm_roi_mean_multi_clip: K rectangles (rois_host[k] = x, y, w, h; several subjects in one frame) over the clip in one call:
 *        out_host[i * K + k] = rm_roi_mean of frame i and rectangle k, bit for bit, for every frame dtype.  One launch whatever N and
 *        K, one result copy, one stream wait.  Rectangles may overlap, repeat, be 1 x 1 or the whole frame.  RM_E_BADARG -- nothing is
 *        launched, out_host is not written -- for K outside 1..RM_MAX_ROIS, N < 1, or any rectangle that does not lie inside the frame.
 *        K == 1 equals rm_roi_mean_clip. */
int rm_roi_mean_multi_clip(rm_ctx *ctx, const void *frames_dev, int dtype, int N, int H, int W,
                           const int32_t *rois_host /* [K][4] x,y,w,h */, int K, double *out_host /* [N][K] */, void *stream);
/*      rm_flow_multi_clip: K subjects by optical flow in one call = exactly K rm_flow_clip calls, subject k on states_host[k] with
 *        rectangle rois_host[k], bit for bit: mean_xy_host[i][k], n_good_host[i][k] for every frame i, and the state every
 *        rm_flow_state is left in (the last crop with its pyramid, the survivors packed in point order, the point count), so
 *        rm_flow_step, rm_flow_clip, rm_flow_multi_clip and rm_flow_points may be mixed freely on a state and a clip may be split
 *        anywhere.  A subject whose state has no points left only advances its previous image to the clip's last frame; its outputs
 *        are zeros.  The subjects share every launch: the front kernels run over (pixel block, image, subject), the tracker is one
 *        wavefront per (subject, point), the finish one workgroup per (frame, subject); the launches of a chunk grow with the level
 *        count only, the call makes one table upload, one result copy and one stream wait.  The chunk workspace (256 MiB at most,
 *        summed over the subjects) belongs to the context.
 *        Refusal is all or nothing -- nothing is enqueued, no state is touched, no output is written; the error text names the
 *        first offending subject.  RM_E_BADARG: K outside 1..RM_MAX_ROIS, N < 1, NULL pointers (a NULL entry of states_host
 *        included), a dtype that is no frame dtype, win_w or win_h < 3, max_level < 0, N * K beyond int, a rectangle outside the
 *        frame, a state that is not begun, was begun for another ROI size or belongs to another device, the same state twice.
 *        RM_E_UNSUPPORTED where rm_flow_step returns it for a subject that still has points.  K == 1 is rm_flow_clip.
 *      rm_pca_reduce_windows_multi: K motion lists in one call.  motion_host holds the rows of all lists; seg_host[k] = {first row
 *        of list k, its number of rows n_k, first_k}; out_host takes, list after list, the n_k - first_k values
 *        rm_pca_reduce_windows(rows of k, n_k, first_k, window) returns, bit for bit.  One upload, one launch, one download, one
 *        wait.  A list with first_k == n_k contributes nothing.  RM_E_BADARG: K outside 1..RM_MAX_ROIS, window < 1, a negative
 *        entry, first_k > n_k, lists that overlap.  K == 1 is rm_pca_reduce_windows. */
int rm_flow_multi_clip(rm_ctx *ctx, rm_flow_state *const *states_host /* [K] */, const void *frames_dev, int dtype,
                       int N, int H, int W, const int32_t *rois_host /* [K][4] x,y,w,h */, int K,
                       int win_w, int win_h, int max_level, int max_count, double epsilon,
                       float *mean_xy_host /* [N][K][2] */, int32_t *n_good_host /* [N][K] */, void *stream);
int rm_pca_reduce_windows_multi(rm_ctx *ctx, const float *motion_host /* rows of all lists, [.][2] */,
                                const int32_t *seg_host /* [K][3]: first row, n rows, `first` */, int K, int window,
                                double *out_host /* sum_k (n_k - first_k) values, list after list */, void *stream);

/* ---- multi-GPU steps with RCCL behind the C-ABI (the call site they replace is base.py:444, run once per GPU).
 *      One process per GPU, one context per process.  librccl is opened at run time (dlopen), so single-GPU users never need it.
 *        rm_comm_unique_id   rank 0 makes the id (RM_COMM_ID_BYTES bytes = ncclUniqueId) and hands it to the other ranks by any
 *                            out-of-band way (a file, MPI, a torch.distributed broadcast: INTEGRATION.md)
 *        rm_comm_init        ncclCommInitRank on the context's device.  world == 1 with unique_id == NULL: no library involved,
 *                            the collectives are the identity (rm_locate_streams then equals rm_locate)
 *        rm_comm_info        rank / world of the context and ncclCommCount of its communicator (0: none)
 *        rm_shard_frames     Mode A frame shard [t0, t1) of `rank`: contiguous, sizes differ by at most one
 *        rm_locate_streams   Mode B (BASELINE config 4): every rank calibrates ITS OWN [T,H,W] buffer; the float64 heatmaps are
 *                            summed over the ranks in rank order -- one ncclAllGather of sparse packets (a stream's heatmap is one
 *                            constant outside the tiles that survive the pruning), dense ncclAllReduce(sum) when a packet
 *                            overflows (the cap then grows / the exchange stays dense for a while, identically on every rank) --
 *                            and every rank extracts the same ROI.  fused_heat_dev (nullable): the summed heatmap.
 *        rm_locate_sharded   Mode A: ONE [T,H,W] buffer whose frames rm_shard_frames(T, rank, world) are frames_local_dev on this
 *                            rank: pyramid of the local frames -> ncclAllGather -> temporal filter + collapse + pruning for all
 *                            frames -> ncclAllReduce(max) of {-min, max} -> masked time sum of the local frames -> sparse packets
 *                            / dense all-reduce of the partial sums -> heatmap = sum / T -> ROI (every rank the same).
 *      Both enqueue on `stream` and synchronise the host once (twice after a packet overflow).  *exchange_out (nullable):
 *      RM_EXCHANGE_SPARSE / RM_EXCHANGE_DENSE.  Return RM_OK / RM_NO_CONTOUR like rm_locate; RM_E_COMM on an RCCL failure. */
#define RM_COMM_ID_BYTES 128
#define RM_EXCHANGE_SPARSE 1
#define RM_EXCHANGE_DENSE 2
#define RM_SPARSE_CAP_TILES 128   /* tiles (64x16 px) a packet carries at first: 1 MB per rank */
#define RM_SPARSE_MAX_TILES 512   /* ... and at most: 4 MB */
#define RM_DENSE_HOLD 64          /* steps a stream that does not fit stays on the dense all-reduce before the sparse form is tried again */
int rm_comm_unique_id(void *id_out);
int rm_comm_init(rm_ctx *ctx, int rank, int world, const void *unique_id);
int rm_comm_destroy(rm_ctx *ctx);
int rm_comm_info(rm_ctx *ctx, int *rank, int *world, int *rccl_ranks);
int rm_shard_frames(int T, int rank, int world, int *t0, int *t1);
int rm_locate_streams(rm_ctx *ctx, const void *frames_dev, int dtype, int T, int H, int W, double fps, double fmin, double fmax, double amp,
                      int levels, int skip, double temporal_thr, int threshold, unsigned flags, double *fused_heat_dev, int32_t *xywh_host,
                      int *exchange_out, void *stream);
int rm_locate_sharded(rm_ctx *ctx, const void *frames_local_dev, int dtype, int T, int H, int W, double fps, double fmin, double fmax, double amp,
                      int levels, int skip, double temporal_thr, int threshold, unsigned flags, double *heatmap_dev, int32_t *xywh_host,
                      int *exchange_out, void *stream);

/* ---- base.py:230-231: cv2.cvtColor(BGR2GRAY) then uint8_to_float, on device ("next" row f3) */
int rm_bgr_to_gray(rm_ctx *ctx, const uint8_t *bgr_dev, size_t npix, uint8_t *gray_dev, void *stream);

/* ---- base.py:567-568: which cv2.findContours the ROI stage reproduces.  The reference pins no OpenCV version (README.md:12
 *      installs "opencv3" from conda channel menpo; base.py:567 keeps a `thresh_copy` because the version its author ran MUTATED
 *      the input).  OpenCV <= 3.1 zeroes the 1-pixel image frame in place before tracing, so components are clipped to
 *      [1, W-2] x [1, H-2]; OpenCV >= 3.2 traces on a zero-padded copy and frame pixels count.
 *      on = 0 (default): the >= 3.2 rule.  on = 1: the <= 3.1 rule, for every later ROI extraction of this context
 *      (rm_heatmap_to_roi, rm_locate, rm_shard_finish, rm_heat_sparse_merge_roi); rm_locate also takes it per call as
 *      RM_FLAG_CONTOUR_CLIP_FRAME. */
int rm_set_contour_clip_frame(rm_ctx *ctx, int on);
int rm_get_contour_clip_frame(rm_ctx *ctx, int *on);   /* so that a per-call override can put back what the context had */

/* ---- base.py:568-575 on noisy thresholded images.  locate() keeps ONE contour (max contourArea -> boundingRect); when the
 *      image holds thousands of specks (BASELINE configs 2 / 5) the device labels the 8-connected components, reduces their
 *      bounding boxes and the host follows only the borders whose (w-1)*(h-1) bound can reach the best area -- same contour,
 *      same tie rule, no per-speck border following (csrc/rm_ccl.h).
 *      mode = -1 (default): taken when the previous ROI extraction of this geometry met more than 512 components, or when its
 *      host stage walked more than 24 000 border steps (few components with long borders, e.g. a frame of noise blobs; the
 *      host-only stage runs again every 64th call to refresh the count).  Counts only, no clock: a stream takes the same path in
 *      every run;
 *      0: never (every border is followed on the host); 1: always.  The ROI does not depend on the mode.
 *      rm_contour_stats: components / contours met by the last ROI extraction and whether it ran labelled (diagnostics). */
int rm_set_contour_labelling(rm_ctx *ctx, int mode);
int rm_get_contour_labelling(rm_ctx *ctx, int *mode);
int rm_contour_stats(rm_ctx *ctx, int *n_components, int *labelled);

#ifdef __cplusplus
}
#endif
#endif /* RESPMON_HIP_H */
