// respmon_amd/csrc/rm_stream_kernels.h -- the causal band-pass of a live stream: a cascade of second-order sections with carried state
// (rm_sosfilt, rm_stream_push)
//
//   out = scipy.signal.sosfilt(sos, x, axis=0[, zi]) * scale          on x[n, NP] float64
//
// scipy's loop (_sosfilt), per element and sample, sections in order, every operation rounded once (the library is built with
// -ffp-contract=off):
//
//   cur = x[t]
//   for s in 0 .. nsec-1:                sos[s] = (b0, b1, b2, a0 == 1, a1, a2)
//       new     = b0 * cur + z[s][0]
//       z[s][0] = (b1 * cur - a1 * new) + z[s][1]
//       z[s][1] =  b2 * cur - a2 * new
//       cur = new
//   y[t] = cur * scale
//
// Why sections and not rm_lfilter's `ba` polynomials: the order-6 Butterworth band-pass of transforms.py:38-44 has, in `ba` form and
// float64, poles OUTSIDE the unit circle at camera rates (fps 30, 0.1-0.5 Hz: largest pole 1.056, |y| reaches 1.7e19 within 2 000
// samples of noise in [0, 1]); the same design as sections has its largest pole at 0.9963 and |y| stays below 0.3.  DESIGN 4.9.
//
// One lane owns one element and runs the recurrence sequentially in time; the 2 nsec state values live in registers during a call (the
// recurrence is instantiated per section count: no test of it inside the time loop).
// Coefficients are wave-uniform (the kernel argument), loads are coalesced across elements and the next sample is requested one step
// ahead of the recurrence, as in k_lfilter.
//   STATE = 0: the state starts at rest (or at the steady state, INIT) and is dropped at the end: rm_sosfilt.
//   STATE = 1: z[nsec][2][NP] is loaded before the first sample (unless INIT) and stored after the last: a stream cut into calls gives
//              bit for bit the output of one call over the whole of it.
//   INIT  = 1: the first sample sets z[s][k] = zi[s][k] * x[0] (one multiplication), zi the table of scipy.signal.sosfilt_zi: the
//              steady state of a constant input x[0].  A band-pass has no DC gain, so the stream does not begin with seconds of ringing
//              from the step 0 -> first frame.
#pragma once
#include "rm_kernels.h"

namespace rm {

constexpr int SOS_MAX = 8;   // sections (an order-6 band-pass has 6, order 8 has 8)
struct SosCoef { double b0[SOS_MAX], b1[SOS_MAX], b2[SOS_MAX], a1[SOS_MAX], a2[SOS_MAX], zi[SOS_MAX][2]; int n; };

// the recurrence for a compile-time number of sections: straight-line code, the state in 4 NS registers
template <int STATE, int INIT, int NS>
__device__ __forceinline__ void sos_run(const double *x, int n, size_t NP, const SosCoef &c, double scale, double *y, double *z, size_t p)
{
    double z0[NS], z1[NS];
    double nxt = x[p];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if constexpr (INIT) { z0[s] = c.zi[s][0] * nxt; z1[s] = c.zi[s][1] * nxt; }
        else if constexpr (STATE) { z0[s] = z[(size_t)(2 * s) * NP + p]; z1[s] = z[(size_t)(2 * s + 1) * NP + p]; }
        else { z0[s] = 0.0; z1[s] = 0.0; }
    }
    for (int t = 0; t < n; ++t) {
        double cur = nxt;
        if (t + 1 < n) nxt = x[(size_t)(t + 1) * NP + p];   // one sample ahead of the recurrence
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const double nw = c.b0[s] * cur + z0[s];
            z0[s] = (c.b1[s] * cur - c.a1[s] * nw) + z1[s];
            z1[s] = c.b2[s] * cur - c.a2[s] * nw;
            cur = nw;
        }
        y[(size_t)t * NP + p] = cur * scale;
    }
    if constexpr (STATE) {
#pragma unroll
        for (int s = 0; s < NS; ++s) { z[(size_t)(2 * s) * NP + p] = z0[s]; z[(size_t)(2 * s + 1) * NP + p] = z1[s]; }
    }
}

// grid: ceil(NP / 64) single-wave workgroups; c.n in 1 .. SOS_MAX (checked on the host) selects the instance of the recurrence (uniform)
template <int STATE, int INIT>
__global__ __launch_bounds__(64) void k_sosfilt(const double *x, int n, size_t NP, SosCoef c, double scale, double *y, double *z)
{
    const size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= NP) return;
    switch (c.n) {
    case 1: sos_run<STATE, INIT, 1>(x, n, NP, c, scale, y, z, p); break;
    case 2: sos_run<STATE, INIT, 2>(x, n, NP, c, scale, y, z, p); break;
    case 3: sos_run<STATE, INIT, 3>(x, n, NP, c, scale, y, z, p); break;
    case 4: sos_run<STATE, INIT, 4>(x, n, NP, c, scale, y, z, p); break;
    case 5: sos_run<STATE, INIT, 5>(x, n, NP, c, scale, y, z, p); break;
    case 6: sos_run<STATE, INIT, 6>(x, n, NP, c, scale, y, z, p); break;
    case 7: sos_run<STATE, INIT, 7>(x, n, NP, c, scale, y, z, p); break;
    case 8: sos_run<STATE, INIT, 8>(x, n, NP, c, scale, y, z, p); break;
    default: break;
    }
}

}  // namespace rm
