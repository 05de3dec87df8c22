// bench_micro/dc16_bench.hip -- developer microbenchmark of the uint16 register chain (rm_down_u16.h) alone: the two exact unpack forms
// and the float16 chain of the same geometry (the yardstick: same bytes, same loads, two converts per pixel instead of extract +
// convert + multiply), alternating in ONE process on the same resident buffer.
//   uint16_t     the library's form: 16-bit extract, v_cvt_f64_u32, v_mul_f64
//   u16_magic_t  the form that was dropped: k or-ed into the mantissa of 2^52, minus 2^52 (v_add_f64), v_mul_f64
// Prints per shape the median / best kernel ms of each and a checksum of the output (equal checksums = equal bits).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o bench_micro/dc16_bench bench_micro/dc16_bench.hip
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include "../respmon_amd/csrc/rm_kernels.h"
#include "../respmon_amd/csrc/rm_down_u16.h"
using namespace rm;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1); } } while (0)

struct u16_magic_t { uint16_t k; };
static_assert(sizeof(u16_magic_t) == 2, "a 16-bit sample");
namespace rm {
template <> struct VecTraits<u16_magic_t> { static constexpr int V = 8; };
template <> struct RegTraits<u16_magic_t> : RegTraits<uint16_t> {};
template <> __device__ __forceinline__ double unpack_px<u16_magic_t>(const Raw16 &r, int e)
{
    const unsigned int wd = (e >> 1) == 0 ? r.x : (e >> 1) == 1 ? r.y : (e >> 1) == 2 ? r.z : r.w;
    const unsigned int k = (e & 1) ? (wd >> 16) : (wd & 0xffffu);
    const double kd = __longlong_as_double((long long)(0x4330000000000000ull | k)) - 4503599627370496.0;   // (2^52 + k) - 2^52, both exact
    return kd * (1.0 / 65535);
}
}  // namespace rm

// 16-bit samples with every bit in use (the half buffer gets the same smooth image as values in [0, 1])
__global__ void k_fill16(uint16_t *p, size_t n, int W, int H)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H), t = (int)(i / ((size_t)W * H));
        const int lvl = 128 + (int)(60.0f * __sinf(x * 0.01f) * __cosf(y * 0.013f)) + (t & 3);
        p[i] = (uint16_t)((lvl << 8) | (int)((((unsigned)i * 2654435761u) >> 13) & 255u));
    }
}
__global__ void k_fill_half(__half *p, const uint16_t *src, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = (__half)((float)src[i] * (1.0f / 65535));
}
__global__ __launch_bounds__(256) void k_sum(const double *p, size_t n, double *out)   // deterministic: fixed partition, fixed order
{
    __shared__ double part[256];
    double s = 0;
    for (size_t i = threadIdx.x; i < n; i += 256) s += p[i] * (1 + (i % 7));
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0; for (int i = 0; i < 256; ++i) t += part[i]; *out = t; }
}

template <int S> void run(int T, int H, int W, const char *name, int rounds)
{
    std::vector<int> h(S + 1), w(S + 1);
    h[0] = H; w[0] = W;
    for (int k = 1; k <= S; ++k) { h[k] = (h[k - 1] + 1) / 2; w[k] = (w[k - 1] + 1) / 2; }
    const size_t n = (size_t)T * H * W, no = (size_t)T * h[S] * w[S];
    uint16_t *src; __half *srch; double *dst, *d_sum;
    CK(hipMalloc(&src, n * 2)); CK(hipMalloc(&srch, n * 2)); CK(hipMalloc(&dst, no * sizeof(double))); CK(hipMalloc(&d_sum, 8));
    hipLaunchKernelGGL(k_fill16, dim3(4096), dim3(256), 0, 0, src, n, W, H);
    hipLaunchKernelGGL(k_fill_half, dim3(4096), dim3(256), 0, 0, srch, src, n);
    DownGeom g;
    if (!make_down_geom_u8(S, h.data(), w.data(), T, g, false)) { printf("geometry refused\n"); return; }
    const unsigned grid = (unsigned)(((T + 7) / 8) * 8 * g.strips * g.segs);
    const size_t fs = (size_t)H * W;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto launch = [&](int which) {
        if (which == 0) hipLaunchKernelGGL((k_down_chain_u8<S, uint16_t>), dim3(grid), dim3(64), narrow_ring_bytes<uint16_t>(), 0, src, fs, g, dst);
        else if (which == 1) hipLaunchKernelGGL((k_down_chain_u8<S, u16_magic_t>), dim3(grid), dim3(64), narrow_ring_bytes<u16_magic_t>(), 0, (const u16_magic_t *)src, fs, g, dst);
        else hipLaunchKernelGGL((k_down_chain_u8<S, __half>), dim3(grid), dim3(64), narrow_ring_bytes<__half>(), 0, srch, fs, g, dst);
    };
    const char *label[3] = {"u16 cvt_f64_u32", "u16 2^52 magic", "f16 (yardstick)"};
    std::vector<float> ms[3];
    double sums[3];
    for (int which = 0; which < 3; ++which) {   // warm up, and the checksum of each form's output
        CK(hipMemset(dst, 0, no * sizeof(double)));
        for (int i = 0; i < 3; ++i) launch(which);
        hipLaunchKernelGGL(k_sum, dim3(1), dim3(256), 0, 0, dst, no, d_sum);
        CK(hipMemcpy(&sums[which], d_sum, 8, hipMemcpyDeviceToHost));
    }
    for (int r = 0; r < rounds; ++r)
        for (int which = 0; which < 3; ++which) {
            CK(hipEventRecord(e0, 0));
            launch(which);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float t; CK(hipEventElapsedTime(&t, e0, e1));
            ms[which].push_back(t);
        }
    for (int which = 0; which < 3; ++which) {
        std::sort(ms[which].begin(), ms[which].end());
        printf("%-16s S=%d strips=%d segs=%d grid=%u  %-16s : median %.4f ms  best %.4f ms  %.0f GB/s  checksum %.17g\n", name, S, g.strips, g.segs, grid,
               label[which], ms[which][ms[which].size() / 2], ms[which][0], n * 2 / (ms[which][ms[which].size() / 2] * 1e-3) / 1e9, sums[which]);
    }
    printf("%-16s the two uint16 forms %s\n", name, sums[0] == sums[1] ? "agree bit for bit (equal checksums)" : "DIFFER");
    CK(hipFree(src)); CK(hipFree(srch)); CK(hipFree(dst)); CK(hipFree(d_sum));
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 30;
    run<4>(256, 1080, 1920, "256x1080p", rounds);
    run<2>(128, 720, 1280, "128x720p", rounds);
    run<2>(256, 1080, 1920, "256x1080p", rounds);
    return 0;
}
