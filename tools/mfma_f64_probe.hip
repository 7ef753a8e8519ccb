// Issue rate of v_mfma_f64_16x16x4_f64 (chains of dependent accumulations), by number of independent accumulators per wave and
// waves per SIMD, in the manner of mfma_f32_probe.hip; in-kernel clock = d s_memtime / d s_memrealtime (100 MHz).  The last line
// is the best rate seen, "peak_tflops <value>", which tools/cca_bench.py reads.
//   hipcc -O3 --offload-arch=gfx950 tools/mfma_f64_probe.hip -o mfma_f64_probe && ./mfma_f64_probe
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int NACC> __global__ __launch_bounds__(64) void k(double *out, unsigned long long *stamps, int iters)
{
    f64x4 acc[NACC];
    for (int i = 0; i < NACC; ++i) acc[i] = (f64x4){0., 0., 0., 0.};
    double a = threadIdx.x * 0.001 + 1., b = 2. - threadIdx.x * 0.002;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
#pragma unroll
            for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
            asm volatile("" : "+v"(a), "+v"(b));
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    double s = 0.;
    for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 1.2345) out[0] = s;
    if (threadIdx.x == 0 && blockIdx.x < 4096) { stamps[2 * blockIdx.x] = t1 - t0; stamps[2 * blockIdx.x + 1] = r1 - r0; }
}

static double g_best = 0.;

template <int NACC> static void run(int wps, double *out, unsigned long long *st)
{
    const int iters = 2048 / NACC, grid = 256 * 4 * wps;
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    float best = 1e9f;
    for (int t = 0; t < 4; ++t) {
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL((k<NACC>), dim3(grid), dim3(64), 0, 0, out, st, iters);
        (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    unsigned long long h[2];
    (void)hipMemcpy(h, st, sizeof(h), hipMemcpyDeviceToHost);
    const double n_mfma = 16.0 * NACC * iters;                 // per wave
    const double ghz = (double)h[0] / ((double)h[1] / 100e6) / 1e9;
    const double tflops = n_mfma * grid * 2048.0 / (best * 1e-3) / 1e12;
    if (tflops > g_best) g_best = tflops;
    printf("%d accumulators, %d wave(s)/SIMD: %7.1f us; %.1f cycles per MFMA per SIMD; clock %.2f GHz; %.1f TFLOP/s\n", NACC, wps, best * 1e3,
           (double)h[0] / (n_mfma * wps), ghz, tflops);
}

int main()
{
    double *out; unsigned long long *st;
    if (hipMalloc(&out, 64) != hipSuccess || hipMalloc(&st, 4096 * 16) != hipSuccess) { printf("no device\n"); return 1; }
    for (int wps : {1, 2, 4}) { run<1>(wps, out, st); run<2>(wps, out, st); run<4>(wps, out, st); }
    printf("peak_tflops %.2f\n", g_best);
    return 0;
}
