// fp64 VALU issue-rate probe for gfx950 (MI355X): the roof csrc/gs_cluster.hip (the importer's nearest-mean assignment) is priced
// against.  Neither guide states the fp64 vector rate, and that kernel may use neither v_fma_f64 nor MFMA (its contract is a separately
// rounded multiply and add per term), so its roof is what a stream of v_mul_f64 / v_add_f64 pairs issues at: 16 independent accumulators
// per lane, acc[i] = acc[i] + b[i] * c, like the kernel's 4 x 4 register tile.  Also measured: v_mul_f64 alone, v_add_f64 alone and
// v_fma_f64 (what contraction would have bought).  Each at 1, 2, 3 and 4 waves per SIMD on every CU (the kernel runs 3), launch timed by
// hipEvents, every wave timing its own loop with s_memtime against the 100 MHz s_memrealtime for the shader clock the run had.
//
//   hipcc --offload-arch=gfx950 -O2 -o valu_issue_f64 valu_issue_f64.hip && ./valu_issue_f64        (one JSON line per configuration)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

enum Kind { MULADD = 0, MUL = 1, ADD = 2, FMA = 3, NKIND = 4 };
static const char* kName[NKIND] = { "v_mul_f64+v_add_f64", "v_mul_f64", "v_add_f64", "v_fma_f64" };
static const int kInstrPerStep[NKIND] = { 2, 1, 1, 1 };
constexpr int ACC = 16;

template <int KIND> __global__ __launch_bounds__(256) void probe(double* __restrict__ sink, int iters, unsigned long long* __restrict__ cycles,
                                                                 unsigned long long* __restrict__ realtime) {
    double a[ACC], b[ACC];
    const double c = 1.0000000001;
#pragma unroll
    for (int k = 0; k < ACC; ++k) { a[k] = 0.5 + 1e-3 * (double)(threadIdx.x & 63) + (double)k; b[k] = 1e-9 * (double)(k + 1); }
    __syncthreads();
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < ACC; ++k) {
            if (KIND == MULADD) {
                double t;
                asm volatile("v_mul_f64 %0, %1, %2" : "=v"(t) : "v"(b[k]), "v"(c));
                asm volatile("v_add_f64 %0, %0, %1" : "+v"(a[k]) : "v"(t));
            } else if (KIND == MUL) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(a[k]) : "v"(c));
            else if (KIND == ADD) asm volatile("v_add_f64 %0, %0, %1" : "+v"(a[k]) : "v"(b[k]));
            else asm volatile("v_fma_f64 %0, %1, %2, %0" : "+v"(a[k]) : "v"(b[k]), "v"(c));
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < ACC; ++k) acc += a[k];
    if (acc == 123.456) sink[0] = acc;                            // keeps the chains alive
    if ((threadIdx.x & 63) == 0) {
        const size_t w = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        cycles[w] = t1 - t0; realtime[w] = r1 - r0;
    }
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount, iters = 4000;
    const size_t maxWaves = (size_t)cus * 16;
    double* sink; unsigned long long *cyc, *rt;
    CK(hipMalloc(&sink, 64)); CK(hipMalloc(&cyc, maxWaves * 8)); CK(hipMalloc(&rt, maxWaves * 8));
    std::vector<unsigned long long> hc(maxWaves), hr(maxWaves);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int kind = 0; kind < NKIND; ++kind)
        for (int wps : { 1, 2, 3, 4 }) {
            const int grid = cus * wps;                           // 256-thread blocks: one wave per SIMD each, wps of them per CU
            float ms = 0.f;
            for (int rep = 0; rep < 3; ++rep) {                   // the first two warm up (clocks, code)
                CK(hipEventRecord(e0, 0));
                switch (kind) {
                    case MULADD: hipLaunchKernelGGL(probe<MULADD>, dim3(grid), dim3(256), 0, 0, sink, iters, cyc, rt); break;
                    case MUL: hipLaunchKernelGGL(probe<MUL>, dim3(grid), dim3(256), 0, 0, sink, iters, cyc, rt); break;
                    case ADD: hipLaunchKernelGGL(probe<ADD>, dim3(grid), dim3(256), 0, 0, sink, iters, cyc, rt); break;
                    default: hipLaunchKernelGGL(probe<FMA>, dim3(grid), dim3(256), 0, 0, sink, iters, cyc, rt); break;
                }
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                CK(hipEventElapsedTime(&ms, e0, e1));
            }
            const size_t waves = (size_t)grid * 4;
            CK(hipMemcpy(hc.data(), cyc, waves * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(hr.data(), rt, waves * 8, hipMemcpyDeviceToHost));
            std::sort(hc.begin(), hc.begin() + waves); std::sort(hr.begin(), hr.begin() + waves);
            const double instr = (double)iters * ACC * kInstrPerStep[kind];            // wave-instructions per wave
            const double mhz = (double)hc[waves / 2] / ((double)hr[waves / 2] / 100.0);
            const double gwi = (double)waves * instr / (ms * 1e-3) / 1e9;              // chip-wide, by the launch's hipEvent bracket
            printf("{\"kind\": \"%s\", \"waves_per_simd\": %d, \"cus\": %d, \"launch_ms\": %.4f, \"gwi_per_s\": %.2f, \"lane_gops_per_s\": %.1f, \"mhz\": %.0f, "
                   "\"cycles_per_instr_one_wave\": %.3f, \"cycles_per_instr_per_simd\": %.3f}\n", kName[kind], wps, cus, ms, gwi, gwi * 64.0, mhz,
                   (double)hc[waves / 2] / instr, (ms * 1e-3) * mhz * 1e6 * cus * 4.0 / ((double)waves * instr));
        }
    return 0;
}
