// Test-only: the TEXT of copy_splats_kernel (csrc/gs_copy.hip, from its constants to the end of the kernel: tests/test_copy_model.py cuts it out and
// passes the file as -DCOPY_KERNEL_TEXT) compiled for the HOST and run thread for thread -- one std::thread per GPU thread of a workgroup, a
// std::barrier for __syncthreads and for the ballot, a static array for the LDS -- so that the kernel's indexing (the early exits, the per-wave
// staging and its dwordx4 loop, the 45th float, the texel address, the atomicOr into shared words) is held to tests/copy_model.py on a box without a
// GPU.  It says nothing about what the GPU's compiler makes of the text.  Never part of the shipped library.
#include <barrier>
#include <thread>
#include <vector>
#include <atomic>
#include "../unitygaussiansplatting_amd/csrc/gs_params.h"
struct dim3s { uint32_t x, y, z; };
static thread_local dim3s threadIdx, blockIdx;
static std::barrier<>* g_bar;
static unsigned long long g_pred[4];
struct float4 { float x, y, z, w; };
struct uint4 { uint32_t x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return { a, b, c, d }; }
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return { a, b, c, d }; }
static void __syncthreads() { g_bar->arrive_and_wait(); }
static unsigned long long __ballot(bool p) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) g_pred[wave] = 0;
    g_bar->arrive_and_wait();
    if (p) __atomic_fetch_or(&g_pred[wave], 1ull << lane, __ATOMIC_SEQ_CST);
    g_bar->arrive_and_wait();
    const unsigned long long v = g_pred[wave];
    g_bar->arrive_and_wait();
    return v;
}
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
#define __global__
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
namespace gs {
#include COPY_KERNEL_TEXT
}
extern "C" void emu_copy(const gs_asset_desc* d, const uint32_t* srcDeleted, const gs_copy_params* p, uint8_t* pos, uint8_t* other, uint8_t* color, uint8_t* sh,
                         uint32_t* deleted, uint32_t dstN, uint32_t srcStart, uint32_t dstStart, uint32_t count) {
    const gsm::AssetView a = gs::asset_view_of(*d);
    const gsm::CopyXform X = gs::copy_xform_of(p);
    gs::CopyDst dst = { pos, other, color, sh, deleted, dstN };
    // the host's clamp (copy_clamp in gs_copy.hip, restated: it sits behind the cut)
    if (srcStart >= a.n || dstStart >= dstN) return;
    if (count > a.n - srcStart) count = a.n - srcStart;
    if (count > dstN - dstStart) count = dstN - dstStart;
    if (!count) return;
    const uint32_t blocks = (count + 255u) / 256u;
    for (uint32_t b = 0; b < blocks; ++b) {
        std::barrier<> bar(256);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < 256; ++t)
            th.emplace_back([&, t] { threadIdx = { t, 0, 0 }; blockIdx = { b, 0, 0 }; gs::copy_splats_kernel(a, srcDeleted, X, dst, srcStart, dstStart, count); });
        for (auto& x : th) x.join();
    }
}
