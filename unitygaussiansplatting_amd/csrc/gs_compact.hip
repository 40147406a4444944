// gs_compact.hip -- what the export, the bake, the imports and the neighbour grid share, as kernels behind host functions (the build has no relocatable
// device code: a kernel is launched from the file that defines it).  Plain launches; only the Onesweep passes of TwoWordSort wait on other workgroups.
//   enqueue_alive_counts   alive_count + export_scan: per 256-splat chunk the number of alive splats (export_alive, gs_block.h: idx < N, not deleted, not
//                          cut; finiteOnly -- the neighbour grid's list -- also every component of the position finite), popcounts of ballots, and their
//                          exclusive prefix, one workgroup looping over the array 1024 counts at a time; base[chunks] = the total.
//   enqueue_alive_chunk_counts / enqueue_scan   its two halves: the scan alone serves counts made elsewhere (the edit history's compaction).
//   enqueue_alive_list     alive_list + bounds_fold: alive[base[chunk] + rank] = idx in index order and per chunk the min / max of the listed positions
//                          (block_rank / block_bounds, gs_block.h), then the fold of the partials.  minOnly -- the neighbour grid, which wants its origin
//                          and nothing else -- reduces, stores and folds the three minima alone.
//   enqueue_bounds_fold    the fold alone, for partials made elsewhere (the imports' bake_source_bounds, gs_bake.hip).
//   TwoWordSort            the stable sort of a 63-bit key -- the bake's Morton codes, the neighbour grid's cell keys -- as two Onesweep sorts.
#include "gs_common.h"
#include "gs_block.h"

namespace gs {

constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kFoldThreads = 1024;

template <bool FINITE>
__device__ __forceinline__ bool alive_listed(const gsm::AssetView& a, const gsm::EditView& e, uint32_t idx, uint32_t ci, gsm::V3& pos) {
    bool cut;
    const bool alive = export_alive(a, e, idx, ci, pos, cut);
    return FINITE ? alive && gsm::NeighbourFinite(pos) : alive;
}

template <bool FINITE>
__global__ __launch_bounds__(256) void alive_count_kernel(gsm::AssetView a, gsm::EditView e, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_cnt[4];
    gsm::V3 pos;
    (void)block_rank(alive_listed<FINITE>(a, e, blockIdx.x * 256u + threadIdx.x, blockIdx.x, pos), threadIdx.x & 63u, threadIdx.x >> 6, s_cnt);
    __syncthreads();
    if (threadIdx.x == 0u) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// base[i] = counts[0] + .. + counts[i - 1] for i in [0, n]; one workgroup
__global__ __launch_bounds__(kScanThreads) void export_scan_kernel(const uint32_t* __restrict__ counts, uint32_t* __restrict__ base, uint32_t n) {
    __shared__ uint32_t s_wave[kScanThreads / 64];
    __shared__ uint32_t s_carry;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    if (t == 0u) s_carry = 0u;
    __syncthreads();
    for (uint32_t start = 0; start < n; start += kScanThreads) {
        const uint32_t i = start + t;
        const uint32_t v = i < n ? counts[i] : 0u;
        uint32_t incl = v;                                         // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = s_carry;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        if (i < n) base[i] = before + incl - v;
        __syncthreads();                                           // everyone has read s_carry and s_wave
        if (t == kScanThreads - 1u) s_carry = before + incl;
        __syncthreads();
    }
    if (t == 0u) base[n] = s_carry;
}

int32_t enqueue_alive_chunk_counts(hipStream_t st, const gsm::AssetView& a, const gsm::EditView& e, bool finiteOnly, uint32_t chunks, uint32_t* counts) {
    if (finiteOnly) hipLaunchKernelGGL(alive_count_kernel<true>, dim3(chunks), dim3(256), 0, st, a, e, counts);
    else hipLaunchKernelGGL(alive_count_kernel<false>, dim3(chunks), dim3(256), 0, st, a, e, counts);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

int32_t enqueue_scan(hipStream_t st, const uint32_t* counts, uint32_t* base, uint32_t n) {
    hipLaunchKernelGGL(export_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, counts, base, n);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

int32_t enqueue_alive_counts(hipStream_t st, const gsm::AssetView& a, const gsm::EditView& e, bool finiteOnly, uint32_t chunks, uint32_t* counts, uint32_t* base) {
    GS_TRY(enqueue_alive_chunk_counts(st, a, e, finiteOnly, chunks, counts));
    return enqueue_scan(st, counts, base, chunks);
}

// alive[base[chunk] + rank] = idx for the listed splats of source chunk blockIdx.x; partial[chunk][0..2 / 3..5] = min / max of their positions -- as
// stored, or (X.through: the SPZ export's bounds) through the matrix a baked export moves them by.  MAX = false: three partials per chunk, the minima
template <bool FINITE, bool MAX>
__global__ __launch_bounds__(256) void alive_list_kernel(gsm::AssetView a, gsm::EditView e, AliveXform X, const uint32_t* __restrict__ base,
                                                         uint32_t* __restrict__ alive, float* __restrict__ partial) {
    __shared__ uint32_t s_cnt[4];
    __shared__ float s_red[4][6];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    gsm::V3 pos;
    const bool mine = alive_listed<FINITE>(a, e, idx, blockIdx.x, pos);
    const uint32_t slot = block_rank(mine, lane, wave, s_cnt);
    float p[3] = { pos.x, pos.y, pos.z };
    if (X.through != 0u) {                                         // BakeSplatTransform's position
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = gsm::mrow(X.m, c, pos.x, pos.y, pos.z);
    }
    block_bounds<MAX>(mine, p, lane, wave, s_red);
    __syncthreads();
    if (mine) alive[block_first(s_cnt, wave, base[blockIdx.x]) + slot] = idx;
    block_bounds_store<MAX>(s_red, partial + blockIdx.x * (MAX ? 6u : 3u));
}

// bounds[0..2 / 3..5] = min / max over the partials; one workgroup.  MAX = false: three partials per chunk, bounds[0..2]
template <bool MAX>
__global__ __launch_bounds__(kFoldThreads) void bounds_fold_kernel(const float* __restrict__ partial, uint32_t chunks, float* __restrict__ bounds) {
    constexpr uint32_t kCols = MAX ? 6u : 3u;
    __shared__ float s_red[kFoldThreads / 64][kCols];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const float inf = gsm::u2f(0x7f800000u);
    float v[6] = { inf, inf, inf, -inf, -inf, -inf };
    for (uint32_t i = t; i < chunks; i += kFoldThreads) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = fminf(v[c], partial[i * kCols + c]);
            if (MAX) v[3 + c] = fmaxf(v[3 + c], partial[i * kCols + 3 + c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float mn = wave_min(v[c]);
        if (lane == 0u) s_red[wave][c] = mn;
        if (MAX) {
            const float mx = wave_max(v[3 + c]);
            if (lane == 0u) s_red[wave][kCols - 3 + c] = mx;
        }
    }
    __syncthreads();
    if (t < kCols) {
        float r = s_red[0][t];
        for (uint32_t w = 1; w < kFoldThreads / 64; ++w) r = t < 3u ? fminf(r, s_red[w][t]) : fmaxf(r, s_red[w][t]);
        bounds[t] = r;
    }
}

int32_t enqueue_bounds_fold(hipStream_t st, const float* partial, uint32_t count, float* bounds, bool minOnly) {
    if (minOnly) hipLaunchKernelGGL(bounds_fold_kernel<false>, dim3(1), dim3(kFoldThreads), 0, st, partial, count, bounds);
    else hipLaunchKernelGGL(bounds_fold_kernel<true>, dim3(1), dim3(kFoldThreads), 0, st, partial, count, bounds);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

template <bool FINITE>
static void launch_alive_list(hipStream_t st, const gsm::AssetView& a, const gsm::EditView& e, bool minOnly, const AliveXform& X, uint32_t chunks, const uint32_t* base,
                              uint32_t* alive, float* partial) {
    if (minOnly) hipLaunchKernelGGL((alive_list_kernel<FINITE, false>), dim3(chunks), dim3(256), 0, st, a, e, X, base, alive, partial);
    else hipLaunchKernelGGL((alive_list_kernel<FINITE, true>), dim3(chunks), dim3(256), 0, st, a, e, X, base, alive, partial);
}

int32_t enqueue_alive_list(hipStream_t st, const gsm::AssetView& a, const gsm::EditView& e, bool finiteOnly, bool minOnly, const AliveXform& X, uint32_t chunks,
                           const uint32_t* base, uint32_t* alive, float* partial, float* bounds) {
    if (finiteOnly) launch_alive_list<true>(st, a, e, minOnly, X, chunks, base, alive, partial);
    else launch_alive_list<false>(st, a, e, minOnly, X, chunks, base, alive, partial);
    return enqueue_bounds_fold(st, partial, chunks, bounds, minOnly);
}

// ---- TwoWordSort ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sort_gather_kernel(const uint32_t* __restrict__ hi, const uint32_t* __restrict__ rank, uint32_t m, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < m) out[i] = hi[rank[i]];
}

int32_t TwoWordSort::alloc(gs_context* ctx, uint32_t m) {
    for (DevBuf<uint32_t>* b : { &lo, &hi, &hi2, &rank }) GS_HIP(b->alloc(((size_t)m + 16) * 4));
    GS_TRY(sort_state_create(ctx, sort, m, true));
    GS_HIP(control.alloc(2 * sizeof(SortControl)));
    return GS_OK;
}

// one stable sort of `keys` over keyBits bits, `rank` the payload
static int32_t sort_word(gs_context* ctx, TwoWordSort& s, SortControl* control, uint32_t* keys, uint32_t m, uint32_t keyBits) {
    const int passes = (int)((keyBits + 7u) / 8u);
    const uint32_t lastMask = (1u << (keyBits - 8u * (uint32_t)(passes - 1))) - 1u;
    GS_TRY(enqueue_histogram(ctx, ctx->stream, keys, m, nullptr, passes, lastMask, control, s.sort));
    return enqueue_sort_passes(ctx, ctx->stream, s.sort, control, keys, s.rank, m, nullptr, passes, lastMask);
}

int32_t TwoWordSort::enqueue(gs_context* ctx, uint32_t m) {
    GS_TRY(sort_word(ctx, *this, control.get(), lo, m, 32u));
    hipLaunchKernelGGL(sort_gather_kernel, dim3((m + 255u) / 256u), dim3(256), 0, ctx->stream, (const uint32_t*)hi.get(), (const uint32_t*)rank.get(), m, hi2.get());
    GS_HIP(hipGetLastError());
    return sort_word(ctx, *this, control.get() + 1, hi2, m, 31u);
}

hipError_t TwoWordSort::enqueue_error_readback(hipStream_t st, uint32_t err[2]) const {
    for (int k = 0; k < 2; ++k) {
        const hipError_t e = hipMemcpyAsync(&err[k], &control.get()[k].error, 4, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace gs
