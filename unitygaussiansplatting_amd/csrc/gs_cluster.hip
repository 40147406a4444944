// gs_cluster.hip -- the importer's one hot loop on the GPU: nearest-mean assignment of the 45-D SH vectors to the K palette
// entries of the Cluster* SH formats (GaussianSplatAssetCreator.cs:476-518; host form: assign_clusters in gs_import.cpp).
//
// The contract is the host loop, operation for operation, so that the two give the same index for every point and an import
// is the same bytes wherever the assignment ran.  For point i and mean j:
//     dot = 0.0;  for k = 0..44 in that order: dot = dot + (double)x[i][k] * (double)m[j][k]      (product rounded, then the sum)
//     d_j = c2[j] - 2.0 * dot          c2[j] = the same sequential sum of m*m, computed once on the host
// with plain fp64 VALU multiplies and adds: no FMA (the file is compiled without contraction and says so itself below), no
// reassociation, no MFMA (whose internal summation order is not ours to fix).  IEEE double multiply and add round on gfx950 as
// on x86, so the distances are the host's bits and ties fall the same way.
// The index is what the host's scan (best = 0; take j when d_j < bd) gives: 0 if d_0 is NaN, else the smallest j attaining the
// minimum over the non-NaN d_j.  Partial results -- a thread's running best over the mean tiles, then the 16 threads that share
// a point -- are merged with "d < bd, or d == bd and j < bj", under which a NaN never wins; the lane that owns mean 0 remembers
// whether d_0 was NaN.  NaN, +-inf, -0.0 and denormals therefore need no route of their own.
//
// Shape: a workgroup of 256 threads holds 64 points (fp64, converted once, in LDS for the whole kernel) and walks the means in
// tiles of 64 (fp64 in LDS, converted once per tile; the next tile's floats are fetched into registers under the arithmetic).
// A thread owns 4 points x 4 means = 16 accumulators: per k it reads 2 + 2 double2 from LDS for 16 multiplies + 16 adds,
// 2 B of LDS per lane-operation, half of what the CU's LDS delivers beside four SIMDs of fp64 VALU.
//
// Below it, the rest of cluster_shs (gs_import.cpp) on device pointers -- enqueue_cluster_shs: the seeds, the training subset, c2, and the mean update, whose
// summation order is part of the bytes -- so that the bake (gs_bake.hip) and gs_import_cluster_shs with a context keep the whole palette on the GPU.
#include <stdlib.h>

#include <algorithm>

#include "gs_common.h"

#pragma clang fp contract(off)

namespace gs {

namespace {

constexpr int kDim = 45;                  // floats per SH vector
constexpr int kTile = 64;                 // points per workgroup = means per tile
constexpr int kClusterThreads = 256;
constexpr int kRow = 66;                  // doubles per LDS row [k][0..63]: 64 + 2 of padding -- rows stay 16-byte aligned for the double2 reads and
                                          // the staging stores of one wave (consecutive k, 528 B apart) spread over the banks
constexpr int kTileElems = kTile * kDim;  // 2,880 floats of a full tile, contiguous in memory
constexpr int kPre = (kTileElems + kClusterThreads - 1) / kClusterThreads;   // 12 staged floats per thread
constexpr uint32_t kNone = 0xFFFFFFFFu;   // "no candidate yet": loses every index tie

// the one merge rule: in-thread over ascending j, across mean tiles and across threads.  A NaN d compares false twice.
__device__ __forceinline__ void take_better(double d, uint32_t j, double& bd, uint32_t& bj) {
    if (d < bd || (d == bd && j < bj)) { bd = d; bj = j; }
}

__global__ __launch_bounds__(kClusterThreads) void assign_clusters_kernel(const float* __restrict__ x, uint32_t n, const float* __restrict__ means,
                                                                          const double* __restrict__ c2, uint32_t K, uint32_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double xs[kDim * kRow];
    __shared__ __attribute__((aligned(16))) double ms[kDim * kRow];
    __shared__ double c2s[kTile];
    const uint32_t t = threadIdx.x;
    const uint32_t mg = t & 15, pg = t >> 4;       // this thread: means 2mg, 2mg+1, 32+2mg, 33+2mg of a tile x points 2pg, 2pg+1, 32+2pg, 33+2pg
    const uint32_t p0 = blockIdx.x * (uint32_t)kTile;
    const uint32_t np = min((uint32_t)kTile, n - p0);
    const float* xb = x + (size_t)p0 * kDim;
    for (uint32_t e = t; e < (uint32_t)kTileElems; e += kClusterThreads) {     // points: fp64 once, [k][point]; rows past n are zero and never stored
        const uint32_t p = e / kDim, k = e - p * kDim;
        xs[k * kRow + p] = p < np ? (double)xb[e] : 0.0;
    }

    float pre[kPre];
    auto fetch = [&](uint32_t j0) {                                            // the floats of tile j0.. (contiguous), zero past mean K-1
        const size_t base = (size_t)j0 * kDim, end = (size_t)K * kDim;
#pragma unroll
        for (int i = 0; i < kPre; ++i) {
            const uint32_t e = t + (uint32_t)i * kClusterThreads;
            pre[i] = (e < (uint32_t)kTileElems && base + e < end) ? means[base + e] : 0.0f;
        }
    };

    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double bd[4] = { inf, inf, inf, inf };
    uint32_t bj[4] = { kNone, kNone, kNone, kNone };
    uint32_t d0nan = 0;                            // bit a: d_0 of point a was NaN (only the thread that owns mean 0 ever sets it: mg == 0, the storing lane)
    const uint32_t jl[4] = { 2 * mg, 2 * mg + 1, 32 + 2 * mg, 33 + 2 * mg };  // ascending

    fetch(0);
    for (uint32_t j0 = 0; j0 < K; j0 += kTile) {
        __syncthreads();                           // the previous tile has been read by every wave
#pragma unroll
        for (int i = 0; i < kPre; ++i) {
            const uint32_t e = t + (uint32_t)i * kClusterThreads;
            if (e < (uint32_t)kTileElems) { const uint32_t j = e / kDim, k = e - j * kDim; ms[k * kRow + j] = (double)pre[i]; }
        }
        if (t < (uint32_t)kTile) c2s[t] = j0 + t < K ? c2[j0 + t] : 0.0;
        __syncthreads();
        if (j0 + kTile < K) fetch(j0 + kTile);     // lands under the arithmetic below

        double acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
#pragma unroll 5
        for (int k = 0; k < kDim; ++k) {
            const double2 x0 = *(const double2*)&xs[k * kRow + 2 * pg], x1 = *(const double2*)&xs[k * kRow + 32 + 2 * pg];
            const double2 m0 = *(const double2*)&ms[k * kRow + 2 * mg], m1 = *(const double2*)&ms[k * kRow + 32 + 2 * mg];
            const double xv[4] = { x0.x, x0.y, x1.x, x1.y }, mv[4] = { m0.x, m0.y, m1.x, m1.y };
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = acc[a][b] + xv[a] * mv[b];       // v_mul_f64, v_add_f64: two roundings
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t j = j0 + jl[b];
            if (j < K) {                           // the K tail: padding means take no part
                const double c = c2s[jl[b]];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const double d = c - 2.0 * acc[a][b];
                    if (j == 0 && d != d) d0nan |= 1u << a;
                    take_better(d, j, bd[a], bj[a]);
                }
            }
        }
    }

    // the 16 threads that share a point are 16 consecutive lanes of one wave
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double od = __shfl_xor(bd[a], s);
            const uint32_t oj = __shfl_xor(bj[a], s);
            take_better(od, oj, bd[a], bj[a]);
        }
    if (mg == 0) {
        const uint32_t pl[4] = { 2 * pg, 2 * pg + 1, 32 + 2 * pg, 33 + 2 * pg };
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (pl[a] < np) out[p0 + pl[a]] = ((d0nan >> a) & 1u) || bj[a] == kNone ? 0u : bj[a];    // d_0 NaN, or every d NaN: the host's scan stays at 0
    }
}

constexpr uint64_t kPointBudgetBytes = 256ull << 20;        // device memory for one batch of points + their indices
constexpr uint64_t kMaxBatch = 1ull << 24;                  // 32-bit point offsets inside the kernel

// points per launch: b (host points: what the fixed device buffer holds; resident points: the kernel's limit), or GSPLAT_IMPORT_BATCH
uint64_t batch_points(uint64_t n, uint64_t b = kPointBudgetBytes / (kDim * 4 + 4)) {
    if (const char* e = getenv("GSPLAT_IMPORT_BATCH")) {     // read per call
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (end != e && v > 0) b = v;
    }
    return std::max<uint64_t>(1, std::min(std::min(b, kMaxBatch), n));
}

// ---- the Lloyd loop's other kernels: everything that keeps the palette on the GPU between the assignment passes ---------------------------
constexpr uint32_t kSubset = 200000;      // cluster_shs' training subset
constexpr int kRowsInFlight = 16;         // rows a wave of the mean update has loads out for at once

// dst[i] = x[(i * n) / count] for i < count: the stride-sampled seeds (count = K) and training subset (count = 200,000); one thread per float
__global__ __launch_bounds__(256) void cluster_gather_rows_kernel(const float* __restrict__ x, uint64_t n, uint32_t count, float* __restrict__ dst) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= count * (uint32_t)kDim) return;
    const uint32_t i = e / kDim, k = e - i * kDim;
    dst[e] = x[(((uint64_t)i * n) / count) * kDim + k];
}

// c2[j] = the host's sequential sum of m * m (product rounded, then the sum); one thread per mean
__global__ __launch_bounds__(256) void cluster_c2_kernel(const float* __restrict__ means, uint32_t K, double* __restrict__ c2) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= K) return;
    double sq = 0.0;
    for (int k = 0; k < kDim; ++k) { const double m = (double)means[(size_t)j * kDim + k]; sq = sq + m * m; }
    c2[j] = sq;
}

__global__ __launch_bounds__(256) void cluster_iota_kernel(uint32_t* __restrict__ pts, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) pts[i] = i;
}

// keys: the cluster of every point after the stable sort, ascending.  range[j] / range[K + j] = where cluster j's run starts / ends; both stay 0
// (zeroed before the launch) for a cluster that has no point.  It also carries the sort's error word into `sticky`, which outlives the next sort's
// zeroing of the control block: a look-back spin that expired in any pass fails the call (GS_ERR_SORT_TIMEOUT).  After such a sort keys and pts are
// not a permutation; the two range checks here and in the mean update only keep that call's reads inside the buffers until it has failed.
__global__ __launch_bounds__(256) void cluster_ranges_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t K, uint32_t* __restrict__ range,
                                                             const uint32_t* __restrict__ sortError, uint32_t* __restrict__ sticky) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t == 0u && *sortError != 0u) *sticky = 1u;
    if (t >= n) return;
    const uint32_t j = keys[t];
    if (j >= K) return;
    if (t == 0u || keys[t - 1u] != j) range[j] = t;
    if (t == n - 1u || keys[t + 1u] != j) range[K + j] = t + 1u;
}

// The mean update: one wave per cluster, lane k < 45 owns coefficient k, so a point is one contiguous 180-byte read and the sum of a coefficient is
// one lane's sequential chain sum = sum + (double)sub[p][k] over the cluster's points in ascending point index (pts is (cluster, point) sorted) --
// never split across waves, never reassociated.  The chain is sequential, the loads are not: the wave reads 64 point numbers at once (the slots past
// the run's end repeat its last point), issues the kRowsInFlight row loads of a group UNCONDITIONALLY -- every address is a valid row, so nothing
// stands between two loads -- and only then adds, the adds alone being predicated on the run's length.  The cluster, its run and the point numbers
// are wave-uniform and say so (readfirstlane / readlane): the run's ends and the row bases live in SGPRs.  A cluster without points keeps its mean.
__global__ __launch_bounds__(256) void cluster_mean_update_kernel(const float* __restrict__ sub, const uint32_t* __restrict__ pts, const uint32_t* __restrict__ range,
                                                                  uint32_t n, uint32_t K, float* __restrict__ means) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t j = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= K) return;
    const uint32_t s = range[j], e = range[K + j];
    if (e <= s) return;
    const uint32_t k = lane < (uint32_t)kDim ? lane : (uint32_t)kDim - 1u;     // lanes 45..63 repeat lane 44's reads and store nothing
    double sum = 0.0;
    for (uint32_t t0 = s; t0 < e; t0 += 64u) {
        const uint32_t m = min(64u, e - t0);
        uint32_t id = pts[t0 + min(lane, m - 1u)];
        if (id >= n) id = 0u;                                                  // (only after a failed sort: see cluster_ranges_kernel)
        for (uint32_t g = 0; g < m; g += (uint32_t)kRowsInFlight) {
            float v[kRowsInFlight];
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) {
                const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)(g + (uint32_t)u));
                v[u] = sub[(size_t)p * kDim + k];
            }
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u)
                if (g + (uint32_t)u < m) sum = sum + (double)v[u];
        }
    }
    if (lane < (uint32_t)kDim) means[(size_t)j * kDim + lane] = (float)(sum / (double)(e - s));
}

int32_t enqueue_assign(hipStream_t st, const float* x, uint64_t n, const float* means, const double* c2, uint32_t K, uint32_t* out) {
    const uint64_t batch = batch_points(n, kMaxBatch);        // device-resident points: no buffer to fit
    for (uint64_t i0 = 0; i0 < n; i0 += batch) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(batch, n - i0);
        assign_clusters_kernel<<<dim3((nb + kTile - 1) / kTile), dim3(kClusterThreads), 0, st>>>(x + (size_t)i0 * kDim, nb, means, c2, K, out + i0);
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}

inline uint32_t blocks_of(uint64_t threads) { return (uint32_t)((threads + 255u) / 256u); }

} // namespace

int32_t cluster_run_alloc(gs_context* ctx, ClusterRun& run, uint64_t n, uint32_t K) {
    const uint32_t ns = (uint32_t)std::min<uint64_t>(n, kSubset);
    if (n > kSubset) GS_HIP(run.sub.alloc((size_t)kSubset * kDim * 4));
    GS_HIP(run.c2.alloc((size_t)K * 8));
    GS_HIP(run.keys.alloc(((size_t)ns + 16) * 4));
    GS_HIP(run.pts.alloc(((size_t)ns + 16) * 4));
    GS_HIP(run.range.alloc((size_t)K * 2 * 4));
    GS_TRY(sort_state_create(ctx, run.sort, ns, true));
    GS_HIP(run.control.alloc(sizeof(SortControl)));
    GS_HIP(run.error.alloc(4));
    return GS_OK;
}

// cluster_shs of gs_import.cpp on device pointers, enqueued on the context's stream with no host round trip: seeds, training subset, four Lloyd
// passes on the subset (assignment; stable Onesweep sort of (cluster, point) by the cluster's ceil(log2 K) bits; the runs' ends; the mean update),
// one assignment pass over all n.  x: n x 45, means: K x 45, index: n.  ev: null, or ten events -- the start, after each pass's assignment and
// mean update, after the final assignment.  The caller waits for the stream and reads run.error (a bounded look-back spin expired in one of the sorts).
int32_t enqueue_cluster_shs(gs_context* ctx, ClusterRun& run, const float* x, uint64_t n, uint32_t K, float* means, uint32_t* index, const hipEvent_t* ev) {
    hipStream_t st = ctx->stream;
    const uint32_t ns = (uint32_t)std::min<uint64_t>(n, kSubset);
    const float* sub = x;
    GS_HIP(hipMemsetAsync(run.error, 0, 4, st));
    hipLaunchKernelGGL(cluster_gather_rows_kernel, dim3(blocks_of((uint64_t)K * kDim)), dim3(256), 0, st, x, n, K, means);
    if (n > kSubset) {
        hipLaunchKernelGGL(cluster_gather_rows_kernel, dim3(blocks_of((uint64_t)kSubset * kDim)), dim3(256), 0, st, x, n, kSubset, run.sub.get());
        sub = run.sub;
    }
    GS_HIP(hipGetLastError());
    uint32_t keyBits = 1;
    while (keyBits < 16u && (1u << keyBits) < K) ++keyBits;
    const int passes = (int)((keyBits + 7u) / 8u);
    const uint32_t lastMask = (1u << (keyBits - 8u * (uint32_t)(passes - 1))) - 1u;
    if (ev) GS_HIP(hipEventRecord(ev[0], st));
    for (int it = 0; it < 4; ++it) {
        hipLaunchKernelGGL(cluster_c2_kernel, dim3(blocks_of(K)), dim3(256), 0, st, (const float*)means, K, run.c2.get());
        GS_TRY(enqueue_assign(st, sub, ns, means, run.c2, K, run.keys));
        if (ev) GS_HIP(hipEventRecord(ev[1 + 2 * it], st));
        hipLaunchKernelGGL(cluster_iota_kernel, dim3(blocks_of(ns)), dim3(256), 0, st, run.pts.get(), ns);
        GS_HIP(hipGetLastError());
        GS_TRY(enqueue_histogram(ctx, st, run.keys, ns, nullptr, passes, lastMask, run.control, run.sort));
        GS_TRY(enqueue_sort_passes(ctx, st, run.sort, run.control, run.keys, run.pts, ns, nullptr, passes, lastMask));
        GS_HIP(hipMemsetAsync(run.range, 0, (size_t)K * 2 * 4, st));
        hipLaunchKernelGGL(cluster_ranges_kernel, dim3(blocks_of(ns)), dim3(256), 0, st, (const uint32_t*)run.keys.get(), ns, K, run.range.get(),
                           (const uint32_t*)&run.control.get()->error, run.error.get());
        hipLaunchKernelGGL(cluster_mean_update_kernel, dim3((K + 3u) / 4u), dim3(256), 0, st, sub, (const uint32_t*)run.pts.get(), (const uint32_t*)run.range.get(), ns, K, means);
        GS_HIP(hipGetLastError());
        if (ev) GS_HIP(hipEventRecord(ev[2 + 2 * it], st));
    }
    hipLaunchKernelGGL(cluster_c2_kernel, dim3(blocks_of(K)), dim3(256), 0, st, (const float*)means, K, run.c2.get());
    GS_TRY(enqueue_assign(st, x, n, means, run.c2, K, index));
    if (ev) GS_HIP(hipEventRecord(ev[9], st));
    return GS_OK;
}

// gs_import_cluster_shs with a context: the points are uploaded once, the loop above runs, means and indices come back at the end
int32_t cluster_shs_gpu(gs_context* ctx, const float* x, uint64_t n, uint32_t K, float* means_out, uint32_t* index_out) {
    GS_HIP(hipSetDevice(ctx->device));
    GS_TRY(gs_context_synchronize(ctx));           // the Onesweep passes assume their workgroups have the GPU to themselves (as the bake's do)
    DevBuf<float> dX, dMeans; DevBuf<uint32_t> dIndex; ClusterRun run;          // freed on every path out
    GS_HIP(dX.alloc((size_t)n * kDim * 4));
    GS_HIP(dMeans.alloc((size_t)K * kDim * 4));
    GS_HIP(dIndex.alloc((size_t)n * 4));
    hipStream_t st = ctx->stream;
    int32_t rc = cluster_run_alloc(ctx, run, n, K);
    uint32_t sortError = 0;
    hipError_t he = hipSuccess;
    if (rc == GS_OK) {
        he = hipMemcpyAsync(dX, x, (size_t)n * kDim * 4, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) rc = enqueue_cluster_shs(ctx, run, dX, n, K, dMeans, dIndex, nullptr);
        if (rc == GS_OK && he == hipSuccess) he = hipMemcpyAsync(means_out, dMeans, (size_t)K * kDim * 4, hipMemcpyDeviceToHost, st);
        if (rc == GS_OK && he == hipSuccess) he = hipMemcpyAsync(index_out, dIndex, (size_t)n * 4, hipMemcpyDeviceToHost, st);
        if (rc == GS_OK && he == hipSuccess) he = hipMemcpyAsync(&sortError, run.error.get(), 4, hipMemcpyDeviceToHost, st);
    }
    const hipError_t hs = hipStreamSynchronize(st);            // whatever failed: nothing in flight outlives the buffers
    GS_TRY(rc);
    GS_HIP(he);
    GS_HIP(hs);
    if (sortError) return fail(GS_ERR_SORT_TIMEOUT, "cluster: a bounded look-back spin expired");
    return GS_OK;
}

// gs_import_assign_clusters with a context: the means (+ their squared norms, summed on the host exactly as the host loop sums them) are uploaded
// once, the points go through one device buffer in batches; everything is enqueued on the context's stream in order and waited for at the end.
int32_t assign_clusters_gpu(gs_context* ctx, const float* x, uint64_t n, const float* means, uint32_t K, uint32_t* out) {
    GS_HIP(hipSetDevice(ctx->device));
    std::vector<double> c2(K);
    for (uint32_t j = 0; j < K; ++j) {
        double sq = 0.0;
        for (int k = 0; k < kDim; ++k) { const double m = means[(size_t)j * kDim + k]; sq += m * m; }
        c2[j] = sq;
    }
    const uint64_t batch = batch_points(n);
    DevBuf<float> dMeans, dX; DevBuf<double> dC2; DevBuf<uint32_t> dOut;      // freed on every path out
    GS_HIP(dMeans.alloc((size_t)K * kDim * 4));
    GS_HIP(dC2.alloc((size_t)K * 8));
    GS_HIP(dX.alloc((size_t)batch * kDim * 4));
    GS_HIP(dOut.alloc((size_t)batch * 4));
    hipStream_t st = ctx->stream;
    GS_HIP(hipMemcpyAsync(dMeans, means, (size_t)K * kDim * 4, hipMemcpyHostToDevice, st));
    GS_HIP(hipMemcpyAsync(dC2, c2.data(), (size_t)K * 8, hipMemcpyHostToDevice, st));
    for (uint64_t i0 = 0; i0 < n; i0 += batch) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(batch, n - i0);
        GS_HIP(hipMemcpyAsync(dX, x + (size_t)i0 * kDim, (size_t)nb * kDim * 4, hipMemcpyHostToDevice, st));
        assign_clusters_kernel<<<dim3((nb + kTile - 1) / kTile), dim3(kClusterThreads), 0, st>>>(dX, nb, dMeans, dC2, K, dOut);
        GS_HIP(hipGetLastError());
        GS_HIP(hipMemcpyAsync(out + i0, dOut, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    }
    GS_HIP(hipStreamSynchronize(st));              // (on an error path above, the hipFree calls of the buffers' handles wait for what was enqueued)
    return GS_OK;
}

} // namespace gs
