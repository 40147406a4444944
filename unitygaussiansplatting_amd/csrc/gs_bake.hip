// gs_bake.hip -- the edit path's way back into the render path's format: gs_renderer_edit_bake_asset makes, from a renderer in its current state (any
// preset, the asset's blobs or private ones, deleted bits, cutouts), a new immutable device-resident gs_asset of the ALIVE splats in the formats the
// caller asks for, Morton-reordered and chunked as GaussianSplatAssetCreator does it (GaussianSplatAssetCreator.cs:362-429, 520-638, 727-805, 873-1037)
// -- the bytes gs_import_encode (linearize = 0) produces from the same splats.  Nothing leaves the GPU.  The arithmetic is gsm::Bake* (gs_device_math.h),
// host and device from one text.  gs_asset_download_blobs reads any asset back.
//
// Plain launches on the context's stream; the only kernels that wait on other workgroups are the library's Onesweep passes.
//   1. alive list + bounds   enqueue_alive_counts, then enqueue_alive_list (gs_compact.hip): alive[j] = source index of the j-th alive splat in index order,
//                            and per workgroup the min / max of its alive positions; bounds_fold folds the partials (min / max: exact in any order).
//   2. order                 morton = 1: bake_codes writes the 63-bit code of every alive splat as two words; TwoWordSort (gs_compact.hip) -- two stable
//                            Onesweep sorts, the low word with payload = rank, then the high word gathered through the payload, 31 bits -- leaves the
//                            payload in (code, rank) order.  The sort state is the bake's own: the renderer's may be in use.  Each sort has an error
//                            word of its own and bake_finish reads both.
//   3. encode                one 256-thread workgroup per DESTINATION chunk, so that the chunk record is workgroup-uniform; lane k decodes source splat
//                            alive[order[256 c + k]] (its own source chunk ci = src >> 8) with gsm::LoadSplatDataFull from the renderer's current view.  The
//                            26 reductions run by cross-lane shuffles inside a wave and through LDS across the four.  Stores: pos / other per lane (2-16
//                            bytes, contiguous across the wave), the colour texel per lane (a chunk is one 16 x 16 tile: 16 rows of 64-256 contiguous
//                            bytes), the SH items (32 / 60 / 96 / 192 bytes) staged per wave in LDS and written as one contiguous, 16-byte aligned range
//                            with dwordx4 stores -- the shape of the export and the merge (gs_export.hip, gs_copy.hip).
// A Cluster* SH target (every one is chunked) puts the importer's palette between 2 and 3, on the GPU as well:
//   2a. SH rows              bake_sh_rows: x[i] = the 45 raw SH floats of destination splat i (coefficient-major, before the chunk normalisation) in a
//                            transient n x 180 byte buffer, staged per wave through LDS like the SH items (64 rows = 11,520 contiguous bytes).
//   2b. palette              enqueue_cluster_shs (gs_cluster.hip): seeds, training subset, four Lloyd passes, the final assignment -> K means, n indices.
//   2c. table                bake_sh_table: K x 45 floats -> K x 96 bytes (gsm::BakeEmitSHTableItem).
//   3.  encode               as above, except that no SH item is staged or written and the u16 index follows the scale in `other` (gsm::BakeEmitOther).
// The five blobs are zero-filled first, as the importer's are: the pad bytes, the texels past N and the last chunk's tail are part of the bytes.
//
// The same file is the import on the GPU, gs_import_encode_to_asset: steps 2 and 3 are templates over where a splat comes
// from -- BakeRendererSource, the above, or BakeArraySource, the six raw arrays of gs_import_input in device memory (uploaded first when they are the
// host's), linearised on the fly by gsm::ImportRecord -- and step 1 is then only the bounds: every input splat is alive.  That route accepts a BC7
// colour target: bake_encode_kernel<Src, true> compresses a chunk's 16 x 16 tile in place as sixteen mode-6 blocks, sixteen lanes (one DPP row) per
// block, and writes the texture's tiles behind the last chunk as the encoding of an all-zero block.  The bake itself still refuses BC7.
//
// gs_import_file_to_asset is that import straight from a file: two more sources, BakePlyRowsSource and BakeSpzSource, read a
// PLY's vertex rows as they lie in the file and an SPZ's gunzipped columns from one transient device buffer (gsm::PlyRowRecord / gsm::SpzRecord: the
// host readers' transpose, linearise and unpack per splat), so that the six arrays are never built; a PLY's rows get there through two pinned slices.
#include <new>

#include "gs_common.h"
#include "gs_block.h"
#include "gs_splat_file.h"

namespace gs {

struct BakeDst { uint8_t* pos; uint8_t* other; uint8_t* color; uint8_t* sh; uint8_t* chunk; uint32_t n; gsm::BakeFormats f; const uint32_t* shIndex; };   // shIndex: Cluster* SH targets only

// Where the kernels of steps 2 and 3 take splat j from (j: a place in the source's own order, before the Morton reorder).
// BakeRendererSource: the j-th alive splat of a renderer, decoded from its current view.  BakeArraySource: splat j of six raw arrays in device
// memory (gs_import_encode_to_asset), linearised on the fly: every one of them is alive, so there is no alive list.
struct BakeRendererSource {
    gsm::AssetView a; const uint32_t* alive;
    __device__ __forceinline__ gsm::V3 position(uint32_t j) const { const uint32_t src = alive[j]; return gsm::LoadSplatPosChunk(a, src, src >> 8); }
    __device__ __forceinline__ void record(uint32_t j, gsm::BakeRec& rec) const {
        const uint32_t src = alive[j], ci = src >> 8;
        gsm::SplatFull s;
        gsm::LoadSplatDataFull(a, src, ci, gsm::LoadSplatPosChunk(a, src, ci), s);
        gsm::BakeLinearRecord(s, rec);
    }
};
struct BakeArraySource {
    gsm::ImportSrc in; uint32_t linearize;
    __device__ __forceinline__ gsm::V3 position(uint32_t j) const { return { in.pos[(size_t)j * 3u], in.pos[(size_t)j * 3u + 1u], in.pos[(size_t)j * 3u + 2u] }; }
    __device__ __forceinline__ void record(uint32_t j, gsm::BakeRec& rec) const { gsm::ImportRecord(in, j, linearize, rec); }
};
// A file's own bytes in device memory (gs_import_file_to_asset): BakePlyRowsSource, vertex row j of a PLY as it lies in the file, through the table
// of property offsets; BakeSpzSource, point j of an SPZ's gunzipped columns.  What the host readers do to build the six arrays happens per splat here
struct BakePlyRowsSource {
    gsm::PlyRowSrc s;
    __device__ __forceinline__ gsm::V3 position(uint32_t j) const { return gsm::PlyRowPosition(s, j); }
    __device__ __forceinline__ void record(uint32_t j, gsm::BakeRec& rec) const { gsm::PlyRowRecord(s, j, rec); }
};
struct BakeSpzSource {
    gsm::SpzSrc s;
    __device__ __forceinline__ gsm::V3 position(uint32_t j) const { return gsm::SpzPosition(s, j); }
    __device__ __forceinline__ void record(uint32_t j, gsm::BakeRec& rec) const { gsm::SpzRecord(s, j, rec); }
};

// the alive list's partials (alive_list, gs_compact.hip) for a source whose every splat is alive: partial[block][0..2 / 3..5] = min / max of the
// positions [256 block, 256 block + 256) below n
template <class Src>
__global__ __launch_bounds__(256) void bake_source_bounds_kernel(Src src, uint32_t n, float* __restrict__ partial) {
    __shared__ float s_red[4][6];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    const bool mine = idx < n;
    const gsm::V3 pos = mine ? src.position(idx) : gsm::V3{ 0.0f, 0.0f, 0.0f };
    const float p[3] = { pos.x, pos.y, pos.z };
    block_bounds(mine, p, threadIdx.x & 63u, threadIdx.x >> 6, s_red);
    __syncthreads();
    block_bounds_store(s_red, partial + blockIdx.x * 6u);
}

// the Morton code of the source's splat j as two sort keys, and the identity payload
template <class Src>
__global__ __launch_bounds__(256) void bake_codes_kernel(Src src, const float* __restrict__ bounds, uint32_t total,
                                                         uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, uint32_t* __restrict__ rank) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= total) return;
    const unsigned long long code = gsm::BakeMortonCode(src.position(j), bounds, bounds + 3);
    lo[j] = (uint32_t)code; hi[j] = (uint32_t)(code >> 32); rank[j] = j;
}

// bytes in { 2, 4, 6, 8, 10, 12, 16, 18 } of w (5 words) to p; p is `bytes`-strided from an aligned base: a multiple of 4 bytes = dword stores, else
// halfword stores
__device__ __forceinline__ void bake_store(uint8_t* p, const uint32_t* w, uint32_t bytes) {
    if ((bytes & 3u) == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) if (k * 4u < bytes) ((uint32_t*)p)[k] = w[k];
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 9u; ++k) if (k * 2u < bytes) ((uint16_t*)p)[k] = (uint16_t)(w[k >> 1] >> ((k & 1u) * 16u));
    }
}

// words [0, words) of a wave's LDS staging area to dst, contiguous and 16-byte aligned: dwordx4 stores, then the few words left
__device__ __forceinline__ void bake_flush_wave(uint8_t* dst, const uint32_t* staged, uint32_t words, uint32_t lane) {
    const uint32_t quads = words / 4u;
    for (uint32_t q = lane; q < quads; q += 64u) ((uint4*)dst)[q] = ((const uint4*)staged)[q];
    if (quads * 4u + lane < words) ((uint32_t*)dst)[quads * 4u + lane] = staged[quads * 4u + lane];
}

// rows[i] = the 45 raw SH floats of destination splat i: what cluster_shs of the importer is given (gs_import.cpp: x[i] = s[order[i]].sh)
template <class Src>
__global__ __launch_bounds__(256) void bake_sh_rows_kernel(Src src, const uint32_t* __restrict__ order, uint32_t n, float* __restrict__ rows) {
    __shared__ __attribute__((aligned(16))) uint32_t s_sh[4][64 * 45];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (i < n) {
        gsm::BakeRec rec;
        src.record(order ? order[i] : i, rec);
        uint32_t* row = s_sh[wave] + lane * 45u;
#pragma unroll
        for (int k = 0; k < 45; ++k) row[k] = gsm::f2u(rec.sh[k]);
    }
    __syncthreads();
    const uint32_t waveFirst = blockIdx.x * 256u + wave * 64u;      // 64 rows of 180 bytes: every wave's range starts 16-byte aligned
    if (waveFirst < n) bake_flush_wave((uint8_t*)rows + (size_t)waveFirst * 180u, s_sh[wave], (n - waveFirst < 64u ? n - waveFirst : 64u) * 45u, lane);
}

// the SH table of a Cluster* target: one thread per entry, 96 bytes = six dwordx4 stores
__global__ __launch_bounds__(256) void bake_sh_table_kernel(const float* __restrict__ means, uint32_t K, uint8_t* __restrict__ table) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= K) return;
    float m[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) m[k] = means[(size_t)j * 45u + k];
    uint32_t w[24];
    gsm::BakeEmitSHTableItem(m, w);
    uint4* out = (uint4*)(table + (size_t)j * 96u);
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// One step of a reduction over a DPP row: the sixteen lanes whose index shares its upper bits, which in bake_encode_kernel are the sixteen texels of
// one BC7 block.  Quad swaps (lane ^ 1, lane ^ 2), then the half-row and the row mirrored: after the four steps every lane holds the row's result.
// All lanes of the wave are active where this is used.
template <int CTRL> __device__ __forceinline__ uint32_t row_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false); }
constexpr int kDppQuadXor1 = 0xB1, kDppQuadXor2 = 0x4E, kDppRowHalfMirror = 0x141, kDppRowMirror = 0x140;
__device__ __forceinline__ float row_min(float v) {
    v = fminf(v, gsm::u2f(row_dpp<kDppQuadXor1>(gsm::f2u(v))));
    v = fminf(v, gsm::u2f(row_dpp<kDppQuadXor2>(gsm::f2u(v))));
    v = fminf(v, gsm::u2f(row_dpp<kDppRowHalfMirror>(gsm::f2u(v))));
    return fminf(v, gsm::u2f(row_dpp<kDppRowMirror>(gsm::f2u(v))));
}
__device__ __forceinline__ float row_max(float v) {
    v = fmaxf(v, gsm::u2f(row_dpp<kDppQuadXor1>(gsm::f2u(v))));
    v = fmaxf(v, gsm::u2f(row_dpp<kDppQuadXor2>(gsm::f2u(v))));
    v = fmaxf(v, gsm::u2f(row_dpp<kDppRowHalfMirror>(gsm::f2u(v))));
    return fmaxf(v, gsm::u2f(row_dpp<kDppRowMirror>(gsm::f2u(v))));
}
__device__ __forceinline__ uint32_t row_or(uint32_t v) {
    v |= row_dpp<kDppQuadXor1>(v);
    v |= row_dpp<kDppQuadXor2>(v);
    v |= row_dpp<kDppRowHalfMirror>(v);
    return v | row_dpp<kDppRowMirror>(v);
}

// The BC7 colour texel of a chunk's lane (gsm::BC7*: bc7_encode_mode6 of the importer with one texel per lane): the sixteen lanes of a row are one
// 4 x 4 block of the chunk's 16 x 16 tile.  Channel minima / maxima over the row, the endpoints redundantly per lane, the lane's own index, the
// sixteen indices gathered in the block's texel order, one 16-byte store by the row's first lane.  A lane past N takes part with a zero texel, as
// the importer's zero-initialised texture has it.
__device__ __forceinline__ void bake_store_bc7(uint8_t* color, uint32_t i, bool mine, const gsm::V4& col) {
    float px[4], lo[4], hi[4];
    gsm::BC7Texel(mine ? col : gsm::V4{ 0.0f, 0.0f, 0.0f, 0.0f }, px);
#pragma unroll
    for (int c = 0; c < 4; ++c) { lo[c] = row_min(px[c]); hi[c] = row_max(px[c]); }
    gsm::BC7Block b;
    gsm::BC7Endpoints(lo, hi, b);
    const uint32_t at = gsm::BC7TexelOfLane(i) * 4u;
    const uint32_t index = gsm::BC7TexelIndex(b, px);
    const uint32_t nibLo = row_or(at < 32u ? index << at : 0u), nibHi = row_or(at < 32u ? 0u : index << (at - 32u));
    if ((i & 15u) != 0u) return;
    uint32_t w[4];
    gsm::BC7Pack(b, ((uint64_t)nibHi << 32) | nibLo, w);
    *(uint4*)(color + gsm::BC7BlockOfSplat(i) * 16u) = make_uint4(w[0], w[1], w[2], w[3]);
}

// BC7: the colour target is GS_COLOR_BC7 (d.f.color == 3), and the grid covers every 16 x 16 tile of the texture, not only the chunks: a workgroup
// past the last chunk writes its tile's sixteen blocks as the encoding of an all-zero block, which is not zero bytes.
template <class Src, bool BC7>
__global__ __launch_bounds__(256) void bake_encode_kernel(Src src, const uint32_t* __restrict__ order, BakeDst d) {
    __shared__ float s_red[4][2 * gsm::kBakeCols];
    __shared__ __attribute__((aligned(16))) uint32_t s_sh[4][64 * 48];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (BC7 && blockIdx.x * 256u >= d.n) {                         // (workgroup-uniform: the texture has tiles behind the last chunk)
        if (threadIdx.x < 16u) *(uint4*)(d.color + gsm::BC7BlockOfSplat(blockIdx.x * 256u + threadIdx.x * 16u) * 16u) = make_uint4(0x40u, 0u, 0u, 0u);
        return;
    }
    const bool mine = i < d.n;
    gsm::BakeRec rec;
    if (mine) src.record(order ? order[i] : i, rec);
    if (d.f.chunked) {                                             // (workgroup-uniform)
        gsm::BakeBounds b;
        gsm::BakeBoundsEmpty(b);
        if (mine) { gsm::BakeChunkSpace(rec); gsm::BakeBoundsOf(rec, b); }
#pragma unroll
        for (int c = 0; c < gsm::kBakeCols; ++c) {
            const float mn = wave_min(b.mn[c]), mx = wave_max(b.mx[c]);
            if (lane == 0u) { s_red[wave][c] = mn; s_red[wave][gsm::kBakeCols + c] = mx; }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < gsm::kBakeCols; ++c) {
            b.mn[c] = fminf(fminf(s_red[0][c], s_red[1][c]), fminf(s_red[2][c], s_red[3][c]));
            b.mx[c] = fmaxf(fmaxf(s_red[0][gsm::kBakeCols + c], s_red[1][gsm::kBakeCols + c]), fmaxf(s_red[2][gsm::kBakeCols + c], s_red[3][gsm::kBakeCols + c]));
        }
        gsm::BakeBoundsWiden(b);
        if (threadIdx.x == 0u) {
            uint32_t w[16];
            gsm::BakeChunkWords(b, w);
            uint4* out = (uint4*)(d.chunk + (size_t)blockIdx.x * 64u);
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        }
        if (mine) gsm::BakeNormalise(rec, b);
    }
    const bool clustered = gsm::shIsClustered(d.f.sh);             // (kernel-uniform) the SH blob is the table: no item per splat
    const uint32_t shWords = gsm::shStrideOf(d.f.sh) / 4u;
    if (mine && !clustered) {
        uint32_t w[48];
        gsm::BakeEmitSH(rec.sh, d.f.sh, w);
        uint32_t* s = s_sh[wave] + lane * shWords;
#pragma unroll
        for (uint32_t k = 0; k < 48u; ++k) if (k < shWords) s[k] = w[k];
    }
    __syncthreads();
    const uint32_t waveFirst = blockIdx.x * 256u + wave * 64u;      // the wave's first destination record; its lanes that write are a prefix
    if (waveFirst < d.n && !clustered) {
        const uint32_t waveCount = d.n - waveFirst < 64u ? d.n - waveFirst : 64u;
        bake_flush_wave(d.sh + (size_t)waveFirst * (shWords * 4u), s_sh[wave], waveCount * shWords, lane);     // 16-byte aligned: 64 records of a multiple of 4 bytes
    }
    if (BC7) bake_store_bc7(d.color, i, mine, rec.col);            // (every lane of the workgroup: the rows reduce across lanes past N too)
    if (!mine) return;
    uint32_t w[5];
    gsm::BakeEmitVec(rec.pos, d.f.pos, w);
    const uint32_t posSz = gsm::vecStride(d.f.pos);
    bake_store(d.pos + (size_t)i * posSz, w, posSz);
    const uint32_t othSz = gsm::BakeEmitOther(rec.rot, rec.scale, d.f.scale, clustered, clustered ? d.shIndex[i] : 0u, w);
    bake_store(d.other + (size_t)i * othSz, w, othSz);
    if (BC7) return;
    uint32_t px, py;
    gsm::SplatIndexToPixelIndex(i, px, py);
    gsm::BakeEmitColor(rec.col, d.f.color, w);
    const uint32_t colSz = d.f.color == 0u ? 16u : (d.f.color == 1u ? 8u : 4u);
    bake_store(d.color + ((size_t)py * 2048u + px) * colSz, w, colSz);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// everything a bake holds besides the asset it makes: freed when the call returns
struct BakeRun {
    DevBuf<uint32_t> counts, base, alive;
    DevBuf<float> partial, bounds;
    TwoWordSort keys;                       // morton = 1: the Morton codes and their order
    DevBuf<float> shRows, shMeans;          // a Cluster* SH target: the n x 45 SH rows in destination order, the K x 45 means,
    DevBuf<uint32_t> shIndex;               // the n table indices
    ClusterRun cluster;                     // and the Lloyd loop's own state
};

// what steps 2 and 3 need besides the source: the sort's buffers and state (morton = 1), the palette's (a Cluster* SH target)
static int32_t bake_run_alloc(gs_context* ctx, const gs_import_formats* f, BakeRun& run, uint32_t total) {
    GS_HIP(run.bounds.alloc(6 * 4));
    if (f->morton) GS_TRY(run.keys.alloc(ctx, total));
    const uint32_t K = gsm::shClusterCount(f->sh_format);
    if (K) {                                                       // n x 184 bytes + the subset and the sort state: freed with `run`
        GS_HIP(run.shRows.alloc((size_t)total * 180));
        GS_HIP(run.shIndex.alloc((size_t)total * 4));
        GS_HIP(run.shMeans.alloc((size_t)K * 180));
        GS_TRY(cluster_run_alloc(ctx, run.cluster, total, K));
    }
    return GS_OK;
}

// the encode of `total` splats of `src` in `order`: a BC7 colour target takes the kernel with the block encoder compiled in, over every tile of the
// colour texture (256 texels of one byte each)
template <class Src>
static void bake_launch_encode(hipStream_t st, const Src& src, const uint32_t* order, uint32_t total, const BakeDst& d, uint64_t colorBytes) {
    if (d.f.color == GS_COLOR_BC7) hipLaunchKernelGGL((bake_encode_kernel<Src, true>), dim3((uint32_t)(colorBytes / 256u)), dim3(256), 0, st, src, order, d);
    else hipLaunchKernelGGL((bake_encode_kernel<Src, false>), dim3((total + 255u) / 256u), dim3(256), 0, st, src, order, d);
}

// steps 2 and 3 for any source, run.bounds already enqueued.  ev: null, or six events -- 4 and 5 are recorded here, after the sorts and after the
// encode.  cev: null, or twelve events of a Cluster* target -- before and after the SH rows, enqueue_cluster_shs' nine further ones, after the
// table + encode
template <class Src>
static int32_t bake_enqueue_from(gs_context* ctx, const Src& src, const gs_import_formats* f, BakeRun& run, uint32_t total, BakeDst d, uint64_t colorBytes,
                                 Event* ev, const hipEvent_t* cev) {
    hipStream_t st = ctx->stream;
    const uint32_t blocks = (total + 255u) / 256u;
    if (f->morton) {
        hipLaunchKernelGGL(bake_codes_kernel<Src>, dim3(blocks), dim3(256), 0, st, src, (const float*)run.bounds.get(), total, run.keys.lo.get(), run.keys.hi.get(),
                           run.keys.rank.get());
        GS_HIP(hipGetLastError());
        GS_TRY(run.keys.enqueue(ctx, total));
    }
    if (ev) GS_HIP(hipEventRecord(ev[4], st));
    const uint32_t* order = f->morton ? (const uint32_t*)run.keys.rank.get() : (const uint32_t*)nullptr;
    const uint32_t K = gsm::shClusterCount(f->sh_format);
    if (K) {
        if (cev) GS_HIP(hipEventRecord(cev[0], st));
        hipLaunchKernelGGL(bake_sh_rows_kernel<Src>, dim3(blocks), dim3(256), 0, st, src, order, total, run.shRows.get());
        GS_HIP(hipGetLastError());
        GS_TRY(enqueue_cluster_shs(ctx, run.cluster, run.shRows, total, K, run.shMeans, run.shIndex, cev ? cev + 1 : nullptr));      // (records cev[1 .. 10])
        hipLaunchKernelGGL(bake_sh_table_kernel, dim3((K + 255u) / 256u), dim3(256), 0, st, (const float*)run.shMeans.get(), K, d.sh);
        d.shIndex = run.shIndex;
    }
    bake_launch_encode(st, src, order, total, d, colorBytes);
    GS_HIP(hipGetLastError());
    if (ev) GS_HIP(hipEventRecord(ev[5], st));
    if (K && cev) GS_HIP(hipEventRecord(cev[11], st));
    return GS_OK;
}

// steps 1 (second half) to 3 of a renderer's bake on the context's stream; the caller synchronises whatever this returns.  ev: null, or six events --
// 2 and 3 are recorded here, before the alive list and after the bounds, 4 and 5 by bake_enqueue_from
static int32_t bake_enqueue(gs_renderer* r, const gs_import_formats* f, BakeRun& run, uint32_t chunks, uint32_t total, BakeDst d, uint64_t colorBytes, Event* ev,
                            const hipEvent_t* cev) {
    gs_context* ctx = r->ctx;
    hipStream_t st = ctx->stream;
    GS_HIP(run.alive.alloc(((size_t)total + 16) * 4));
    GS_HIP(run.partial.alloc((size_t)chunks * 6 * 4));
    GS_TRY(bake_run_alloc(ctx, f, run, total));
    const BakeRendererSource src = { asset_view(r), run.alive.get() };
    if (ev) GS_HIP(hipEventRecord(ev[2], st));
    GS_TRY(enqueue_alive_list(st, src.a, edit_view(r), false, false, AliveXform{}, chunks, run.base.get(), run.alive.get(), run.partial.get(), run.bounds.get()));
    if (ev) GS_HIP(hipEventRecord(ev[3], st));
    return bake_enqueue_from(ctx, src, f, run, total, d, colorBytes, ev, cev);
}

// the new asset of a bake or an import: every blob padded like an owned upload's (the decoders' trailing-dword reads) and zero-filled on the
// context's stream, as the importer's are.  On failure nothing is left allocated
static int32_t bake_asset_alloc(gs_context* ctx, const uint64_t need[5], gs_asset** out) {
    gs_asset* a = new (std::nothrow) gs_asset();
    if (!a) return fail(GS_ERR_OUT_OF_MEMORY, "host allocation");
    a->ctx = ctx; a->owned = true;
    for (int k = 0; k < 5; ++k) {
        a->sizes[k] = need[k];
        if (!need[k]) continue;
        hipError_t e = a->ownedBlobs[k].alloc((size_t)need[k] + 16);
        a->blobs[k] = a->ownedBlobs[k];
        if (e == hipSuccess) e = hipMemsetAsync(a->blobs[k], 0, (size_t)need[k] + 16, ctx->stream);
        if (e != hipSuccess) {
            const int32_t rc = fail_hip(e, "bake: allocate blob", __FILE__, __LINE__);
            (void)hipStreamSynchronize(ctx->stream);
            (void)gs_asset_destroy(a);
            return rc;
        }
    }
    *out = a;
    return GS_OK;
}
static BakeDst bake_dst_of(const gs_asset* a, uint32_t total, const gs_import_formats* f) {
    BakeDst d;
    d.pos = (uint8_t*)a->blobs[0]; d.other = (uint8_t*)a->blobs[1]; d.color = (uint8_t*)a->blobs[2]; d.sh = (uint8_t*)a->blobs[3]; d.chunk = (uint8_t*)a->blobs[4];
    d.n = total;
    d.f = { f->pos_format, f->scale_format, f->color_format, f->sh_format, a->sizes[4] != 0 ? 1u : 0u };
    d.shIndex = nullptr;
    return d;
}
// what follows the enqueue (rc: its result): the bounds and the sorts' error words read back, the stream drained -- whatever failed, nothing in
// flight outlives the transient buffers or the asset -- and the asset's view filled in, or the asset destroyed
static int32_t bake_finish(gs_context* ctx, int32_t rc, BakeRun& run, const gs_import_formats* f, gs_asset* a, uint32_t total, float hostBounds[6]) {
    hipStream_t st = ctx->stream;
    uint32_t sortError[2] = { 0u, 0u }, clusterSortError = 0;
    if (rc == GS_OK) {
        hipError_t he = hipMemcpyAsync(hostBounds, run.bounds.get(), 6 * sizeof(float), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess && f->morton) he = run.keys.enqueue_error_readback(st, sortError);
        if (he == hipSuccess && f->sh_format > GS_SH_NORM6) he = hipMemcpyAsync(&clusterSortError, run.cluster.error.get(), 4, hipMemcpyDeviceToHost, st);
        if (he != hipSuccess) rc = fail_hip(he, "bake: read back", __FILE__, __LINE__);
    }
    rc = drain(st, rc, "bake");
    if (rc == GS_OK && (sortError[0] | sortError[1] | clusterSortError)) rc = fail(GS_ERR_SORT_TIMEOUT, "bake: a bounded look-back spin expired");
    if (rc != GS_OK) { (void)gs_asset_destroy(a); return rc; }
    gsm::AssetView& v = a->view;
    v.pos = (const uint8_t*)a->blobs[0]; v.other = (const uint8_t*)a->blobs[1]; v.color = (const uint8_t*)a->blobs[2]; v.sh = (const uint8_t*)a->blobs[3];
    v.chunk = (const uint8_t*)a->blobs[4];
    v.n = total; v.posFmt = f->pos_format; v.scaleFmt = f->scale_format; v.colorFmt = f->color_format; v.shFmt = f->sh_format;
    v.chunkCount = a->sizes[4] ? (total + 255u) / 256u : 0u;
    return GS_OK;
}

static int32_t bake_impl(gs_renderer* r, const gs_import_formats* f, gs_asset** out, uint32_t* alive, float bounds_min[3], float bounds_max[3], Event* ev = nullptr,
                         const hipEvent_t* cev = nullptr) {
    if (out) *out = nullptr;
    if (!r || !f || !out || !alive) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (r->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane holds no edit state: bake its owner");
    if (f->pos_format > 3 || f->scale_format > 3 || f->color_format > 3 || f->sh_format > 8) return fail(GS_ERR_INVALID_ARGUMENT, "format enum out of range");
    if (f->linearize != 0) return fail(GS_ERR_INVALID_ARGUMENT, "bake: linearize must be 0 (the renderer's data is linear)");
    if (f->morton > 1) return fail(GS_ERR_INVALID_ARGUMENT, "bake: morton must be 0 or 1");
    if (f->color_format == GS_COLOR_BC7) return fail(GS_ERR_INVALID_ARGUMENT, "bake: a BC7 colour target is not supported");
    if (r->n == 0u) return fail(GS_ERR_INVALID_ARGUMENT, "bake: no alive splat");
    GS_HIP(hipSetDevice(r->ctx->device));
    // after everything already enqueued, the lanes' frames included: the sort below assumes its workgroups have the GPU to themselves the way the
    // renderer's own full sorts do
    GS_TRY(gs_context_synchronize(r->ctx));
    hipStream_t st = r->ctx->stream;
    const uint32_t chunks = (r->n + 255u) / 256u;
    BakeRun run;
    GS_HIP(run.counts.alloc((size_t)chunks * 4));
    GS_HIP(run.base.alloc(((size_t)chunks + 1) * 4));
    if (ev) GS_HIP(hipEventRecord(ev[0], st));
    GS_TRY(enqueue_alive_counts(st, asset_view(r), edit_view(r), false, chunks, run.counts.get(), run.base.get()));
    if (ev) GS_HIP(hipEventRecord(ev[1], st));
    uint32_t total = 0;
    GS_TRY(drain(st, [&]() -> int32_t { GS_HIP(hipMemcpyAsync(&total, run.base.get() + chunks, 4, hipMemcpyDeviceToHost, st)); return GS_OK; }(), "bake: the alive count"));
    if (total == 0u) return fail(GS_ERR_INVALID_ARGUMENT, "bake: no alive splat");
    uint64_t need[5];
    GS_TRY(gs_import_blob_sizes(total, f, need));               // (a Cluster* SH target needs more alive splats than table entries: the importer's rule)
    gs_asset* a = nullptr;
    GS_TRY(bake_asset_alloc(r->ctx, need, &a));
    float hostBounds[6] = { 0, 0, 0, 0, 0, 0 };
    const int32_t rc = bake_enqueue(r, f, run, chunks, total, bake_dst_of(a, total, f), need[2], ev, cev);
    GS_TRY(bake_finish(r->ctx, rc, run, f, a, total, hostBounds));
    *alive = total;
    for (int c = 0; c < 3; ++c) {
        if (bounds_min) bounds_min[c] = hostBounds[c];
        if (bounds_max) bounds_max[c] = hostBounds[3 + c];
    }
    *out = a;
    return GS_OK;
}

// What every import does once its source lies in device memory: the per-workgroup bounds partials + the bake's fold, steps 2 and 3 as the bake runs
// them, bake_finish.  Whatever fails, the stream is drained before this returns: the caller's upload may still be in flight.  ev: null, or six events
// -- 3 after the bounds, 4 / 5 by bake_enqueue_from
template <class Src>
static int32_t import_from_source(gs_context* ctx, const Src& src, const gs_import_formats* f, uint32_t total, const uint64_t need[5], BakeRun& run, gs_asset** out,
                                  float bounds_min[3], float bounds_max[3], Event* ev, const hipEvent_t* cev) {
    hipStream_t st = ctx->stream;
    const uint32_t blocks = (total + 255u) / 256u;
    {
        const int32_t rcAlloc = [&]() -> int32_t { GS_HIP(run.partial.alloc((size_t)blocks * 6 * 4)); return bake_run_alloc(ctx, f, run, total); }();
        if (rcAlloc != GS_OK) { (void)hipStreamSynchronize(st); return rcAlloc; }       // (the uploads may still be in flight)
    }
    gs_asset* a = nullptr;
    {
        const int32_t rcAsset = bake_asset_alloc(ctx, need, &a);
        if (rcAsset != GS_OK) { (void)hipStreamSynchronize(st); return rcAsset; }
    }
    int32_t rc = [&]() -> int32_t {
        hipLaunchKernelGGL(bake_source_bounds_kernel<Src>, dim3(blocks), dim3(256), 0, st, src, total, run.partial.get());
        GS_TRY(enqueue_bounds_fold(st, run.partial.get(), blocks, run.bounds.get(), false));
        if (ev) GS_HIP(hipEventRecord(ev[3], st));
        return bake_enqueue_from(ctx, src, f, run, total, bake_dst_of(a, total, f), need[2], ev, cev);
    }();
    float hostBounds[6] = { 0, 0, 0, 0, 0, 0 };
    GS_TRY(bake_finish(ctx, rc, run, f, a, total, hostBounds));
    for (int c = 0; c < 3; ++c) {
        if (bounds_min) bounds_min[c] = hostBounds[c];
        if (bounds_max) bounds_max[c] = hostBounds[3 + c];
    }
    *out = a;
    return GS_OK;
}

// gs_import_encode_to_asset: the importer's pipeline with the six raw arrays as the source.  memory_kind 0 copies them into transient device buffers
// (N x 236 bytes) first; then per-workgroup bounds partials + the bake's fold, and steps 2 and 3 as the bake runs them.  One stream; everything
// transient is freed when the call returns.  ev: null, or six events -- 0 / 1 around the upload, 3 after the bounds, 4 / 5 by bake_enqueue_from
static int32_t import_impl(gs_context* ctx, const gs_import_input* in, uint32_t memory_kind, const gs_import_formats* f, gs_asset** out, float bounds_min[3],
                           float bounds_max[3], Event* ev = nullptr, const hipEvent_t* cev = nullptr) {
    if (out) *out = nullptr;
    if (!ctx || !in || !f || !out) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (!in->pos || !in->dc0 || !in->sh || !in->opacity || !in->scale || !in->rot) return fail(GS_ERR_INVALID_ARGUMENT, "an input array is null");
    if (f->linearize > 1 || f->morton > 1) return fail(GS_ERR_INVALID_ARGUMENT, "import: linearize and morton must be 0 or 1");
    if (memory_kind > 1) return fail(GS_ERR_INVALID_ARGUMENT, "import: memory_kind must be 0 (host arrays) or 1 (device arrays)");
    const uint32_t total = in->splat_count;
    uint64_t need[5];
    GS_TRY(gs_import_blob_sizes(total, f, need));               // (no splats, an enum out of range, a Cluster* target with too few splats)
    GS_HIP(hipSetDevice(ctx->device));
    GS_TRY(gs_context_synchronize(ctx));                        // the sorts need the GPU the way the bake's do
    hipStream_t st = ctx->stream;
    BakeRun run;
    DevBuf<float> up[6];
    const float* arrays[6] = { in->pos, in->dc0, in->sh, in->opacity, in->scale, in->rot };
    if (ev) GS_HIP(hipEventRecord(ev[0], st));
    if (memory_kind == 0u) {
        const size_t floats[6] = { 3, 3, 45, 1, 3, 4 };
        for (int k = 0; k < 6; ++k) GS_HIP(up[k].alloc((size_t)total * floats[k] * 4));
        hipError_t he = hipSuccess;
        for (int k = 0; k < 6 && he == hipSuccess; ++k) he = hipMemcpyAsync(up[k].get(), arrays[k], (size_t)total * floats[k] * 4, hipMemcpyHostToDevice, st);
        if (he != hipSuccess) { (void)hipStreamSynchronize(st); return fail_hip(he, "import: upload", __FILE__, __LINE__); }
        for (int k = 0; k < 6; ++k) arrays[k] = up[k].get();
    }
    if (ev) GS_HIP(hipEventRecord(ev[1], st));
    const BakeArraySource src = { { arrays[0], arrays[1], arrays[2], arrays[3], arrays[4], arrays[5] }, f->linearize };
    return import_from_source(ctx, src, f, total, need, run, out, bounds_min, bounds_max, ev, cev);
}

// the pinned slice of a PLY upload when the caller names none, and the smallest one it may name
constexpr size_t kFileSliceDefault = (size_t)64 << 20, kFileSliceMin = 4096;

// A PLY's vertex rows from the file's stream to dev[0, bytes) through two pinned slices, filled alternately: fread into one while the other's copy is
// in flight; the slice's event says when it may be refilled.  Whatever happens, the stream is drained before the slices are freed
static int32_t upload_ply_rows(hipStream_t st, gs_splat_file* file, uint8_t* dev, size_t bytes, size_t slice) {
    if (fseeko(file->f, file->bodyAt, SEEK_SET) != 0) return fail(GS_ERR_INVALID_ASSET, "PLY read error: the file cannot be positioned at its vertex rows");
    PinnedBuf<uint8_t> pin[2];
    Event refill[2];
    for (int k = 0; k < 2; ++k) {
        GS_HIP(pin[k].alloc(slice, hipHostMallocDefault));
        GS_HIP(refill[k].create(hipEventDisableTiming));
    }
    int32_t rc = GS_OK;
    size_t done = 0;
    for (uint32_t turn = 0; done < bytes && rc == GS_OK; ++turn) {
        const int k = (int)(turn & 1u);
        const size_t want = bytes - done < slice ? bytes - done : slice;
        hipError_t he = turn >= 2u ? hipEventSynchronize(refill[k]) : hipSuccess;       // the copy out of this slice two turns ago
        if (he == hipSuccess) {
            if (fread(pin[k].get(), 1, want, file->f) != want) { rc = fail(GS_ERR_INVALID_ASSET, "PLY read error: fewer data bytes than the header announces"); break; }
            he = hipMemcpyAsync(dev + done, pin[k].get(), want, hipMemcpyHostToDevice, st);
        }
        if (he == hipSuccess) he = hipEventRecord(refill[k], st);
        if (he != hipSuccess) rc = fail_hip(he, "import: upload the vertex rows", __FILE__, __LINE__);
        done += want;
    }
    (void)hipStreamSynchronize(st);                                 // before the slices are freed
    return rc;
}

// gs_import_file_to_asset: the importer's pipeline with the file's own bytes as the source.  The body goes to one transient device buffer (a PLY's
// rows through upload_ply_rows, an SPZ's gunzipped stream as it is), then import_from_source with BakePlyRowsSource / BakeSpzSource.  One stream;
// everything transient is freed when the call returns.  ev: null, or six events -- 0 / 1 around the upload, the rest as in import_impl
static int32_t import_file_impl(gs_context* ctx, gs_splat_file* file, const gs_import_formats* f, uint32_t slice_bytes, gs_asset** out, float bounds_min[3],
                                float bounds_max[3], Event* ev = nullptr, const hipEvent_t* cev = nullptr) {
    if (out) *out = nullptr;
    if (!ctx || !file || !f || !out) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (!splat_file_is_open(file)) return fail(GS_ERR_INVALID_ARGUMENT, "not an open splat file handle");
    const gs_splat_file_info& fi = file->info;
    const bool ply = fi.kind == GS_SPLAT_FILE_PLY;
    if (f->linearize != (ply ? 1u : 0u)) return fail(GS_ERR_INVALID_ARGUMENT, "import: linearize must be 1 for a PLY file and 0 for an SPZ file");
    if (f->morton > 1) return fail(GS_ERR_INVALID_ARGUMENT, "import: morton must be 0 or 1");
    if (slice_bytes != 0u && slice_bytes < kFileSliceMin) return fail(GS_ERR_INVALID_ARGUMENT, "import: slice_bytes must be 0 or at least 4096");
    const uint32_t total = fi.splat_count;
    uint64_t need[5];
    GS_TRY(gs_import_blob_sizes(total, f, need));               // (an enum out of range, a Cluster* target with too few splats)
    GS_HIP(hipSetDevice(ctx->device));
    GS_TRY(gs_context_synchronize(ctx));                        // the sorts need the GPU the way the bake's do
    hipStream_t st = ctx->stream;
    BakeRun run;
    DevBuf<uint8_t> body;
    const size_t bytes = (size_t)fi.body_bytes;
    GS_HIP(body.alloc(bytes));
    if (ev) GS_HIP(hipEventRecord(ev[0], st));
    if (ply) {
        size_t slice = slice_bytes ? (size_t)slice_bytes : kFileSliceDefault;
        const size_t whole = (bytes + kFileSliceMin - 1) / kFileSliceMin * kFileSliceMin;      // no slice larger than the body needs
        if (slice > whole) slice = whole;
        GS_TRY(upload_ply_rows(st, file, body.get(), bytes, slice));
    } else {
        const hipError_t he = hipMemcpyAsync(body.get(), file->raw.data(), bytes, hipMemcpyHostToDevice, st);
        if (he != hipSuccess) { (void)hipStreamSynchronize(st); return fail_hip(he, "import: upload", __FILE__, __LINE__); }
    }
    if (ev) {
        const hipError_t he = hipEventRecord(ev[1], st);
        if (he != hipSuccess) { (void)hipStreamSynchronize(st); return fail_hip(he, "import: event", __FILE__, __LINE__); }
    }
    if (ply) {
        BakePlyRowsSource src;
        src.s.rows = body.get(); src.s.stride = fi.stride;
        for (int k = 0; k < gsm::kPlyOffsets; ++k) src.s.off[k] = fi.offsets[k];
        gsm::PlyRowLayout(src.s);                                   // dword loads where everything is aligned, the INRIA layout's merged ones where it is that
        return import_from_source(ctx, src, f, total, need, run, out, bounds_min, bounds_max, ev, cev);
    }
    const BakeSpzSource src = { { body.get(), total, fi.sh_level == 1u ? 3u : (fi.sh_level == 2u ? 8u : (fi.sh_level == 3u ? 15u : 0u)), fi.fract_bits } };
    return import_from_source(ctx, src, f, total, need, run, out, bounds_min, bounds_max, ev, cev);
}

// the events of a finished import as the five stage times the timing scripts report
static int32_t import_stage_times(const gs_import_formats* formats, const Event* ev, const hipEvent_t* cev, float ms[5]) {
    const bool palette = formats->sh_format > GS_SH_NORM6;
    GS_HIP(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    GS_HIP(hipEventElapsedTime(&ms[1], ev[1], ev[3]));
    GS_HIP(hipEventElapsedTime(&ms[2], ev[3], ev[4]));
    ms[3] = 0.0f;
    if (palette) GS_HIP(hipEventElapsedTime(&ms[3], cev[0], cev[10]));
    if (palette) GS_HIP(hipEventElapsedTime(&ms[4], cev[10], cev[11]));
    else GS_HIP(hipEventElapsedTime(&ms[4], ev[4], ev[5]));
    return GS_OK;
}

} // namespace gs

using namespace gs;

extern "C" {

int32_t gs_renderer_edit_bake_asset(gs_renderer* r, const gs_import_formats* formats, gs_asset** out, uint32_t* alive, float bounds_min[3], float bounds_max[3]) {
    return bake_impl(r, formats, out, alive, bounds_min, bounds_max);
}

int32_t gs_import_encode_to_asset(gs_context* ctx, const gs_import_input* in, uint32_t memory_kind, const gs_import_formats* formats, gs_asset** out,
                                  float bounds_min[3], float bounds_max[3]) {
    return import_impl(ctx, in, memory_kind, formats, out, bounds_min, bounds_max);
}

int32_t gs_import_file_to_asset(gs_context* ctx, gs_splat_file* file, const gs_import_formats* formats, uint32_t slice_bytes, gs_asset** out,
                                float bounds_min[3], float bounds_max[3]) {
    return import_file_impl(ctx, file, formats, slice_bytes, out, bounds_min, bounds_max);
}

int32_t gs_asset_download_blobs(const gs_asset* asset, void* const blobs[5], const uint64_t sizes[5]) {
    if (!asset || !blobs || !sizes) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    for (int k = 0; k < 5; ++k)
        if (blobs[k] && sizes[k] > (asset->blobs[k] ? asset->sizes[k] : 0u)) return fail(GS_ERR_INVALID_ARGUMENT, "more bytes asked for than the blob holds");
    GS_HIP(hipSetDevice(asset->ctx->device));
    hipStream_t st = asset->ctx->stream;
    hipError_t he = hipSuccess;
    for (int k = 0; k < 5 && he == hipSuccess; ++k)
        if (blobs[k] && sizes[k]) he = hipMemcpyAsync(blobs[k], asset->blobs[k], (size_t)sizes[k], hipMemcpyDeviceToHost, st);
    return drain(st, he == hipSuccess ? GS_OK : fail_hip(he, "download_blobs", __FILE__, __LINE__), "download_blobs");
}

// A measurement aid of scripts/bake_timing.py, which binds it itself: not declared in gsplat_c.h, not part of the ABI.  One whole bake whose asset is
// destroyed again; ms[0..3] = GPU milliseconds of alive_count + export_scan, of the alive list + bounds, of the Morton codes + the two sorts, of the encode.
__attribute__((visibility("default"))) int32_t gs_bake_stage_times_for_scripts(gs_renderer* r, const gs_import_formats* formats, float ms[4], uint32_t* alive) {
    if (!r || !formats || !ms || !alive) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    GS_HIP(hipSetDevice(r->ctx->device));
    Event ev[6];
    for (Event& e : ev) GS_HIP(e.create(hipEventDefault));
    gs_asset* a = nullptr;
    GS_TRY(bake_impl(r, formats, &a, alive, nullptr, nullptr, ev));
    (void)gs_asset_destroy(a);
    for (int k = 0; k < 4; ++k) GS_HIP(hipEventElapsedTime(&ms[k], ev[k == 0 ? 0 : k + 1], ev[k == 0 ? 1 : k + 2]));
    return GS_OK;
}

// The same for a Cluster* SH target, for scripts/bake_cluster_timing.py: ms[0] = the SH rows (+ the gathers of the seeds and the subset),
// ms[1 + 2 p] / ms[2 + 2 p] = the assignment / the mean update (sort included) of Lloyd pass p = 0..3, ms[9] = the final assignment, ms[10] = the
// table + the encode, ms[11] = everything before the SH rows.
__attribute__((visibility("default"))) int32_t gs_bake_cluster_stage_times_for_scripts(gs_renderer* r, const gs_import_formats* formats, float ms[12], uint32_t* alive) {
    if (!r || !formats || !ms || !alive) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (formats->sh_format <= GS_SH_NORM6 || formats->sh_format > 8u) return fail(GS_ERR_INVALID_ARGUMENT, "not a Cluster* SH target");
    GS_HIP(hipSetDevice(r->ctx->device));
    Event ev[6], cevOwned[12];
    hipEvent_t cev[12];
    for (Event& e : ev) GS_HIP(e.create(hipEventDefault));
    for (int k = 0; k < 12; ++k) { GS_HIP(cevOwned[k].create(hipEventDefault)); cev[k] = cevOwned[k]; }
    gs_asset* a = nullptr;
    GS_TRY(bake_impl(r, formats, &a, alive, nullptr, nullptr, ev, cev));
    (void)gs_asset_destroy(a);
    for (int k = 0; k < 11; ++k) GS_HIP(hipEventElapsedTime(&ms[k], cev[k], cev[k + 1]));
    GS_HIP(hipEventElapsedTime(&ms[11], ev[0], cev[0]));
    return GS_OK;
}

// The same for scripts/import_gpu_timing.py: one whole gs_import_encode_to_asset whose asset is destroyed again; ms[0..4] = GPU milliseconds of the
// upload (memory_kind 0; else next to nothing), the bounds, the Morton codes + the two sorts, the palette (SH rows + the Lloyd loop; 0 without a
// Cluster* target), the encode (+ the SH table).
__attribute__((visibility("default"))) int32_t gs_import_gpu_stage_times_for_scripts(gs_context* ctx, const gs_import_input* in, uint32_t memory_kind,
                                                                                     const gs_import_formats* formats, float ms[5]) {
    if (!ctx || !in || !formats || !ms) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    GS_HIP(hipSetDevice(ctx->device));
    Event ev[6], cevOwned[12];
    hipEvent_t cev[12];
    for (Event& e : ev) GS_HIP(e.create(hipEventDefault));
    for (int k = 0; k < 12; ++k) { GS_HIP(cevOwned[k].create(hipEventDefault)); cev[k] = cevOwned[k]; }
    gs_asset* a = nullptr;
    GS_TRY(import_impl(ctx, in, memory_kind, formats, &a, nullptr, nullptr, ev, cev));
    (void)gs_asset_destroy(a);
    return import_stage_times(formats, ev, cev, ms);
}

// The same for scripts/import_file_timing.py: one whole gs_import_file_to_asset whose asset is destroyed again; ms[0] is then the upload of the file's
// bytes, for a PLY with the reads of the file it overlaps.
__attribute__((visibility("default"))) int32_t gs_import_file_stage_times_for_scripts(gs_context* ctx, gs_splat_file* file, const gs_import_formats* formats,
                                                                                      uint32_t slice_bytes, float ms[5]) {
    if (!ctx || !file || !formats || !ms) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    GS_HIP(hipSetDevice(ctx->device));
    Event ev[6], cevOwned[12];
    hipEvent_t cev[12];
    for (Event& e : ev) GS_HIP(e.create(hipEventDefault));
    for (int k = 0; k < 12; ++k) { GS_HIP(cevOwned[k].create(hipEventDefault)); cev[k] = cevOwned[k]; }
    gs_asset* a = nullptr;
    GS_TRY(import_file_impl(ctx, file, formats, slice_bytes, &a, nullptr, nullptr, ev, cev));
    (void)gs_asset_destroy(a);
    return import_stage_times(formats, ev, cev, ms);
}

} // extern "C"
