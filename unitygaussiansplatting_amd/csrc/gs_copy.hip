// gs_copy.hip -- the merge path: CSCopySplats (SplatUtilities.compute:675-758), GaussianSplatRenderer.EditSetSplatCount / EditCopySplatsInto /
// EditCopySplats (GaussianSplatRenderer.cs:960-1075) as gs_renderer_edit_set_splat_count / gs_renderer_edit_copy_splats_into, and the readback
// of the four blobs (gs_renderer_edit_download_splat_data).  The editor's MergeSplatObjects (GaussianSplatRendererEditor.cs:213-235) is host code
// over the two (renderer.py).
//
// The kernel decodes a source splat of ANY format (gsm::LoadSplatDataFull), applies the copy transform -- the bake of the export, one shared
// function -- and writes one record in the reference's fixed VeryHigh layout: pos 12 B, other 16 B = { Norm10 rotation word, fp32 scale }, the
// colour texel at SplatIndexToPixelIndex(dstIdx) as four fp32, 45 fp32 SH coefficients in a 192-byte record.  The per-splat arithmetic is
// gsm::CopySplat (gs_device_math.h).  Two things of the reference's text are kept literally:
//   - the kernel bounds-checks srcIdx = srcStart + idx and reads the DELETED BIT of srcIdx, but loads the splat idx (LoadSplatData(idx), :697).
//     Both callers of the reference pass srcStart = 0, where the two agree;
//   - there is no IsSplatCut test: cut splats are copied like any other.
// A deleted source bit is OR-ed into the destination's word and never cleared; a source without a deleted buffer reads as zeros.
//
// Shape: one thread per copied splat, 256-thread workgroups; the loaded index is idx, so the chunk header is workgroup-uniform (chunk
// blockIdx.x).  One plain launch per call, no workgroup waits on another.  The lanes that copy are a prefix of every wave (all three bounds are
// monotone in idx), and a wave's destination records are contiguous in pos, other and sh:
//   pos / other   stored per lane: one dwordx3 / dwordx4 per lane, and the 64 lanes of that ONE instruction cover 768 / 1024 contiguous bytes --
//                 already the fully coalesced shape, staging would add LDS traffic and change nothing at the memory side;
//   sh            192 bytes per lane: a lane storing its own record would scatter every store instruction over 12 KB (the shape the export
//                 measured 31 % slower for 248-byte records).  So a wave stages its records in LDS -- 64 x 192 B = 12 KB
//                 per wave, 48 KB per workgroup: three workgroups = 12 waves per CU of 160 KB LDS, three waves per SIMD -- and writes the
//                 coefficients of its contiguous, 64-byte aligned range with dwordx4 stores: 11 per record (44 floats), lanes striding over the
//                 wave's records so that one instruction covers 64 consecutive dwordx4s but for the gap of each record's last 16 bytes.  Those
//                 hold the 45th float -- one dword store per lane -- and the 12 pad bytes, which are NOT written, as in the reference;
//   colour        Morton-scattered 16-byte texels: one dwordx4 per lane;
//   deleted bits  dstStart need not be a multiple of 32, so two waves (and two workgroups) can share a destination word: atomicOr from the
//                 lanes whose source bit is set, and only those.
#include <new>

#include "gs_common.h"

namespace gs {

constexpr uint32_t kCopySHFloats = 48;                             // a 192-byte SH record
constexpr uint32_t kCopySHQuads = 11;                              // whole dwordx4s of coefficients in it (44 floats; the 45th goes out alone)

struct CopyDst { uint8_t* pos; uint8_t* other; uint8_t* color; uint8_t* sh; uint32_t* deleted; uint32_t n; };

__global__ __launch_bounds__(256) void copy_splats_kernel(gsm::AssetView a, const uint32_t* __restrict__ srcDeleted, gsm::CopyXform X, CopyDst d,
                                                          uint32_t srcStart, uint32_t dstStart, uint32_t count) {
    __shared__ __attribute__((aligned(16))) float s_sh[4][64 * kCopySHFloats];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // the reference's early exits, in its order (the host clamps count, so that neither sum wraps)
    bool mine = idx < count;
    const uint32_t srcIdx = srcStart + idx, dstIdx = dstStart + idx;
    if (srcIdx >= a.n || dstIdx >= d.n) mine = false;
    gsm::CopyRec rec;
    if (mine) {
        gsm::CopySplat(a, X, idx, blockIdx.x, rec);                // LoadSplatData(idx): the literal index
        float* s = s_sh[wave] + lane * kCopySHFloats;
#pragma unroll
        for (int k = 0; k < 15; ++k) { s[3 * k] = rec.sh[k].x; s[3 * k + 1] = rec.sh[k].y; s[3 * k + 2] = rec.sh[k].z; }
    }
    __syncthreads();
    const uint32_t waveCount = (uint32_t)__popcll(__ballot(mine)); // the copying lanes are lanes 0 .. waveCount - 1
    if (waveCount != 0u) {
        const uint32_t waveDst = dstStart + (blockIdx.x * 256u + wave * 64u);      // the wave's first destination record
        float4* dst = (float4*)(d.sh + (size_t)waveDst * 192u);
        const float4* src = (const float4*)s_sh[wave];
        for (uint32_t i = lane; i < waveCount * kCopySHQuads; i += 64u) {
            const uint32_t r = i / kCopySHQuads, q = i - r * kCopySHQuads;
            dst[r * (kCopySHFloats / 4) + q] = src[r * (kCopySHFloats / 4) + q];
        }
    }
    if (!mine) return;
    *(float*)(d.sh + (size_t)dstIdx * 192u + 176u) = rec.sh[14].z;
    float* dp = (float*)(d.pos + (size_t)dstIdx * 12u);
    dp[0] = rec.pos.x; dp[1] = rec.pos.y; dp[2] = rec.pos.z;
    *(uint4*)(d.other + (size_t)dstIdx * 16u) = make_uint4(rec.rot, gsm::f2u(rec.scale.x), gsm::f2u(rec.scale.y), gsm::f2u(rec.scale.z));
    uint32_t px, py;
    gsm::SplatIndexToPixelIndex(dstIdx, px, py);
    *(float4*)(d.color + ((size_t)py * 2048u + px) * 16u) = make_float4(rec.color.x, rec.color.y, rec.color.z, rec.color.w);
    if (srcDeleted && ((srcDeleted[srcIdx >> 5] >> (srcIdx & 31u)) & 1u)) atomicOr(d.deleted + (dstIdx >> 5), 1u << (dstIdx & 31u));
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// bytes of the four blobs of a VeryHigh, chunk-less renderer of n splats (the colour texture: 2048 x CalcTextureSize(n).h texels of 16 bytes)
static inline size_t copy_blob_bytes(int k, uint32_t n) {
    if (k == 2) return (size_t)2048 * ((((size_t)n + 2047) / 2048 + 15) / 16 * 16) * 16;
    return (size_t)n * (k == 0 ? 12u : (k == 1 ? 16u : 192u));
}

// The reference tests only chunkData != null (GaussianSplatRenderer.cs:967); with its importer that implies the VeryHigh preset, and the kernel's
// fixed strides assume it.  The C ABI accepts any chunk-less descriptor, so the gate states the formats.
static bool copy_dst_gate(const gs_renderer* r) {
    const gsm::AssetView& a = r->asset->view;
    return a.chunkCount == 0 && a.posFmt == 0 && a.scaleFmt == 0 && a.shFmt == 0 && a.colorFmt == 0;
}

// what the kernel writes of a renderer whose four blobs are private (a resize's new state, or after edit_make_private of all four)
static CopyDst copy_dst_of(gs_renderer* r) { return { r->priv[0], r->priv[1], r->priv[2], r->priv[3], r->deletedBits, r->n }; }

// count clamped so that srcStart + idx and dstStart + idx stay inside both renderers (what the kernel's two tests leave): 0 = nothing to launch
static uint32_t copy_clamp(uint32_t srcN, uint32_t dstN, uint32_t srcStart, uint32_t dstStart, uint32_t count) {
    if (srcStart >= srcN || dstStart >= dstN) return 0u;
    if (count > srcN - srcStart) count = srcN - srcStart;
    if (count > dstN - dstStart) count = dstN - dstStart;
    return count;
}

static int32_t copy_launch(hipStream_t st, const gsm::AssetView& a, const uint32_t* srcDeleted, const gsm::CopyXform& X, const CopyDst& d,
                           uint32_t srcStart, uint32_t dstStart, uint32_t count) {
    count = copy_clamp(a.n, d.n, srcStart, dstStart, count);
    if (count == 0u) return GS_OK;
    hipLaunchKernelGGL(copy_splats_kernel, dim3((count + 255u) / 256u), dim3(256), 0, st, a, srcDeleted, X, d, srcStart, dstStart, count);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

static int32_t zeroed(DevBuf<uint8_t>& b, size_t bytes, hipStream_t st) {          // padded like an owned upload of an asset
    GS_HIP(b.alloc(bytes + 16));
    GS_HIP(hipMemsetAsync(b, 0, bytes + 16, st));
    return GS_OK;
}

// The new state of a resize: a renderer of newN splats made the way gs_renderer_create makes one (identity order, zeroed view buffer, an empty
// visible-sort history ...), with the four zero-filled private blobs, a zeroed deleted buffer, zeroed selection buffers and r's settings.
static int32_t resize_build(gs_renderer* r, uint32_t newN, gs_renderer* f) {
    hipStream_t st = r->ctx->stream;
    for (int k = 0; k < 4; ++k) {
        GS_TRY(zeroed(f->priv[k], copy_blob_bytes(k, newN), st));
        f->privBytes[k] = copy_blob_bytes(k, newN);
    }
    GS_TRY(ensure_deleted_bits(f, st));
    GS_TRY(edit_ensure(f));
    // settings: the plain values are one struct; what owns memory is applied again
    f->set = r->set;
    if (r->pairCapacity > f->pairCapacity) GS_TRY(gs_renderer_reserve_pairs(f, r->pairCapacity));
    if (r->cutoutCount) GS_TRY(gs_renderer_set_cutouts(f, (const gs_cutout*)r->cutoutsHost.get(), r->cutoutCount));
    if (r->profCapacity > 0) {
        GS_TRY(gs_renderer_set_profiling(f, r->profCapacity));
        if (!r->profiling) GS_TRY(gs_renderer_set_profiling(f, 0));
    }
    if (r->sortMode != f->sortMode) GS_TRY(gs_renderer_set_sort_mode(f, r->sortMode));
    return GS_OK;
}

static int32_t set_splat_count_impl(gs_renderer* r, uint32_t newN, const gs_copy_params* p) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    if (r->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane holds no edit state: edit its owner");
    if (newN == 0u || newN > kSortMaxCount) return fail(GS_ERR_INVALID_ARGUMENT, "set_splat_count: the count must be in [1, 2^30]");
    if (!copy_dst_gate(r)) return fail(GS_ERR_INVALID_ARGUMENT, "set_splat_count: only a chunk-less asset with fp32 pos / scale / sh and Float32x4 colour can be resized");
    if (newN == r->n) return GS_OK;
    GS_TRY(gs_context_synchronize(r->ctx));                        // the context's two streams and the lanes
    const int32_t lanes = r->lanes.empty() ? 1 : (int32_t)r->lanes.size();
    const gsm::CopyXform X = copy_xform_of(p);
    // everything new is allocated before anything old is released: on a failure the renderer is unchanged
    gs_renderer* f = nullptr;
    GS_TRY(renderer_create_n(r->ctx, r->asset, newN, &f));
    int32_t rc = resize_build(r, newN, f);
    if (rc == GS_OK) {
        // copy existing data over into the new buffers (EditCopySplats(transform, ..., newSplatCount, 0, 0, m_SplatCount), :1004); shrinking
        // truncates through the kernel's dstIdx >= dstN test
        rc = copy_launch(r->ctx->stream, asset_view(r), r->deletedBits, X, copy_dst_of(f), 0u, 0u, r->n);
    }
    if (rc == GS_OK && hipStreamSynchronize(r->ctx->stream) != hipSuccess) rc = fail(GS_ERR_HIP, "set_splat_count: the copy failed");
    if (rc != GS_OK) { (void)gs_renderer_destroy(f); return rc; }
    // use the new buffers and the new count: r becomes f (every per-N buffer and every flag derived from one), f leaves with the old state
    // the lanes were made for the old N.  (Everything is synchronised, so dropping them only frees; should it fail all the same, the new state goes.)
    rc = gs_renderer_set_frames_in_flight(r, 1);
    if (rc != GS_OK) { (void)gs_renderer_destroy(f); return rc; }
    std::swap(*r, *f);
    hist_carry(r, f);                                              // the edit history's entries go with the old state; its switch, budget and counters stay
    (void)gs_renderer_destroy(f);
    if (lanes > 1) GS_TRY(gs_renderer_set_frames_in_flight(r, lanes));
    return GS_OK;
}

static int32_t copy_splats_into_impl(gs_renderer* src, gs_renderer* dst, const gs_copy_params* p, uint32_t srcStart, uint32_t dstStart, uint32_t count) {
    if (!src || !dst) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    if (src == dst) return fail(GS_ERR_INVALID_ARGUMENT, "copy_splats_into: source and destination are the same renderer");
    if (src->laneOf || dst->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane holds no edit state: edit its owner");
    if (src->ctx->device != dst->ctx->device) return fail(GS_ERR_INVALID_ARGUMENT, "copy_splats_into: source and destination live on different GPUs");
    if (!copy_dst_gate(dst)) return fail(GS_ERR_INVALID_ARGUMENT, "copy_splats_into: the destination must be chunk-less with fp32 pos / scale / sh and Float32x4 colour");
    if (copy_clamp(src->n, dst->n, srcStart, dstStart, count) == 0u) return GS_OK;
    GS_HIP(hipSetDevice(dst->ctx->device));
    hist_forget(dst);                                              // the copy writes index ranges, not the selection: nothing of it is journalled
    const gsm::CopyXform X = copy_xform_of(p);
    hipStream_t st = dst->ctx->stream;
    GS_TRY(edit_before_move(dst));                                 // positions change: the transform's ordering (gs_edit.hip)
    for (int k = 0; k < 4; ++k) GS_TRY(edit_make_private(dst, k));
    if (src->deletedBits) GS_TRY(ensure_deleted_bits(dst, st));    // a destination without a deleted buffer gets a zeroed one
    const bool cross = src->ctx != dst->ctx;
    if (cross) GS_TRY(signal_to(src->ctx, st));                    // the source's pending edits are visible to the kernel
    GS_TRY(copy_launch(st, asset_view(src), src->deletedBits, X, copy_dst_of(dst), srcStart, dstStart, count));
    if (cross) GS_TRY(signal_to(dst->ctx, src->ctx->stream));      // a later transform of the source does not race the read
    GS_TRY(edit_after_move(dst));
    if (src->deletedBits) GS_TRY(edit_deleted_to_lanes(dst));
    return GS_OK;
}

} // namespace gs

using namespace gs;

extern "C" {

int32_t gs_renderer_splat_count(const gs_renderer* r, uint32_t* out) {
    if (!r || !out) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    *out = r->n;
    return GS_OK;
}

int32_t gs_renderer_edit_set_splat_count(gs_renderer* r, uint32_t new_count, const gs_copy_params* p) {
    try {
        return set_splat_count_impl(r, new_count, p);
    } catch (const std::bad_alloc&) {                              // (the lanes' vectors) must not unwind across the C ABI
        return fail(GS_ERR_OUT_OF_MEMORY, "set_splat_count: out of host memory");
    }
}

int32_t gs_renderer_edit_copy_splats_into(gs_renderer* src, gs_renderer* dst, const gs_copy_params* p, uint32_t src_start, uint32_t dst_start, uint32_t count) {
    return copy_splats_into_impl(src, dst, p, src_start, dst_start, count);
}

int32_t gs_renderer_edit_download_splat_data(gs_renderer* r, void* pos, size_t pos_bytes, void* other, size_t other_bytes,
                                             void* color, size_t color_bytes, void* sh, size_t sh_bytes) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    void* const dst[4] = { pos, other, color, sh };
    const size_t bytes[4] = { pos_bytes, other_bytes, color_bytes, sh_bytes };
    for (int k = 0; k < 4; ++k)
        if (dst[k] && bytes[k] > blob_bytes(r, k)) return fail(GS_ERR_INVALID_ARGUMENT, "more bytes asked for than the blob holds");
    GS_HIP(hipSetDevice(r->ctx->device));
    for (int k = 0; k < 4; ++k)
        if (dst[k] && bytes[k]) GS_HIP(hipMemcpyAsync(dst[k], blob_ptr(r, k), bytes[k], hipMemcpyDeviceToHost, r->ctx->stream));
    GS_HIP(hipStreamSynchronize(r->ctx->stream));
    return GS_OK;
}

// A measurement aid of scripts/copy_timing.py, which binds it itself: not declared in gsplat_c.h, not part of the ABI.  One copy of all of src into dst
// at dst_start 0 on dst's stream between two events: *ms = GPU milliseconds of the kernel.
__attribute__((visibility("default"))) int32_t gs_copy_kernel_time_for_scripts(gs_renderer* src, gs_renderer* dst, float* ms) {
    if (!src || !dst || !ms || src == dst || src->ctx != dst->ctx || !copy_dst_gate(dst)) return fail(GS_ERR_INVALID_ARGUMENT, "bad argument");
    GS_HIP(hipSetDevice(dst->ctx->device));
    for (int k = 0; k < 4; ++k) GS_TRY(edit_make_private(dst, k));
    const gsm::CopyXform X = copy_xform_of(nullptr);
    Event ev[2];
    for (Event& e : ev) GS_HIP(e.create(hipEventDefault));
    hipStream_t st = dst->ctx->stream;
    const CopyDst d = copy_dst_of(dst);
    hipError_t he = hipEventRecord(ev[0], st);
    const int32_t rc = copy_launch(st, asset_view(src), nullptr, X, d, 0u, 0u, src->n);
    if (he == hipSuccess) he = hipEventRecord(ev[1], st);
    const hipError_t hs = hipStreamSynchronize(st);
    GS_TRY(rc);
    GS_HIP(he);
    GS_HIP(hs);
    GS_HIP(hipEventElapsedTime(ms, ev[0], ev[1]));
    return GS_OK;
}

} // extern "C"
