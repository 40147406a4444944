// gs_export.hip -- exporting the edited splats: CSExportData (SplatUtilities.compute:523-673), GaussianSplatRenderer.EditExportData
// (GaussianSplatRenderer.cs:936-958) and the editor's ExportPlyFile (GaussianSplatRendererEditor.cs:394-445) as the gs_renderer_edit_export_* entry points.
//
// CSExportData only READS the asset, the cutouts and the transform and writes a buffer of its own, so it fits the immutable, shared asset of this
// library.  The per-splat arithmetic is gsm::ExportSplat (gs_device_math.h): the full LoadSplatData decode, the optional baked transform, and the
// 62-float record (ExportSplatData = InputSplatData = the PLY vertex), word for word what the reference leaves in memory for the member of HLSL's
// log / sqrt families the project fixes (LogDetFull, the band matrices' recurrence).
//
// Three plain launches, none waits on another workgroup (an offline path on shared machines: no look-back, no spinning):
//   alive_count     (enqueue_alive_counts, gs_compact.hip) per 256-splat chunk, the number of splats that are alive (idx < N, not deleted, not cut):
//                   popcounts of ballots.  Reads positions, the deleted words and the cutouts only.
//   export_scan     (the same call) exclusive prefix over the chunk counts, one workgroup looping over the array 1024 counts at a time;
//                   base[chunks] = the total.
//   export_records  one 256-thread workgroup per chunk (so the chunk header is workgroup-uniform) of a range of whole chunks.  Reference-shaped mode
//                   (base == null) writes all N records at index idx, nor = 1 for a cut splat; compacted mode writes the alive records only, in index
//                   order, at base[chunk] + rank inside the chunk.
// The stores are the hot part: 248 bytes per record (8-byte aligned, never 16).  A lane that stored its own record would scatter the 64 lanes of every
// store instruction over 15.5 KB.  So a wave STAGES its records in LDS (slot = rank inside the wave) and then writes its contiguous byte range -- in
// either mode a wave's records are contiguous in the output -- with dwordx2 stores, 512 contiguous bytes per instruction.  Staging is per wave, 64 x 248
// = 15.5 KB each, 62 KB per workgroup: two workgroups = 8 waves per CU (160 KB LDS), two waves per SIMD.  Per-workgroup staging would need the same 62 KB
// (256 records) for the same occupancy and add a workgroup-wide dependence between the four waves' ranges, so per-wave it is; a streaming kernel whose
// every wave keeps 31 x 512-byte stores in flight does not need more waves to cover the write latency.  -DGS_EXPORT_DIRECT builds the variant in which
// every lane stores its own record (scripts/export_timing.py times one against the other).
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <new>
#include <string>

#include "gs_common.h"
#include "gs_block.h"

namespace gs {

constexpr uint32_t kRecFloats = GS_EXPORT_RECORD_BYTES / 4;       // 62
constexpr uint32_t kExportBatchDefault = 131072;                  // splats per batch: 31 MB of records in the device buffer and in each pinned buffer
static_assert(kRecFloats * 4 == GS_EXPORT_RECORD_BYTES && kRecFloats % 2 == 0, "records are whole dwordx2s");

// out: the records of the chunks [firstChunk, firstChunk + gridDim.x).  base == null: record idx - firstChunk * 256 for every idx < N; else record
// base[chunk] - base[firstChunk] + rank for the alive ones.
__global__ __launch_bounds__(256) void export_records_kernel(gsm::AssetView a, gsm::EditView e, gsm::ExportXform X, const uint32_t* __restrict__ base,
                                                             uint32_t firstChunk, float* __restrict__ out) {
    const uint32_t ci = firstChunk + blockIdx.x, idx = ci * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __shared__ uint32_t s_cnt[4];
    gsm::V3 pos; bool cut;
    const bool alive = export_alive(a, e, idx, ci, pos, cut);
    const bool mine = base ? alive : (idx < a.n);                  // does this lane write a record?
    const uint32_t slot = block_rank(mine, lane, wave, s_cnt);    // rank inside the wave (reference-shaped: the lane itself, the tail is at the end)
    float rec[kRecFloats];
    if (mine) gsm::ExportSplat(a, X, idx, ci, pos, base ? false : cut, rec);
#ifndef GS_EXPORT_DIRECT
    __shared__ __attribute__((aligned(16))) float s_rec[4][64 * kRecFloats];
    if (mine) {
#pragma unroll
        for (uint32_t k = 0; k < kRecFloats; ++k) s_rec[wave][slot * kRecFloats + k] = rec[k];
    }
#endif
    __syncthreads();
    const uint32_t first = block_first(s_cnt, wave, base ? (base[ci] - base[firstChunk]) : blockIdx.x * 256u);      // first record of the workgroup, then of the wave
#ifndef GS_EXPORT_DIRECT
    const uint32_t waveCount = s_cnt[wave];
    // the wave's records are contiguous: waveCount * 31 dwordx2s from an 8-byte aligned address
    float2* dst = (float2*)(out + (size_t)first * kRecFloats);
    const float2* src = (const float2*)s_rec[wave];
    for (uint32_t i = lane; i < waveCount * (kRecFloats / 2); i += 64u) dst[i] = src[i];
#else
    if (mine) {
        float* dst = out + ((size_t)first + slot) * kRecFloats;
#pragma unroll
        for (uint32_t k = 0; k < kRecFloats; ++k) dst[k] = rec[k];
    }
#endif
}

static uint32_t export_batch_chunks() {
    unsigned long long b = kExportBatchDefault;
    if (const char* e = getenv("GSPLAT_EXPORT_BATCH")) {           // read per call
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (end != e && v > 0) b = v;
    }
    if (b > (1ull << 30)) b = 1ull << 30;
    return (uint32_t)((b + 255) / 256);
}

// One export: the count + scan (compacted mode), then export_records over batches of whole chunks into one fixed device buffer, each batch copied into one
// of two pinned buffers that alternate with the host's consumption of the other (sink: a memcpy into the caller's array, or fwrite).
struct ExportRun {
    gs_renderer* r;
    gsm::ExportXform X;
    bool compact;
    uint32_t chunks = 0;
    DevBuf<uint32_t> counts, base;
    std::vector<uint32_t> hostBase;                               // chunks + 1 words (compacted mode)

    int32_t prepare() {                                            // the alive count and every chunk's first record
        hipStream_t st = r->ctx->stream;
        chunks = (r->n + 255u) / 256u;
        if (!compact || chunks == 0u) { hostBase.assign(1, 0u); return GS_OK; }
        hostBase.resize((size_t)chunks + 1);                       // (may throw: before anything is in flight)
        GS_HIP(counts.alloc((size_t)chunks * 4));
        GS_HIP(base.alloc(((size_t)chunks + 1) * 4));
        GS_TRY(enqueue_alive_counts(st, asset_view(r), edit_view(r), false, chunks, counts.get(), base.get()));
        GS_HIP(hipMemcpyAsync(hostBase.data(), base.get(), hostBase.size() * 4, hipMemcpyDeviceToHost, st));
        GS_HIP(hipStreamSynchronize(st));
        return GS_OK;
    }
    uint32_t total() const { return compact ? hostBase[chunks] : r->n; }
    // records of the chunks [c0, c1)
    uint32_t records(uint32_t c0, uint32_t c1) const {
        if (compact) return hostBase[c1] - hostBase[c0];
        const uint64_t hi = (uint64_t)c1 * 256u;
        return (uint32_t)((hi < r->n ? hi : r->n) - (uint64_t)c0 * 256u);
    }
    void launch(uint32_t c0, uint32_t c1, float* out) const {
        hipLaunchKernelGGL(export_records_kernel, dim3(c1 - c0), dim3(256), 0, r->ctx->stream, asset_view(r), edit_view(r), X,
                           compact ? (const uint32_t*)base.get() : (const uint32_t*)nullptr, c0, out);
    }
    // sink(data, bytes) != 0 stops the run with GS_ERR_INVALID_ARGUMENT (its own detail set)
    template <class Sink> int32_t to_host(Sink&& sink) {
        hipStream_t st = r->ctx->stream;
        if (total() == 0u) return GS_OK;
        const uint32_t per = export_batch_chunks() < chunks ? export_batch_chunks() : chunks;
        const size_t bufBytes = (size_t)per * 256 * GS_EXPORT_RECORD_BYTES;
        DevBuf<float> dev;
        PinnedBuf<uint8_t> pin[2];
        Event ev[2];
        GS_HIP(dev.alloc(bufBytes));
        for (int k = 0; k < 2; ++k) {
            GS_HIP(pin[k].alloc(bufBytes, hipHostMallocDefault));
            GS_HIP(ev[k].create(hipEventDisableTiming));
        }
        int32_t rc = GS_OK;
        size_t pendingBytes = 0;
        int pending = -1, cur = 0;
        for (uint32_t c0 = 0; c0 < chunks && rc == GS_OK; c0 += per) {
            const uint32_t c1 = c0 + per < chunks ? c0 + per : chunks;
            const size_t bytes = (size_t)records(c0, c1) * GS_EXPORT_RECORD_BYTES;
            if (bytes) {                                           // (a batch with nothing alive has no output: no launch)
                launch(c0, c1, dev.get());
                hipError_t he = hipGetLastError();
                if (he == hipSuccess) he = hipMemcpyAsync(pin[cur].get(), dev.get(), bytes, hipMemcpyDeviceToHost, st);
                if (he == hipSuccess) he = hipEventRecord(ev[cur], st);
                if (he != hipSuccess) { rc = fail_hip(he, "export batch", __FILE__, __LINE__); break; }
            }
            if (pending >= 0) {                                    // the batch before this one: consumed while this one runs
                const hipError_t he = hipEventSynchronize(ev[pending]);
                if (he != hipSuccess) { rc = fail_hip(he, "hipEventSynchronize", __FILE__, __LINE__); break; }
                if (sink(pin[pending].get(), pendingBytes) != 0) { rc = GS_ERR_INVALID_ARGUMENT; break; }
                pending = -1;
            }
            if (bytes) { pending = cur; pendingBytes = bytes; cur ^= 1; }
        }
        if (rc == GS_OK && pending >= 0) {
            const hipError_t he = hipEventSynchronize(ev[pending]);
            if (he != hipSuccess) rc = fail_hip(he, "hipEventSynchronize", __FILE__, __LINE__);
            else if (sink(pin[pending].get(), pendingBytes) != 0) rc = GS_ERR_INVALID_ARGUMENT;
        }
        (void)hipStreamSynchronize(st);                            // nothing in flight may outlive the buffers
        return rc;
    }
};

static int32_t export_begin(gs_renderer* r, const gs_export_params* p, bool compact, ExportRun& run) {
    if (!r || !p) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    GS_HIP(hipSetDevice(r->ctx->device));
    run.r = r; run.compact = compact;
    run.X = export_xform_of(*p);
    return run.prepare();
}

// ---- SPZ: the alive splats as the six byte columns of an SPZ version 2 stream ----------------------------------------
// After enqueue_alive_counts, the alive list the bake uses too (enqueue_alive_list, gs_compact.hip: alive[j] = source index of the j-th alive splat) with its
// bounds taken of the positions AS EXPORTED (through the matrix when the transform is baked: the automatic fract_bits follows from them; the host
// derives it from the six floats), then one plain launch that waits on no other workgroup:
//   export_spz         256 threads per 256 destination ranks: lane j decodes alive[256 b + j] (LoadSplatDataFull + the ExportSplat body) and packs.
// Each column has a 16-byte aligned region of its own in one transient buffer, padded past its end.  The 64 ranks of a wave own 64 x {9, 1, 3, 3,
// 3, 3k} bytes of each column -- every one a multiple of 4 at a multiple-of-4 offset -- so a wave stages its bytes in LDS (64 x 64 B = 4 KB, 16 KB per
// workgroup: occupancy is not LDS-bound) and writes each column's range with contiguous dword stores.  No two waves store to the same dword: only
// the last wave with any rank below n rounds its byte count up, into the region's padding, and the lanes of ranks >= n stage zeros there.  Those
// lanes read neither alive[] nor the asset, and every lane of the workgroup reaches the barrier.
struct SpzColumns { uint8_t* col[gsm::kSpzColumns]; };

__global__ __launch_bounds__(256) void export_spz_kernel(gsm::AssetView a, gsm::ExportXform X, const uint32_t* __restrict__ alive, uint32_t n, uint32_t fractBits,
                                                         uint32_t shCoeffs, SpzColumns out) {
    // per wave: positions 576, alpha 64, colour / scale / rotation 192 each, SH 2880 bytes -- 4096, each part at a multiple of 4
    constexpr uint32_t kAt[gsm::kSpzColumns] = { 0u, 576u, 640u, 832u, 1024u, 1216u };
    __shared__ __attribute__((aligned(16))) uint8_t s_col[4][4096];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t waveFirst = blockIdx.x * 256u + wave * 64u, rank = waveFirst + lane;
    uint8_t* s = s_col[wave];
    const uint32_t shWidth = 3u * shCoeffs;
    if (rank < n) {
        const uint32_t src = alive[rank], ci = src >> 8;
        float rec[kRecFloats], opacity;
        gsm::ExportSplatLinear(a, X, src, ci, gsm::LoadSplatPosChunk(a, src, ci), false, rec, opacity);
        gsm::SpzPackSplat(rec, opacity, fractBits, shCoeffs, s + kAt[0] + lane * 9u, s + kAt[1] + lane, s + kAt[2] + lane * 3u, s + kAt[3] + lane * 3u,
                          s + kAt[4] + lane * 3u, s + kAt[5] + lane * shWidth);
    } else {                                                       // what the last wave's rounding up carries into the padding
        for (uint32_t k = 0; k < 9u; ++k) s[kAt[0] + lane * 9u + k] = 0u;
        s[kAt[1] + lane] = 0u;
        for (uint32_t k = 0; k < 3u; ++k) { s[kAt[2] + lane * 3u + k] = 0u; s[kAt[3] + lane * 3u + k] = 0u; s[kAt[4] + lane * 3u + k] = 0u; }
        for (uint32_t k = 0; k < shWidth; ++k) s[kAt[5] + lane * shWidth + k] = 0u;
    }
    __syncthreads();
    if (waveFirst >= n) return;                                    // (after the barrier: a wave without a rank writes nothing)
    const uint32_t count = n - waveFirst < 64u ? n - waveFirst : 64u;
#pragma unroll
    for (uint32_t c = 0; c < gsm::kSpzColumns; ++c) {
        const uint32_t w = gsm::SpzColumnWidth(c, shCoeffs);
        const uint32_t dwords = (count * w + 3u) / 4u;             // <= 16 w: inside the wave's 64 w staged bytes, and inside the region's padding
        uint32_t* dst = (uint32_t*)(out.col[c] + (size_t)waveFirst * w);
        const uint32_t* from = (const uint32_t*)(s + kAt[c]);
        for (uint32_t i = lane; i < dwords; i += 64u) dst[i] = from[i];
    }
}

// bytes of column c's region in the transient buffer: n x width, a dword of padding, rounded up to 16
static size_t spz_region_bytes(uint32_t n, uint32_t width) { return (((size_t)n * width + 4u) + 15u) / 16u * 16u; }

// One SPZ export: the alive list and the bounds, fract_bits, the pack, then the columns to the host slice by slice.  ev: null, or six events
// (scripts/export_spz_timing.py): before / after the count + scan, the alive list + bounds, the pack
struct SpzRun {
    gs_renderer* r = nullptr;
    gsm::ExportXform X;
    gs_spz_params s;
    uint32_t chunks = 0, total = 0, fract = 0, shCoeffs = 0;
    DevBuf<uint32_t> counts, base, alive;
    DevBuf<float> partial, bounds;
    DevBuf<uint8_t> cols;
    size_t off[gsm::kSpzColumns] = {}, bytes[gsm::kSpzColumns] = {};

    uint64_t body_bytes() const { return spz_body_bytes(total, s.sh_level); }

    int32_t prepare(Event* ev = nullptr) {
        hipStream_t st = r->ctx->stream;
        shCoeffs = gsm::SpzShCoeffs(s.sh_level);
        chunks = (r->n + 255u) / 256u;
        if (chunks == 0u) return fail(GS_ERR_INVALID_ARGUMENT, spz_alive_refusal(0));
        GS_HIP(counts.alloc((size_t)chunks * 4));
        GS_HIP(base.alloc(((size_t)chunks + 1) * 4));
        if (ev) GS_HIP(hipEventRecord(ev[0], st));
        GS_TRY(enqueue_alive_counts(st, asset_view(r), edit_view(r), false, chunks, counts.get(), base.get()));
        if (ev) GS_HIP(hipEventRecord(ev[1], st));
        GS_TRY(drain(st, [&]() -> int32_t { GS_HIP(hipMemcpyAsync(&total, base.get() + chunks, 4, hipMemcpyDeviceToHost, st)); return GS_OK; }(), "export: the alive count"));
        if (const char* why = spz_alive_refusal(total)) return fail(GS_ERR_INVALID_ARGUMENT, why);
        GS_HIP(alive.alloc(((size_t)total + 16) * 4));
        GS_HIP(partial.alloc((size_t)chunks * 6 * 4));
        GS_HIP(bounds.alloc(6 * 4));
        AliveXform B;
        B.through = X.bake;
        memcpy(B.m, X.o2w, sizeof(B.m));
        float hostBounds[6] = { 0, 0, 0, 0, 0, 0 };
        if (ev) GS_HIP(hipEventRecord(ev[2], st));
        GS_TRY(drain(st, [&]() -> int32_t {
            GS_TRY(enqueue_alive_list(st, asset_view(r), edit_view(r), false, false, B, chunks, base.get(), alive.get(), partial.get(), bounds.get()));
            if (ev) GS_HIP(hipEventRecord(ev[3], st));
            GS_HIP(hipMemcpyAsync(hostBounds, bounds.get(), sizeof(hostBounds), hipMemcpyDeviceToHost, st));
            return GS_OK;
        }(), "export: the alive list"));
        fract = s.fract_bits == GS_SPZ_FRACT_AUTO ? gsm::SpzAutoFractBits(hostBounds) : s.fract_bits;
        return GS_OK;
    }

    // the six columns into the transient buffer; the caller drains the stream (stream() does) before `cols` goes away
    int32_t pack(Event* ev = nullptr) {
        hipStream_t st = r->ctx->stream;
        size_t at = 0;
        for (uint32_t c = 0; c < gsm::kSpzColumns; ++c) {
            const uint32_t w = gsm::SpzColumnWidth(c, shCoeffs);
            off[c] = at; bytes[c] = (size_t)total * w;
            at += spz_region_bytes(total, w);
        }
        GS_HIP(cols.alloc(at));
        SpzColumns out;
        for (uint32_t c = 0; c < gsm::kSpzColumns; ++c) out.col[c] = cols.get() + off[c];
        if (ev) GS_HIP(hipEventRecord(ev[4], st));
        hipLaunchKernelGGL(export_spz_kernel, dim3((total + 255u) / 256u), dim3(256), 0, st, asset_view(r), X, (const uint32_t*)alive.get(), total, fract, shCoeffs, out);
        GS_HIP(hipGetLastError());
        if (ev) GS_HIP(hipEventRecord(ev[5], st));
        return GS_OK;
    }

    // header, then column by column through two pinned slices that fill alternately: the next slice's copy is in flight while the sink has this one.
    // sink(data, bytes) != 0 stops the run with GS_ERR_INVALID_ARGUMENT (its own detail set).  The host never holds the body.
    template <class Sink> int32_t stream(Sink&& sink) {
        hipStream_t st = r->ctx->stream;
        int32_t rc = pack();
        size_t slice = s.slice_bytes ? (size_t)s.slice_bytes : (size_t)kSpzSliceDefault, largest = 0;
        for (size_t b : bytes) largest = b > largest ? b : largest;
        const size_t whole = (largest + kSpzSliceMin - 1) / kSpzSliceMin * kSpzSliceMin;      // no slice larger than a column needs
        if (slice > whole) slice = whole;
        PinnedBuf<uint8_t> pin[2];
        Event ev[2];
        for (int k = 0; k < 2 && rc == GS_OK; ++k) {
            hipError_t he = pin[k].alloc(slice, hipHostMallocDefault);
            if (he == hipSuccess) he = ev[k].create(hipEventDisableTiming);
            if (he != hipSuccess) rc = fail_hip(he, "export: pinned slice", __FILE__, __LINE__);
        }
        if (rc == GS_OK) {
            uint32_t head[4];
            gsm::SpzHeaderWords(total, s.sh_level, fract, head);
            if (sink((const uint8_t*)head, sizeof(head)) != 0) rc = GS_ERR_INVALID_ARGUMENT;
        }
        int pending = -1, cur = 0;
        size_t pendingBytes = 0, at = 0;
        uint32_t c = 0;
        while (rc == GS_OK) {
            while (c < gsm::kSpzColumns && at >= bytes[c]) { ++c; at = 0; }
            const bool have = c < gsm::kSpzColumns;
            size_t len = 0;
            if (have) {
                len = bytes[c] - at < slice ? bytes[c] - at : slice;
                hipError_t he = hipMemcpyAsync(pin[cur].get(), cols.get() + off[c] + at, len, hipMemcpyDeviceToHost, st);
                if (he == hipSuccess) he = hipEventRecord(ev[cur], st);
                if (he != hipSuccess) { rc = fail_hip(he, "export slice", __FILE__, __LINE__); break; }
                at += len;
            }
            if (pending >= 0) {                                    // the slice before this one: consumed while this one's copy runs
                const hipError_t he = hipEventSynchronize(ev[pending]);
                if (he != hipSuccess) { rc = fail_hip(he, "hipEventSynchronize", __FILE__, __LINE__); break; }
                if (sink(pin[pending].get(), pendingBytes) != 0) { rc = GS_ERR_INVALID_ARGUMENT; break; }
                pending = -1;
            }
            if (!have) break;
            pending = cur; pendingBytes = len; cur ^= 1;
        }
        return drain(st, rc, "export");
    }
};

static int32_t spz_begin(gs_renderer* r, const gs_export_params* p, const gs_spz_params* s, SpzRun& run, Event* ev = nullptr) {
    if (!r || !p || !s) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (r->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane holds no edit state: export its owner");
    if (const char* why = spz_params_refusal(*s)) return fail(GS_ERR_INVALID_ARGUMENT, why);
    GS_HIP(hipSetDevice(r->ctx->device));
    run.r = r; run.s = *s;
    run.X = export_xform_of(*p);
    return run.prepare(ev);
}

// the gzip stream of a file being written: deflate with the gzip wrapper, the output through one fixed buffer
struct GzWriter {
    FILE* f = nullptr;
    z_stream z;
    bool live = false;
    uint8_t buf[1 << 16];
    ~GzWriter() { if (live) (void)deflateEnd(&z); }
    int begin(FILE* file, int level) {
        f = file;
        memset(&z, 0, sizeof(z));
        if (deflateInit2(&z, level, Z_DEFLATED, 16 + MAX_WBITS, 8, Z_DEFAULT_STRATEGY) != Z_OK) return 1;
        live = true;
        return 0;
    }
    // 0, 1 = deflate failed, 2 = fwrite failed (errno)
    int write(const uint8_t* data, size_t n, int flush) {
        z.next_in = (Bytef*)data; z.avail_in = (uInt)n;            // (a slice is at most 4 GiB - 1: slice_bytes is 32 bits)
        for (;;) {
            z.next_out = buf; z.avail_out = (uInt)sizeof(buf);
            const int rc = deflate(&z, flush);
            if (rc != Z_OK && rc != Z_STREAM_END && rc != Z_BUF_ERROR) return 1;
            const size_t have = sizeof(buf) - z.avail_out;
            if (have && fwrite(buf, 1, have, f) != have) return 2;
            if (flush == Z_FINISH ? rc == Z_STREAM_END : (z.avail_in == 0 && z.avail_out != 0)) return 0;
        }
    }
};

} // namespace gs

using namespace gs;

// std::bad_alloc (the host vector of chunk bases, the header string) must not unwind across the C ABI: GS_ERR_OUT_OF_MEMORY, as in gs_import.cpp
template <class F> static int32_t export_guarded(F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return gs::fail(GS_ERR_OUT_OF_MEMORY, "export: out of host memory");
    }
}

static int32_t export_data_impl(gs_renderer* r, const gs_export_params* p, void* out, size_t bytes, int32_t memory_kind) {
    if (!r || !p || !out) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (memory_kind != 0 && memory_kind != 1) return fail(GS_ERR_INVALID_ARGUMENT, "export: memory_kind must be 0 (host) or 1 (device)");
    if (bytes < GS_EXPORT_RECORD_BYTES || bytes < (size_t)r->n * GS_EXPORT_RECORD_BYTES) return fail(GS_ERR_INVALID_ARGUMENT, "export: the buffer is smaller than splat_count records");
    if (memory_kind == 1 && ((uintptr_t)out & 7u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "export: a device buffer must be 8-byte aligned");      // dwordx2 stores
    ExportRun run;
    GS_TRY(export_begin(r, p, false, run));
    if (run.chunks == 0u) return GS_OK;                            // no splats: nothing to launch
    if (memory_kind == 1) {
        run.launch(0, run.chunks, (float*)out);
        return drain(r->ctx->stream, [&]() -> int32_t { GS_HIP(hipGetLastError()); return GS_OK; }(), "export_data");
    }
    uint8_t* dst = (uint8_t*)out;
    return run.to_host([&](const uint8_t* data, size_t n) { memcpy(dst, data, n); dst += n; return 0; });
}

static int32_t export_alive_impl(gs_renderer* r, const gs_export_params* p, void* out, size_t capacity_records, uint32_t* alive) {
    if (!r || !p) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    ExportRun run;
    GS_TRY(export_begin(r, p, true, run));
    if (alive) *alive = run.total();
    if (!out) return GS_OK;
    if (capacity_records < run.total()) return fail(GS_ERR_INVALID_ARGUMENT, "export: the buffer is smaller than the alive records");
    uint8_t* dst = (uint8_t*)out;
    return run.to_host([&](const uint8_t* data, size_t n) { memcpy(dst, data, n); dst += n; return 0; });
}

static int32_t export_ply_impl(gs_renderer* r, const gs_export_params* p, const char* path, uint32_t* alive) {
    if (!r || !p || !path) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    ExportRun run;
    GS_TRY(export_begin(r, p, true, run));
    if (alive) *alive = run.total();
    // the header of ExportPlyFile (GaussianSplatRendererEditor.cs:428): LF line ends, the 62 float properties of InputSplatData
    std::string h = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(run.total()) + "\n";
    static const char* const kHead[] = { "x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2" };
    static const char* const kTail[] = { "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3" };
    for (const char* nm : kHead) h += std::string("property float ") + nm + "\n";
    for (int k = 0; k < 45; ++k) h += "property float f_rest_" + std::to_string(k) + "\n";
    for (const char* nm : kTail) h += std::string("property float ") + nm + "\n";
    h += "end_header\n";
    FILE* f = fopen(path, "wb");                                   // (after the last allocation that may throw: the file is never left open)
    if (!f) { set_error_detail("export: cannot create %s: %s", path, strerror(errno)); return GS_ERR_INVALID_ARGUMENT; }
    int32_t rc = GS_OK;
    if (fwrite(h.data(), 1, h.size(), f) != h.size()) { set_error_detail("export: writing %s failed: %s", path, strerror(errno)); rc = GS_ERR_INVALID_ARGUMENT; }
    if (rc == GS_OK)
        rc = run.to_host([&](const uint8_t* data, size_t n) {
            if (fwrite(data, 1, n, f) == n) return 0;
            set_error_detail("export: writing %s failed: %s", path, strerror(errno));
            return 1;
        });
    if (fclose(f) != 0 && rc == GS_OK) { set_error_detail("export: closing %s failed: %s", path, strerror(errno)); rc = GS_ERR_INVALID_ARGUMENT; }
    if (rc != GS_OK) remove(path);                                 // no partially written file is left behind
    return rc;
}

// The three kernels once over the whole asset, compacted mode, into device memory, timed by events between them
static int32_t export_kernel_times_impl(gs_renderer* r, const gs_export_params* p, void* device_out, size_t bytes, float ms[3], uint32_t* alive) {
    if (!r || !p || !device_out || !ms) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (((uintptr_t)device_out & 7u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "export: a device buffer must be 8-byte aligned");
    ExportRun run;
    GS_TRY(export_begin(r, p, true, run));                         // untimed: the alive count the buffer must hold
    if (alive) *alive = run.total();
    if (bytes < (size_t)run.total() * GS_EXPORT_RECORD_BYTES) return fail(GS_ERR_INVALID_ARGUMENT, "export: the buffer is smaller than the alive records");
    ms[0] = ms[1] = ms[2] = 0.0f;
    if (run.chunks == 0u) return GS_OK;
    hipStream_t st = r->ctx->stream;
    Event ev[4];
    for (Event& e : ev) GS_HIP(e.create(hipEventDefault));         // (nothing is in flight yet)
    GS_TRY(drain(st, [&]() -> int32_t {
        GS_HIP(hipEventRecord(ev[0], st));
        GS_TRY(enqueue_alive_chunk_counts(st, asset_view(r), edit_view(r), false, run.chunks, run.counts.get()));
        GS_HIP(hipEventRecord(ev[1], st));
        GS_TRY(enqueue_scan(st, run.counts.get(), run.base.get(), run.chunks));
        GS_HIP(hipEventRecord(ev[2], st));
        run.launch(0, run.chunks, (float*)device_out);
        GS_HIP(hipGetLastError());
        GS_HIP(hipEventRecord(ev[3], st));
        return GS_OK;
    }(), "export: kernel times"));
    for (int k = 0; k < 3; ++k) GS_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    return GS_OK;
}

static int32_t export_spz_body_impl(gs_renderer* r, const gs_export_params* p, const gs_spz_params* s, void* out, size_t capacity_bytes, uint64_t* body_bytes,
                                    uint32_t* alive, uint32_t* fract_bits_used) {
    SpzRun run;
    GS_TRY(spz_begin(r, p, s, run));
    if (out && capacity_bytes < run.body_bytes()) return fail(GS_ERR_INVALID_ARGUMENT, "export: the buffer is smaller than the SPZ body");
    if (body_bytes) *body_bytes = run.body_bytes();
    if (alive) *alive = run.total;
    if (fract_bits_used) *fract_bits_used = run.fract;
    if (!out) return GS_OK;
    uint8_t* dst = (uint8_t*)out;
    return run.stream([&](const uint8_t* data, size_t n) { memcpy(dst, data, n); dst += n; return 0; });
}

static int32_t export_spz_impl(gs_renderer* r, const gs_export_params* p, const gs_spz_params* s, const char* path, uint32_t* alive) {
    if (!path) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    SpzRun run;
    GS_TRY(spz_begin(r, p, s, run));                               // every refusal comes before the file exists
    FILE* f = fopen(path, "wb");
    if (!f) { set_error_detail("export: cannot create %s: %s", path, strerror(errno)); return GS_ERR_INVALID_ARGUMENT; }
    int32_t rc = GS_OK;
    {
        GzWriter gz;
        auto put = [&](const uint8_t* data, size_t n, int flush) {
            const int e = gz.write(data, n, flush);
            if (e == 1) set_error_detail("export: deflate failed for %s", path);
            if (e == 2) set_error_detail("export: writing %s failed: %s", path, strerror(errno));
            return e;
        };
        if (gz.begin(f, s->compression_level) != 0) rc = fail(GS_ERR_OUT_OF_MEMORY, "export: deflateInit2 failed");
        if (rc == GS_OK) rc = run.stream([&](const uint8_t* data, size_t n) { return put(data, n, Z_NO_FLUSH); });
        if (rc == GS_OK && put(nullptr, 0, Z_FINISH) != 0) rc = GS_ERR_INVALID_ARGUMENT;
    }
    if (fclose(f) != 0 && rc == GS_OK) { set_error_detail("export: closing %s failed: %s", path, strerror(errno)); rc = GS_ERR_INVALID_ARGUMENT; }
    if (rc != GS_OK) { remove(path); return rc; }                  // no partially written file is left behind
    if (alive) *alive = run.total;
    return GS_OK;
}

// The SPZ export's kernels once, timed by events: ms[0] alive_count + export_scan, ms[1] the alive list + the bounds, ms[2] export_spz
static int32_t export_spz_kernel_times_impl(gs_renderer* r, const gs_export_params* p, const gs_spz_params* s, float ms[3], uint32_t* alive, uint64_t* body_bytes) {
    if (!ms) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    Event ev[6];
    for (Event& e : ev) GS_HIP(e.create(hipEventDefault));
    SpzRun run;
    GS_TRY(spz_begin(r, p, s, run, ev));
    GS_TRY(drain(r->ctx->stream, run.pack(ev), "export: kernel times"));
    for (int k = 0; k < 3; ++k) GS_HIP(hipEventElapsedTime(&ms[k], ev[2 * k], ev[2 * k + 1]));
    if (alive) *alive = run.total;
    if (body_bytes) *body_bytes = run.body_bytes();
    return GS_OK;
}

extern "C" {

int32_t gs_renderer_edit_export_spz_body(gs_renderer* r, const gs_export_params* p, const gs_spz_params* s, void* out, size_t capacity_bytes, uint64_t* body_bytes,
                                         uint32_t* alive, uint32_t* fract_bits_used) {
    return export_guarded([&] { return export_spz_body_impl(r, p, s, out, capacity_bytes, body_bytes, alive, fract_bits_used); });
}

int32_t gs_renderer_edit_export_spz(gs_renderer* r, const gs_export_params* p, const gs_spz_params* s, const char* path, uint32_t* alive) {
    return export_guarded([&] { return export_spz_impl(r, p, s, path, alive); });
}

// A measurement aid of scripts/export_spz_timing.py, which binds it itself: not declared in gsplat_c.h, not part of the ABI
__attribute__((visibility("default"))) int32_t gs_export_spz_kernel_times_for_scripts(gs_renderer* r, const gs_export_params* p, const gs_spz_params* s, float ms[3],
                                                                                    uint32_t* alive, uint64_t* body_bytes) {
    return export_guarded([&] { return export_spz_kernel_times_impl(r, p, s, ms, alive, body_bytes); });
}

int32_t gs_renderer_edit_export_data(gs_renderer* r, const gs_export_params* p, void* out, size_t bytes, int32_t memory_kind) {
    return export_guarded([&] { return export_data_impl(r, p, out, bytes, memory_kind); });
}

int32_t gs_renderer_edit_export_alive(gs_renderer* r, const gs_export_params* p, void* out, size_t capacity_records, uint32_t* alive) {
    return export_guarded([&] { return export_alive_impl(r, p, out, capacity_records, alive); });
}

int32_t gs_renderer_edit_export_ply(gs_renderer* r, const gs_export_params* p, const char* path, uint32_t* alive) {
    return export_guarded([&] { return export_ply_impl(r, p, path, alive); });
}

// A measurement aid of scripts/export_timing.py, which binds it itself: not declared in gsplat_c.h, not part of the ABI.  ms[0..2] = GPU milliseconds of
// alive_count, export_scan and export_records; device_out: device memory, 8-byte aligned, bytes >= alive x 248.
__attribute__((visibility("default"))) int32_t gs_export_kernel_times_for_scripts(gs_renderer* r, const gs_export_params* p, void* device_out, size_t bytes,
                                                                                float ms[3], uint32_t* alive) {
    return export_guarded([&] { return export_kernel_times_impl(r, p, device_out, bytes, ms, alive); });
}

} // extern "C"
