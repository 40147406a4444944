// gs_export.hip -- exporting the edited splats: CSExportData (SplatUtilities.compute:523-673), GaussianSplatRenderer.EditExportData
// (GaussianSplatRenderer.cs:936-958) and the editor's ExportPlyFile (GaussianSplatRendererEditor.cs:394-445) as the gs_renderer_edit_export_* entry points.
//
// CSExportData only READS the asset, the cutouts and the transform and writes a buffer of its own, so it fits the immutable, shared asset of this
// library.  The per-splat arithmetic is gsm::ExportSplat (gs_device_math.h): the full LoadSplatData decode, the optional baked transform, and the
// 62-float record (ExportSplatData = InputSplatData = the PLY vertex), word for word what the reference leaves in memory for the member of HLSL's
// log / sqrt families the project fixes (LogDetFull, the band matrices' recurrence).
//
// Three plain launches, none waits on another workgroup (an offline path on shared machines: no look-back, no spinning):
//   export_count    per 256-splat chunk, the number of splats that are alive (idx < N, not deleted, not cut): popcounts of ballots.  Reads positions,
//                   the deleted words and the cutouts only.
//   export_scan     exclusive prefix over the chunk counts, one workgroup looping over the array 1024 counts at a time; base[chunks] = the total.
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
#include <stdlib.h>
#include <new>
#include <string>

#include "gs_common.h"

namespace gs {

constexpr uint32_t kRecFloats = GS_EXPORT_RECORD_BYTES / 4;       // 62
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kExportBatchDefault = 131072;                  // splats per batch: 31 MB of records in the device buffer and in each pinned buffer
static_assert(kRecFloats * 4 == GS_EXPORT_RECORD_BYTES && kRecFloats % 2 == 0, "records are whole dwordx2s");

__global__ __launch_bounds__(256) void export_count_kernel(gsm::AssetView a, gsm::EditView e, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    gsm::V3 pos; bool cut;
    const bool alive = export_alive(a, e, idx, blockIdx.x, pos, cut);
    const uint32_t c = (uint32_t)__popcll(__ballot(alive));
    if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = c;
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

// counts[c] = alive splats of chunk c, base = their exclusive prefix (base[chunks] = the total), on st: the two launches every compaction starts with
// (the export's, and the bake's in gs_bake.hip)
int32_t enqueue_alive_counts(hipStream_t st, const gsm::AssetView& a, const gsm::EditView& e, uint32_t chunks, uint32_t* counts, uint32_t* base) {
    hipLaunchKernelGGL(export_count_kernel, dim3(chunks), dim3(256), 0, st, a, e, counts);
    hipLaunchKernelGGL(export_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t*)counts, base, chunks);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// out: the records of the chunks [firstChunk, firstChunk + gridDim.x).  base == null: record idx - firstChunk * 256 for every idx < N; else record
// base[chunk] - base[firstChunk] + rank for the alive ones.
__global__ __launch_bounds__(256) void export_records_kernel(gsm::AssetView a, gsm::EditView e, gsm::ExportXform X, const uint32_t* __restrict__ base,
                                                             uint32_t firstChunk, float* __restrict__ out) {
    const uint32_t ci = firstChunk + blockIdx.x, idx = ci * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __shared__ uint32_t s_cnt[4];
    gsm::V3 pos; bool cut;
    const bool alive = export_alive(a, e, idx, ci, pos, cut);
    const bool mine = base ? alive : (idx < a.n);                  // does this lane write a record?
    const unsigned long long bal = __ballot(mine);
    const uint32_t waveCount = (uint32_t)__popcll(bal);
    const uint32_t slot = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));      // rank inside the wave (reference-shaped: the lane itself, the tail is at the end)
    if (lane == 0u) s_cnt[wave] = waveCount;
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
    uint32_t first = base ? (base[ci] - base[firstChunk]) : blockIdx.x * 256u;      // first record of the workgroup, then of the wave
    for (uint32_t w = 0; w < wave; ++w) first += s_cnt[w];
#ifndef GS_EXPORT_DIRECT
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
        GS_TRY(enqueue_alive_counts(st, asset_view(r), edit_view(r), chunks, counts.get(), base.get()));
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
        const hipError_t he = hipGetLastError();
        GS_HIP(hipStreamSynchronize(r->ctx->stream));
        GS_HIP(he);
        return GS_OK;
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
    hipError_t he = hipEventRecord(ev[0], st);
    hipLaunchKernelGGL(export_count_kernel, dim3(run.chunks), dim3(256), 0, st, asset_view(r), edit_view(r), run.counts.get());
    if (he == hipSuccess) he = hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(export_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t*)run.counts.get(), run.base.get(), run.chunks);
    if (he == hipSuccess) he = hipEventRecord(ev[2], st);
    run.launch(0, run.chunks, (float*)device_out);
    if (he == hipSuccess) he = hipEventRecord(ev[3], st);
    if (he == hipSuccess) he = hipGetLastError();
    const hipError_t hs = hipStreamSynchronize(st);                // whatever failed: nothing in flight outlives the events and the buffers
    GS_HIP(he);
    GS_HIP(hs);
    for (int k = 0; k < 3; ++k) GS_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    return GS_OK;
}

extern "C" {

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
// export_count, export_scan and export_records; device_out: device memory, 8-byte aligned, bytes >= alive x 248.
__attribute__((visibility("default"))) int32_t gs_export_kernel_times_for_scripts(gs_renderer* r, const gs_export_params* p, void* device_out, size_t bytes,
                                                                                float ms[3], uint32_t* alive) {
    return export_guarded([&] { return export_kernel_times_impl(r, p, device_out, bytes, ms, alive); });
}

} // extern "C"
