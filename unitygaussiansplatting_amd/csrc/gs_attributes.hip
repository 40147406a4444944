// gs_attributes.hip -- selection by attribute: one fp32 value per splat from the decoded fields (opacity, scale, position, DC colour), the selection of a
// value range, and what an editor's histogram panel shows before it picks the range -- the values themselves, their count / minimum / maximum, a
// histogram, order statistics (gs_renderer_edit_attribute_values / _select_range / _attribute_stats / _attribute_histogram / _attribute_ranks).  No
// counterpart in the reference; the contract and the measurements are DESIGN.md section 4.19, the arithmetic is gsm::Attribute* (gs_device_math.h),
// which tests/attribute_host_harness.cpp runs on the host.
//
// Definitions (gsplat_c.h states them for the host):
//   ALIVE      a splat whose index is < N, that is not deleted and not cut by the renderer's current cutouts (the test of every edit call).
//   FIELDS     LoadSplatData's decoded fields of the renderer's CURRENT blobs (the private copies where a transform or a merge made them), any preset:
//              the object-space position p, the linear scale s (after the chunk de-normalisation and the three squarings), the linear opacity o (after
//              InvSquareCentered01) and the DC colour c (the de-normalised texel rgb, LoadSplatBaseColor).
//   value      gsm::AttributeValue: fp32 throughout, nothing fused, denormals kept, every comparison with NaN false.
//   KEY        gsm::FloatToSortableUint(value): a total order, -0 before +0.
//   SCOPE      GS_SCOPE_ALIVE, or GS_SCOPE_SELECTED: alive, index < N and the selected bit set (empty without edit buffers).
//
// Every kernel walks a grid-stride range of 256-splat chunks with one 256-thread workgroup per chunk, so the chunk header is workgroup-uniform (scalar
// loads), and is built per attribute CLASS -- position, scale, opacity, colour -- so that it loads that class's bytes only: opacity reads the colour
// texel, never `other` or SH; scale reads `other`, never the colour texture; the position is read by its own class and, by the others, only while
// cutouts exist (the cut test needs it).
//   attr_values      the value's bits by splat index, 0xFFFFFFFF for a splat that is not alive
//   attr_select      the chunk's eight selection words from ballots, written whole with |= or &= ~ (selection_apply, gs_block.h): a chunk owns its
//                    words, no atomics
//   attr_stats       per thread the counts and the min / max KEY over its chunks, a wave reduction, one set of global atomics per workgroup into
//                    one of 32 rows the host folds
//   attr_hist        LDS counters (bins + 3 words, at most 4099), one LDS atomic per member (section 4.19: the contention variants that were measured
//                    against it), at the end of the range only non-zero counters flushed with global atomics into a zeroed array.  The grid is
//                    sized to the device
//   attr_keys        the KEY of every splat by index -- all ones for one outside the population -- and the population's size; then the four Onesweep
//                    passes the neighbour grid uses over all N keys (the population's sort to the front), then attr_gather reads the requested positions
#include <cmath>

#include "gs_common.h"
#include "gs_block.h"

namespace gs {

constexpr uint32_t kAttrNotAlive = 0xFFFFFFFFu;
constexpr uint32_t kAttrMaxBins = 4096u, kAttrMaxRanks = 4096u;
constexpr uint32_t kAttrSlots = 32u, kAttrSlotWords = 32u;   // rows of a per-workgroup accumulator (attr_stats, attr_keys) and the words between two rows: a 128-byte line each

struct AttrArgs {
    int attr;
    uint32_t scope;                           // 1: the selected bit must be set
    gsm::V3 q;                                // the point of GS_ATTR_DIST2
    const uint32_t* sel;                      // the selection words (null: no edit buffers -- scope 1 is empty)
};

// is splat idx of chunk ci in the scope, and its value
template <int CLS>
__device__ __forceinline__ bool attr_member(const gsm::AssetView& a, const gsm::EditView& e, const AttrArgs& A, uint32_t idx, uint32_t ci, float& v) {
    v = 0.0f;
    if (idx >= a.n) return false;
    if (e.deletedBits && bit_set(e.deletedBits, idx)) return false;
    if (A.scope && !(A.sel && bit_set(A.sel, idx))) return false;
    gsm::V3 pos = { 0.0f, 0.0f, 0.0f };
    if (CLS == gsm::kAttrClassPos || e.cutoutCount) {              // (wave-uniform) without cutouts nothing is cut and only the position class needs p
        pos = gsm::LoadSplatPosChunk(a, idx, ci);
        if (gsm::IsSplatCut(e, pos.x, pos.y, pos.z)) return false;
    }
    if (CLS == gsm::kAttrClassPos) v = gsm::AttributeOfPos(A.attr, pos, A.q);
    else if (CLS == gsm::kAttrClassScale) v = gsm::AttributeOfScale(A.attr, gsm::LoadSplatScale(a, idx, ci));
    else if (CLS == gsm::kAttrClassOpacity) v = gsm::LoadSplatOpacity(a, idx, ci);
    else v = gsm::AttributeOfColor(A.attr, gsm::LoadSplatBaseColor(a, idx));
    return true;
}

template <int CLS>
__global__ __launch_bounds__(256) void attr_values_kernel(gsm::AssetView a, gsm::EditView e, AttrArgs A, uint32_t chunks, uint32_t* __restrict__ out) {
    for (uint32_t ci = blockIdx.x; ci < chunks; ci += gridDim.x) {
        const uint32_t idx = ci * 256u + threadIdx.x;
        float v;
        const bool mine = attr_member<CLS>(a, e, A, idx, ci, v);
        if (idx < a.n) out[idx] = mine ? gsm::f2u(v) : kAttrNotAlive;
    }
}

// in = alive and lo <= v <= hi; selected |= in (subtract: &= ~in).  A wave owns two consecutive words of its chunk's eight
template <int CLS>
__global__ __launch_bounds__(256) void attr_select_kernel(gsm::AssetView a, gsm::EditView e, AttrArgs A, uint32_t chunks, float lo, float hi, uint32_t* sel,
                                                          uint32_t nWords, uint32_t subtract) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t ci = blockIdx.x; ci < chunks; ci += gridDim.x) {
        const uint32_t idx = ci * 256u + threadIdx.x;
        float v;
        selection_apply(attr_member<CLS>(a, e, A, idx, ci, v) && gsm::AttributeInRange(v, lo, hi), idx, lane, sel, nWords, subtract);
    }
}

// out[0] += members, out[1] += NaN members, out[2] = max(~KEY), out[3] = max(KEY) over the members that are not NaN (both zeroed: a KEY is never 0 or ~0).
// `out` is this workgroup's of kAttrSlots rows, one 128-byte line each: same-address atomics queue behind each other at the memory side (2,048
// workgroups on one line took 40 us, section 4.19), so workgroup b adds to row b % kAttrSlots and the host folds the rows
template <int CLS>
__global__ __launch_bounds__(256) void attr_stats_kernel(gsm::AssetView a, gsm::EditView e, AttrArgs A, uint32_t chunks, uint32_t* __restrict__ rows) {
    uint32_t* out = rows + (blockIdx.x % kAttrSlots) * kAttrSlotWords;
    __shared__ uint32_t s_part[4][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t acc[4] = { 0u, 0u, 0u, 0u };
    for (uint32_t ci = blockIdx.x; ci < chunks; ci += gridDim.x) {
        float v;
        if (!attr_member<CLS>(a, e, A, ci * 256u + threadIdx.x, ci, v)) continue;
        ++acc[0];
        if (gsm::AttributeIsNaN(v)) { ++acc[1]; continue; }
        const uint32_t key = gsm::FloatToSortableUint(v);
        acc[2] = max(acc[2], ~key);
        acc[3] = max(acc[3], key);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        acc[0] += (uint32_t)__shfl_xor((int)acc[0], m);
        acc[1] += (uint32_t)__shfl_xor((int)acc[1], m);
        acc[2] = max(acc[2], (uint32_t)__shfl_xor((int)acc[2], m));
        acc[3] = max(acc[3], (uint32_t)__shfl_xor((int)acc[3], m));
    }
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_part[wave][k] = acc[k];
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < 4u) {
        const uint32_t p0 = s_part[0][t], p1 = s_part[1][t], p2 = s_part[2][t], p3 = s_part[3][t];
        if (t < 2u) {
            const uint32_t sum = p0 + p1 + p2 + p3;
            if (sum) atomicAdd(out + t, sum);
        } else {
            const uint32_t hi = max(max(p0, p1), max(p2, p3));
            if (hi) atomicMax(out + t, hi);
        }
    }
}

// hist[gsm::AttributeBin(v)] += 1 for every member.  s_hist: `copies` x (bins + 3) LDS counters, wave w adding to copy w % copies.  ROUNDS: the lanes of a
// wave that hold the leader's bin are folded into one add of their number, for up to ROUNDS distinct bins; the lanes left add one each
template <int CLS, int ROUNDS>
__global__ __launch_bounds__(256) void attr_hist_kernel(gsm::AssetView a, gsm::EditView e, AttrArgs A, uint32_t chunks, float lo, float hi, float s, uint32_t bins,
                                                        uint32_t copies, uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t s_hist[];
    const uint32_t words = bins + 3u, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < words * copies; i += 256u) s_hist[i] = 0u;
    __syncthreads();
    uint32_t* mine_hist = s_hist + (wave % copies) * words;
    for (uint32_t ci = blockIdx.x; ci < chunks; ci += gridDim.x) {
        float v;
        const bool mine = attr_member<CLS>(a, e, A, ci * 256u + threadIdx.x, ci, v);
        const uint32_t bin = mine ? gsm::AttributeBin(v, lo, hi, s, bins) : 0u;      // < words
        unsigned long long left = __ballot(mine);                  // wave-uniform: the lanes not counted yet
        if (ROUNDS > 0) {
#pragma unroll 1
            for (int round = 0; round < ROUNDS && left; ++round) {
                const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1u;
                const uint32_t b0 = (uint32_t)__shfl((int)bin, (int)leader);
                const unsigned long long group = __ballot(mine && bin == b0);        // every lane that holds b0 is still in `left`: equal bins leave together
                left &= ~group;
                if (lane == leader) atomicAdd(mine_hist + b0, (uint32_t)__popcll(group));
            }
        }
        if ((left >> lane) & 1ull) atomicAdd(mine_hist + bin, 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < words; i += 256u) {
        uint32_t c = 0u;
        for (uint32_t k = 0; k < copies; ++k) c += s_hist[k * words + i];
        if (c) atomicAdd(hist + i, c);
    }
}

// keys[idx] = the KEY of splat idx if it is a member whose value is not NaN, else all ones -- which no number's KEY is and which sorts behind every one --
// for every idx < N, and the population counted into this workgroup's row of `rows` (as attr_stats).  Nothing is compacted: all N keys are sorted and
// the population's stand in front.  (A per-wave atomic append into a compact list was built first: 96,000 returning atomics on one word, 1.8 ms at
// 6.1 M splats against 0.23 ms for the sort itself, section 4.19.)
template <int CLS>
__global__ __launch_bounds__(256) void attr_keys_kernel(gsm::AssetView a, gsm::EditView e, AttrArgs A, uint32_t chunks, uint32_t* __restrict__ keys, uint32_t* __restrict__ rows) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t count = 0u;
    for (uint32_t ci = blockIdx.x; ci < chunks; ci += gridDim.x) {
        const uint32_t idx = ci * 256u + threadIdx.x;
        float v;
        const bool mine = attr_member<CLS>(a, e, A, idx, ci, v) && !gsm::AttributeIsNaN(v);
        if (idx < a.n) keys[idx] = mine ? gsm::FloatToSortableUint(v) : kAttrNotAlive;
        count += mine ? 1u : 0u;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) count += (uint32_t)__shfl_xor((int)count, m);
    if (lane == 0u) s_cnt[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t sum = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (sum) atomicAdd(rows + (blockIdx.x % kAttrSlots) * kAttrSlotWords, sum);
    }
}

// out[k] = the value whose KEY stands at sorted position ranks[k]; 0xFFFFFFFF where there is no such position
__global__ __launch_bounds__(256) void attr_gather_kernel(const uint32_t* __restrict__ keys, uint32_t m, const uint32_t* __restrict__ ranks, uint32_t rankCount,
                                                          uint32_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= rankCount) return;
    const uint32_t at = ranks[k];
    const uint32_t key = at < m ? keys[at] : kAttrNotAlive;       // m = N here: a position behind the population holds all ones
    out[k] = key != kAttrNotAlive ? gsm::f2u(gsm::SortableUintToFloat(key)) : kAttrNotAlive;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
#define GS_ATTR_CLASS_SWITCH(cls, LAUNCH)                                  \
    switch (cls) {                                                         \
    case gsm::kAttrClassPos: LAUNCH(gsm::kAttrClassPos); break;            \
    case gsm::kAttrClassScale: LAUNCH(gsm::kAttrClassScale); break;        \
    case gsm::kAttrClassOpacity: LAUNCH(gsm::kAttrClassOpacity); break;    \
    default: LAUNCH(gsm::kAttrClassColor); break;                          \
    }

// what scripts/attribute_timing.py asks of a call besides its result: events around its kernels (0, 1) and around the sort of the ranks (2, 3), all
// recorded whenever the call succeeds; the histogram's contention variant (-1: the library's choice; else attr_hist_variant's bits)
enum { kAttrEvStart = 0, kAttrEvEnd, kAttrEvSortStart, kAttrEvSortEnd, kAttrEvents };
struct AttrProbe { hipEvent_t ev[kAttrEvents]; int variant; };

// the refusals every entry point shares; fills what the kernels take
static int32_t attr_begin(gs_renderer* r, int32_t attr, const float* point, int32_t scope, AttrArgs& A) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    if (r->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane holds no edit state: edit its owner");
    if (attr < 0 || attr >= gsm::kAttrCount) return fail(GS_ERR_INVALID_ARGUMENT, "attribute: unknown gs_splat_attribute");
    if (scope != GS_SCOPE_ALIVE && scope != GS_SCOPE_SELECTED) return fail(GS_ERR_INVALID_ARGUMENT, "attribute: unknown scope");
    A.attr = attr;
    A.scope = scope == GS_SCOPE_SELECTED ? 1u : 0u;
    A.q = { 0.0f, 0.0f, 0.0f };
    A.sel = r->editSelected.get();
    if (attr == GS_ATTR_DIST2) {
        if (!point || !std::isfinite(point[0]) || !std::isfinite(point[1]) || !std::isfinite(point[2]))
            return fail(GS_ERR_INVALID_ARGUMENT, "attribute: GS_ATTR_DIST2 needs a finite point");
        A.q = { point[0], point[1], point[2] };
    }
    GS_HIP(hipSetDevice(r->ctx->device));
    return GS_OK;
}

static inline uint32_t attr_chunks(const gs_renderer* r) { return (r->n + 255u) / 256u; }
// workgroups of a streaming pass: the chunks, or perCU workgroups on every CU striding over them
static inline uint32_t attr_grid(const gs_renderer* r, uint32_t perCU) {
    const uint32_t chunks = attr_chunks(r), cap = (uint32_t)(r->ctx->cuCount > 0 ? r->ctx->cuCount : 1) * perCU;
    return chunks < cap ? (chunks ? chunks : 1u) : cap;
}

static int32_t attr_values_impl(gs_renderer* r, int32_t attr, const float* point, float* values_out, size_t count, const AttrProbe* probe) {
    AttrArgs A;
    GS_TRY(attr_begin(r, attr, point, GS_SCOPE_ALIVE, A));
    if (!values_out) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_values: values_out is null");
    if (count != (size_t)r->n) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_values: count must be the renderer's splat count");
    hipStream_t st = r->ctx->stream;
    DevBuf<uint32_t> out;
    return drain(st, [&]() -> int32_t {
        GS_HIP(out.alloc(((size_t)r->n + 16) * 4));
        GS_HIP(mark_events(events_of(probe), kAttrEvStart, kAttrEvStart, st));
        if (r->n) {
#define GS_ATTR_LAUNCH(C) hipLaunchKernelGGL(attr_values_kernel<C>, dim3(attr_grid(r, 8u)), dim3(256), 0, st, asset_view(r), edit_view(r), A, attr_chunks(r), out.get())
            GS_ATTR_CLASS_SWITCH(gsm::AttributeClass(attr), GS_ATTR_LAUNCH)
#undef GS_ATTR_LAUNCH
            GS_HIP(hipGetLastError());
        }
        GS_HIP(mark_events(events_of(probe), kAttrEvEnd, kAttrEvSortEnd, st));
        if (r->n) GS_HIP(hipMemcpyAsync(values_out, out.get(), (size_t)r->n * 4, hipMemcpyDeviceToHost, st));
        return GS_OK;
    }(), "attribute_values");
}

static int32_t attr_select_impl(gs_renderer* r, int32_t attr, const float* point, float lo, float hi, int32_t subtract, const AttrProbe* probe) {
    AttrArgs A;
    GS_TRY(attr_begin(r, attr, point, GS_SCOPE_ALIVE, A));
    if (std::isnan(lo) || std::isnan(hi)) return fail(GS_ERR_INVALID_ARGUMENT, "select_range: lo or hi is NaN");
    GS_TRY(edit_ensure(r));
    hist_mutated(r, true);
    hipStream_t st = r->ctx->stream;
    GS_HIP(mark_events(events_of(probe), kAttrEvStart, kAttrEvStart, st));
    if (r->n && lo <= hi) {                                        // lo > hi: nothing is in the range
#define GS_ATTR_LAUNCH(C) hipLaunchKernelGGL(attr_select_kernel<C>, dim3(attr_grid(r, 8u)), dim3(256), 0, st, asset_view(r), edit_view(r), A, attr_chunks(r), lo, hi, \
                                             r->editSelected.get(), (uint32_t)bit_words(r->n), subtract ? 1u : 0u)
        GS_ATTR_CLASS_SWITCH(gsm::AttributeClass(attr), GS_ATTR_LAUNCH)
#undef GS_ATTR_LAUNCH
        GS_HIP(hipGetLastError());
    }
    GS_HIP(mark_events(events_of(probe), kAttrEvEnd, kAttrEvSortEnd, st));
    return edit_selected_to_lanes(r);
}

static int32_t attr_stats_impl(gs_renderer* r, int32_t attr, const float* point, int32_t scope, gs_attribute_stats* out, const AttrProbe* probe) {
    AttrArgs A;
    GS_TRY(attr_begin(r, attr, point, scope, A));
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_stats: out is null");
    hipStream_t st = r->ctx->stream;
    DevBuf<uint32_t> acc;
    constexpr size_t accBytes = (size_t)kAttrSlots * kAttrSlotWords * 4;
    uint32_t rows[kAttrSlots * kAttrSlotWords] = {};
    const int32_t rc = [&]() -> int32_t {
        GS_HIP(acc.alloc(accBytes));
        GS_HIP(hipMemsetAsync(acc, 0, accBytes, st));
        GS_HIP(mark_events(events_of(probe), kAttrEvStart, kAttrEvStart, st));
        if (r->n) {
#define GS_ATTR_LAUNCH(C) hipLaunchKernelGGL(attr_stats_kernel<C>, dim3(attr_grid(r, 8u)), dim3(256), 0, st, asset_view(r), edit_view(r), A, attr_chunks(r), acc.get())
            GS_ATTR_CLASS_SWITCH(gsm::AttributeClass(attr), GS_ATTR_LAUNCH)
#undef GS_ATTR_LAUNCH
            GS_HIP(hipGetLastError());
        }
        GS_HIP(mark_events(events_of(probe), kAttrEvEnd, kAttrEvSortEnd, st));
        GS_HIP(hipMemcpyAsync(rows, acc.get(), accBytes, hipMemcpyDeviceToHost, st));
        return GS_OK;
    }();
    GS_TRY(drain(st, rc, "attribute_stats"));
    uint32_t host[4] = { 0u, 0u, 0u, 0u };
    for (uint32_t k = 0; k < kAttrSlots; ++k) {                    // integer sums and maxima: any grouping gives the same words
        const uint32_t* row = rows + k * kAttrSlotWords;
        host[0] += row[0]; host[1] += row[1];
        host[2] = row[2] > host[2] ? row[2] : host[2]; host[3] = row[3] > host[3] ? row[3] : host[3];
    }
    out->members = host[0];
    out->nans = host[1];
    const bool any = host[0] != host[1];                           // a member that is not NaN
    out->vmin = any ? gsm::SortableUintToFloat(~host[2]) : gsm::u2f(0x7f800000u);
    out->vmax = any ? gsm::SortableUintToFloat(host[3]) : gsm::u2f(0xff800000u);
    return GS_OK;
}

// the contention variant of a histogram launch: bit 0 the wave fold over four bins, bit 1 per-wave LDS copies, bit 2 the wave fold over the leader's bin only.
// The library's is none of them: plain LDS atomics were the fastest on the scene's own opacity and on uniform values, and 5 us behind the fold where
// every value is equal (section 4.19)
constexpr int kAttrHistVariant = 0;
static inline int attr_hist_variant(const AttrProbe* probe) { return probe && probe->variant >= 0 ? probe->variant : kAttrHistVariant; }

static int32_t attr_histogram_impl(gs_renderer* r, int32_t attr, const float* point, int32_t scope, float lo, float hi, uint32_t bins, uint32_t* hist_out, size_t count,
                                   const AttrProbe* probe) {
    AttrArgs A;
    GS_TRY(attr_begin(r, attr, point, scope, A));
    if (!hist_out) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_histogram: hist_out is null");
    if (bins < 1u || bins > kAttrMaxBins) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_histogram: bins must be within [1, 4096]");
    if (count != (size_t)bins + 3) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_histogram: count must be bins + 3");
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_histogram: lo and hi must be finite and lo < hi");
    const float w = hi - lo;
    if (!std::isfinite(w)) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_histogram: hi - lo is not finite in fp32");
    const float s = (float)bins / w;
    if (!std::isfinite(s)) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_histogram: bins / (hi - lo) is not finite in fp32");
    hipStream_t st = r->ctx->stream;
    const uint32_t words = bins + 3u;
    const int variant = attr_hist_variant(probe);
    const uint32_t copies = ((variant & 2) && words <= 1024u) ? 4u : 1u;
    DevBuf<uint32_t> hist;
    return drain(st, [&]() -> int32_t {
        GS_HIP(hist.alloc((size_t)words * 4));
        GS_HIP(hipMemsetAsync(hist, 0, (size_t)words * 4, st));
        GS_HIP(mark_events(events_of(probe), kAttrEvStart, kAttrEvStart, st));
        if (r->n) {
            const size_t lds = (size_t)words * copies * 4;
#define GS_ATTR_LAUNCH_V(C, G) hipLaunchKernelGGL((attr_hist_kernel<C, G>), dim3(attr_grid(r, 4u)), dim3(256), lds, st, asset_view(r), edit_view(r), A, attr_chunks(r), lo, hi, s, \
                                                  bins, copies, hist.get())
#define GS_ATTR_LAUNCH(C) do { if (variant & 1) GS_ATTR_LAUNCH_V(C, 4); else if (variant & 4) GS_ATTR_LAUNCH_V(C, 1); else GS_ATTR_LAUNCH_V(C, 0); } while (0)
            GS_ATTR_CLASS_SWITCH(gsm::AttributeClass(attr), GS_ATTR_LAUNCH)
#undef GS_ATTR_LAUNCH
#undef GS_ATTR_LAUNCH_V
            GS_HIP(hipGetLastError());
        }
        GS_HIP(mark_events(events_of(probe), kAttrEvEnd, kAttrEvSortEnd, st));
        GS_HIP(hipMemcpyAsync(hist_out, hist.get(), (size_t)words * 4, hipMemcpyDeviceToHost, st));
        return GS_OK;
    }(), "attribute_histogram");
}

static int32_t attr_ranks_impl(gs_renderer* r, int32_t attr, const float* point, int32_t scope, const uint32_t* ranks, uint32_t rank_count, float* values_out,
                               uint32_t* population, const AttrProbe* probe) {
    AttrArgs A;
    GS_TRY(attr_begin(r, attr, point, scope, A));
    if (!population) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_ranks: population is null");
    if (rank_count > kAttrMaxRanks) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_ranks: at most 4096 ranks");
    if (rank_count && (!ranks || !values_out)) return fail(GS_ERR_INVALID_ARGUMENT, "attribute_ranks: ranks or values_out is null");
    GS_TRY(gs_context_synchronize(r->ctx));                        // after everything enqueued, the lanes' frames included: the sort wants the GPU to itself
    hipStream_t st = r->ctx->stream;
    gs_context* ctx = r->ctx;
    DevBuf<uint32_t> keys, vals, counter, ranksDev, outDev;
    DevBuf<SortControl> control;
    SortState sort;
    constexpr size_t rowBytes = (size_t)kAttrSlots * kAttrSlotWords * 4;
    uint32_t rows[kAttrSlots * kAttrSlotWords] = {};
    uint32_t err = 0;
    const uint32_t n = r->n;
    std::vector<uint32_t> got(rank_count, kAttrNotAlive);
    const int32_t rc = [&]() -> int32_t {
        GS_HIP(mark_events(events_of(probe), kAttrEvStart, kAttrEvStart, st));
        if (n) {
            GS_HIP(keys.alloc(((size_t)n + 16) * 4));
            GS_HIP(vals.alloc(((size_t)n + 16) * 4));              // the sorter moves pairs: a payload nobody reads
            GS_HIP(counter.alloc(rowBytes));
            GS_HIP(hipMemsetAsync(counter, 0, rowBytes, st));
            GS_HIP(hipMemsetAsync(vals, 0, (size_t)n * 4, st));
            GS_TRY(sort_state_create(ctx, sort, n, true));
            GS_HIP(control.alloc(sizeof(SortControl)));
#define GS_ATTR_LAUNCH(C) hipLaunchKernelGGL(attr_keys_kernel<C>, dim3(attr_grid(r, 8u)), dim3(256), 0, st, asset_view(r), edit_view(r), A, attr_chunks(r), keys.get(), counter.get())
            GS_ATTR_CLASS_SWITCH(gsm::AttributeClass(attr), GS_ATTR_LAUNCH)
#undef GS_ATTR_LAUNCH
            GS_HIP(hipGetLastError());
            GS_HIP(hipMemcpyAsync(rows, counter.get(), rowBytes, hipMemcpyDeviceToHost, st));
            GS_HIP(mark_events(events_of(probe), kAttrEvSortStart, kAttrEvSortStart, st));
            GS_TRY(enqueue_histogram(ctx, st, keys, n, nullptr, 4, 255u, control.get(), sort));
            GS_TRY(enqueue_sort_passes(ctx, st, sort, control.get(), keys, vals, n, nullptr, 4, 255u));
            GS_HIP(mark_events(events_of(probe), kAttrEvSortEnd, kAttrEvSortEnd, st));
        } else {
            GS_HIP(mark_events(events_of(probe), kAttrEvSortStart, kAttrEvSortEnd, st));
        }
        if (rank_count && n) {
            // the population m is not known on the host yet: a rank at or beyond it reads a key of all ones, the word the gather writes for it anyway
            GS_HIP(ranksDev.alloc((size_t)rank_count * 4));
            GS_HIP(outDev.alloc((size_t)rank_count * 4));
            GS_HIP(hipMemcpyAsync(ranksDev, ranks, (size_t)rank_count * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(attr_gather_kernel, dim3((rank_count + 255u) / 256u), dim3(256), 0, st, (const uint32_t*)keys.get(), n, (const uint32_t*)ranksDev.get(),
                               rank_count, outDev.get());
            GS_HIP(hipGetLastError());
            GS_HIP(hipMemcpyAsync(got.data(), outDev.get(), (size_t)rank_count * 4, hipMemcpyDeviceToHost, st));
        }
        GS_HIP(mark_events(events_of(probe), kAttrEvEnd, kAttrEvEnd, st));
        if (n) GS_HIP(hipMemcpyAsync(&err, &control.get()->error, 4, hipMemcpyDeviceToHost, st));
        return GS_OK;
    }();
    GS_TRY(drain(st, rc, "attribute_ranks"));
    if (err) return fail(GS_ERR_SORT_TIMEOUT, "attribute_ranks: a bounded look-back spin expired");
    uint32_t m = 0;
    for (uint32_t k = 0; k < kAttrSlots; ++k) m += rows[k * kAttrSlotWords];
    if (rank_count) memcpy(values_out, got.data(), (size_t)rank_count * 4);
    *population = m;
    return GS_OK;
}

} // namespace gs

using namespace gs;

extern "C" {

int32_t gs_renderer_edit_attribute_values(gs_renderer* r, int32_t attr, const float point[3], float* values_out, size_t count) {
    return attr_values_impl(r, attr, point, values_out, count, nullptr);
}

int32_t gs_renderer_edit_select_range(gs_renderer* r, int32_t attr, const float point[3], float lo, float hi, int32_t subtract) {
    return attr_select_impl(r, attr, point, lo, hi, subtract, nullptr);
}

int32_t gs_renderer_edit_attribute_stats(gs_renderer* r, int32_t attr, const float point[3], int32_t scope, gs_attribute_stats* out) {
    return attr_stats_impl(r, attr, point, scope, out, nullptr);
}

int32_t gs_renderer_edit_attribute_histogram(gs_renderer* r, int32_t attr, const float point[3], int32_t scope, float lo, float hi, uint32_t bins, uint32_t* hist_out,
                                             size_t count) {
    return attr_histogram_impl(r, attr, point, scope, lo, hi, bins, hist_out, count, nullptr);
}

int32_t gs_renderer_edit_attribute_ranks(gs_renderer* r, int32_t attr, const float point[3], int32_t scope, const uint32_t* ranks, uint32_t rank_count, float* values_out,
                                         uint32_t* population) {
    return attr_ranks_impl(r, attr, point, scope, ranks, rank_count, values_out, population, nullptr);
}

// A measurement aid of scripts/attribute_timing.py, which binds it itself: not declared in gsplat_c.h, not part of the ABI.  One whole call with events
// inside it -- op 0: gs_renderer_edit_select_range(attr, lo, hi, 0); 1: _attribute_stats; 2: _attribute_histogram at `bins` with contention variant
// `variant` (-1: the library's; bit 0 the wave fold over four bins, bit 1 per-wave LDS copies, bit 2 the fold over one bin); 3: _attribute_ranks of rank 0; 4: _attribute_values; 5: the floor --
// the alive count of the export (enqueue_alive_counts: alive_count_kernel and its scan over the chunks), which reads positions, deleted words and cutouts only.
// ms[0] = GPU milliseconds of the call's kernels, ms[1] = of the sort inside op 3 (else 0).
__attribute__((visibility("default"))) int32_t gs_attribute_times_for_scripts(gs_renderer* r, int32_t op, int32_t attr, const float* point, int32_t scope, float lo, float hi,
                                                                               uint32_t bins, int32_t variant, float ms[2]) {
    if (!r || !ms || op < 0 || op > 5) return fail(GS_ERR_INVALID_ARGUMENT, "bad argument");
    GS_HIP(hipSetDevice(r->ctx->device));
    Event owned[kAttrEvents];
    AttrProbe probe = {};
    probe.variant = variant;
    for (int k = 0; k < kAttrEvents; ++k) { GS_HIP(owned[k].create(hipEventDefault)); probe.ev[k] = owned[k]; }
    hipStream_t st = r->ctx->stream;
    if (op == 0) GS_TRY(attr_select_impl(r, attr, point, lo, hi, 0, &probe));
    else if (op == 1) { gs_attribute_stats s; GS_TRY(attr_stats_impl(r, attr, point, scope, &s, &probe)); }
    else if (op == 2) {
        std::vector<uint32_t> h((size_t)bins + 3);
        GS_TRY(attr_histogram_impl(r, attr, point, scope, lo, hi, bins, h.data(), h.size(), &probe));
    } else if (op == 3) {
        const uint32_t rank = 0; float v; uint32_t pop;
        GS_TRY(attr_ranks_impl(r, attr, point, scope, &rank, 1, &v, &pop, &probe));
    } else if (op == 4) {
        std::vector<float> v(r->n);
        GS_TRY(attr_values_impl(r, attr, point, v.data(), v.size(), &probe));
    } else {
        if (r->laneOf || r->n == 0u) return fail(GS_ERR_INVALID_ARGUMENT, "bad argument");
        const uint32_t chunks = (r->n + 255u) / 256u;
        DevBuf<uint32_t> counts, base;
        GS_HIP(counts.alloc((size_t)chunks * 4));
        GS_HIP(base.alloc(((size_t)chunks + 1) * 4));
        GS_HIP(mark_events(probe.ev, kAttrEvStart, kAttrEvStart, st));
        const int32_t rc = enqueue_alive_counts(st, asset_view(r), edit_view(r), false, chunks, counts.get(), base.get());
        GS_HIP(mark_events(probe.ev, kAttrEvEnd, kAttrEvSortEnd, st));
        GS_HIP(hipStreamSynchronize(st));
        GS_TRY(rc);
    }
    GS_HIP(hipEventSynchronize(probe.ev[kAttrEvEnd]));
    GS_HIP(hipEventSynchronize(probe.ev[kAttrEvSortEnd]));
    GS_HIP(hipEventElapsedTime(&ms[0], probe.ev[kAttrEvStart], probe.ev[kAttrEvEnd]));
    ms[1] = 0.0f;
    if (op == 3) GS_HIP(hipEventElapsedTime(&ms[1], probe.ev[kAttrEvSortStart], probe.ev[kAttrEvSortEnd]));
    return GS_OK;
}

} // extern "C"
