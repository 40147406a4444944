// gs_neighbours.hip -- the floater tool: for every alive splat, how many other alive splats lie within `radius` of it (gs_renderer_edit_neighbour_counts),
// and the selection of those with fewer than `min_neighbours` (gs_renderer_edit_select_sparse).  No counterpart in the reference; the contract, the
// grid argument and the measurements are DESIGN.md section 4.17, the arithmetic is gsm::Neighbour* (gs_device_math.h), which tests/neighbour_host_harness.cpp
// runs on the host.
//
// One call, on the context's stream, everything transient and freed before it returns:
//   1. enqueue_alive_counts + enqueue_alive_list   the LIST (gs_compact.hip, finiteOnly): alive splats (index < N, not deleted, not cut -- export_alive, the test
//                                                  of every edit kernel) whose position is finite, in index order, and (minOnly) the per-axis
//                                                  minimum of their positions, the grid's origin
//   2. nb_keys + TwoWordSort                       the 63-bit cell key of every listed splat, x lowest, sorted as the bake sorts its Morton codes
//                                                  (gs_compact.hip): the low word over 32 bits, then the gathered high word over 31
//   3. nb_records                                  the sorted splats as 16-byte records (x, y, z, index) and their keys: what the walk streams
//   4. nb_walk                                     one thread per listed splat in SORTED order -- the lanes of a wave then search for the same runs and walk
//                                                  the same cache lines -- nine runs each (gsm::NeighbourCount: the start by bisection, the end by doubling
//                                                  steps from it), stopping at the limit; one store per splat
//   5. nb_counts_out / nb_apply                    by splat index, 256-thread workgroups like gs_edit.hip: the host's array, or the predicate into the
//                                                  selection words (selection_apply, gs_block.h)
// No atomics (but the optional statistic of the timing script), no workgroup waits on another outside the sorts, no scratch, no LDS beyond the reductions'.
//
// The island tools (gs_renderer_edit_components / _select_islands / _grow_selection) share steps 1 to 3 (nb_grid) and go on:
//   4'. cc_init + cc_link                          a lock-free union-find over the sorted positions: one thread per listed splat in sorted order, every edge
//                                                  to an EARLIER sorted position (gsm::NeighbourForEach) a union -- agent-scope relaxed atomics only, no
//                                                  waiting on another wave
//   5'. cc_flatten, cc_reduce, cc_labels, cc_out   after the kernel boundary: the root of every position, per root the smallest splat index and the
//                                                  size, then both by splat index (an alive splat that is not listed is a component of its own)
//   6'. cc_islands_apply / cc_seed + cc_grow_apply the selection words, in nb_apply's shape
#include <cmath>

#include "gs_common.h"
#include "gs_block.h"

namespace gs {

constexpr uint32_t kNbNotAlive = 0xFFFFFFFFu;

// the cell key of listed splat j as two sort keys, and the identity payload
__global__ __launch_bounds__(256) void nb_keys_kernel(gsm::AssetView a, const uint32_t* __restrict__ list, const float* __restrict__ origin, double h, uint32_t m,
                                                      uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, uint32_t* __restrict__ rank) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= m) return;
    const uint32_t idx = list[j];
    const unsigned long long key = gsm::NeighbourKeyOf(gsm::LoadSplatPosChunk(a, idx, idx >> 8), origin, h);
    lo[j] = (uint32_t)key; hi[j] = (uint32_t)(key >> 32); rank[j] = j;
}

// sorted position i: the record and the key of the splat the two sorts put there
__global__ __launch_bounds__(256) void nb_records_kernel(gsm::AssetView a, const uint32_t* __restrict__ list, const uint32_t* __restrict__ rank,
                                                         const float* __restrict__ origin, double h, uint32_t m, gsm::NeighbourRec* __restrict__ recs,
                                                         unsigned long long* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint32_t idx = list[rank[i]];
    const gsm::V3 p = gsm::LoadSplatPosChunk(a, idx, idx >> 8);
    recs[i] = { p.x, p.y, p.z, idx };
    keys[i] = gsm::NeighbourKeyOf(p, origin, h);
}

// counts[index of the splat at sorted position i] = min(count, limit); tests: null, or where every wave adds the predicates it evaluated
__global__ __launch_bounds__(256) void nb_walk_kernel(const unsigned long long* __restrict__ keys, const gsm::NeighbourRec* __restrict__ recs, uint32_t m, float r2,
                                                      uint32_t limit, uint32_t* __restrict__ counts, unsigned long long* __restrict__ tests) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t mine = 0u;
    if (i < m) counts[recs[i].idx] = gsm::NeighbourCount(keys, recs, m, i, r2, limit, mine);
    if (tests) {
        unsigned long long t = mine;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t += (unsigned long long)__shfl_xor((int)(uint32_t)t, d) | ((unsigned long long)__shfl_xor((int)(uint32_t)(t >> 32), d) << 32);
        if ((threadIdx.x & 63u) == 0u && t) atomicAdd(tests, t);
    }
}

// what the host gets: the count of an alive splat (0 for one that is not listed: its position is not finite), 0xFFFFFFFF for every other splat
__global__ __launch_bounds__(256) void nb_counts_out_kernel(gsm::AssetView a, gsm::EditView e, uint32_t* __restrict__ counts) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= a.n) return;
    gsm::V3 pos; bool cut;
    if (!export_alive(a, e, idx, blockIdx.x, pos, cut)) counts[idx] = kNbNotAlive;
}

// sparse = alive and count < minNeighbours; selected |= sparse (subtract: &= ~sparse).  The shape of gs_edit.hip: a wave owns two consecutive words
__global__ __launch_bounds__(256) void nb_apply_kernel(gsm::AssetView a, gsm::EditView e, const uint32_t* __restrict__ counts, uint32_t minNeighbours,
                                                       uint32_t* __restrict__ sel, uint32_t nWords, uint32_t subtract) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    gsm::V3 pos; bool cut;
    selection_apply(export_alive(a, e, idx, blockIdx.x, pos, cut) && counts[idx] < minNeighbours, idx, lane, sel, nWords, subtract);
}

// ---- connected components of the neighbour graph (gs_renderer_edit_components / _select_islands / _grow_selection) ----------
// A lock-free union-find over the sorted positions 0 .. m - 1 of the grid above.  parent[x] <= x at every moment: a chain strictly descends, there is no
// cycle, every find ends.  Inside cc_link every access to parent[] is an agent-scope relaxed atomic and nothing depends on a load being fresh: an
// earlier value of parent[x] is a member of x's component at a position <= x, and a stale "x is a root" is caught by the compare-and-swap, which acts
// where the word lives.  No loop waits for another wave: a compare-and-swap is repeated only after another thread's hook took effect, and then from
// the value that hook left.
__device__ __forceinline__ uint32_t cc_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a root of x's tree as far as the loads show it, with path halving: every second node of the path is pointed at its grandparent
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = cc_ld(parent + x);
        if (p == x) return x;
        const uint32_t g = cc_ld(parent + p);
        if (g == p) return p;
        cc_st(parent + x, g);                                      // g <= p < x, and g shares x's root from now on whatever else is stored here
        x = g;
    }
}

// joins the trees of a and b, the larger root hooked under the smaller; a is the caller's own root so far, the result its root now
__device__ __forceinline__ uint32_t cc_union(uint32_t* parent, uint32_t a, uint32_t b) {
    b = cc_find(parent, b);
    if (b == a) return a;                                          // the common case in a dense core: nothing to do, whether a is still a root or not
    for (;;) {
        a = cc_find(parent, a);
        if (a == b) return a;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        uint32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return lo;
        a = lo;                                                    // another thread hooked hi first: go on from what it left there (seen < hi)
        b = cc_find(parent, seen);
    }
}

__global__ __launch_bounds__(256) void cc_init_kernel(uint32_t* __restrict__ parent, uint32_t m) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < m) parent[i] = i;
}

// one thread per listed splat in sorted order: every edge to an earlier sorted position (gsm::NeighbourForEach) is a union
__global__ __launch_bounds__(256) void cc_link_kernel(const unsigned long long* __restrict__ keys, const gsm::NeighbourRec* __restrict__ recs, uint32_t m, float r2,
                                                      uint32_t* parent) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    uint32_t mine = i;
    gsm::NeighbourForEach(keys, recs, m, i, r2, [&](uint32_t j) { mine = cc_union(parent, mine, j); });
}

// after the kernel boundary parent[] no longer changes: root[x] by plain loads, nothing stored into parent[]
__global__ __launch_bounds__(256) void cc_flatten_kernel(const uint32_t* __restrict__ parent, uint32_t m, uint32_t* __restrict__ root) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    uint32_t x = i, p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    root[i] = x;
}

// minIdx[root] = the smallest splat index of the component, size[root] = its splats.  A wave folds the lanes that hold one root before it touches memory
// and issues one pair of atomics per DISTINCT root it holds: one pair where all its lanes share a root -- the normal case in sorted order, and the whole
// scene can be one component -- and never a lane-by-lane queue on one word where a large component is sprinkled with small ones (section 4.18: that
// queue took 23 ms at 6.1 M splats).  The loop runs once per distinct root of the wave and waits for nobody
__global__ __launch_bounds__(256) void cc_reduce_kernel(const gsm::NeighbourRec* __restrict__ recs, const uint32_t* __restrict__ root, uint32_t m,
                                                        uint32_t* __restrict__ minIdx, uint32_t* __restrict__ size) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    if (i - lane >= m) return;                                     // the whole wave
    const bool mine = i < m;
    const uint32_t rt = mine ? root[i] : 0u;
    const uint32_t idx = mine ? recs[i].idx : 0xFFFFFFFFu;
    unsigned long long left = __ballot(mine), alone = 0ull;        // wave-uniform: the lanes whose root has not been folded yet; those that share theirs with no lane
    while (left) {
        const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1u;
        const uint32_t r0 = (uint32_t)__shfl((int)rt, (int)leader);
        const bool member = mine && rt == r0;
        const unsigned long long group = __ballot(member);
        left &= ~group;
        if ((group & (group - 1ull)) == 0ull) { alone |= group; continue; }
        uint32_t low = member ? idx : 0xFFFFFFFFu;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)low, d); low = o < low ? o : low; }
        if (lane == leader) { atomicMin(minIdx + r0, low); atomicAdd(size + r0, (uint32_t)__popcll(group)); }
    }
    if ((alone >> lane) & 1ull) { atomicMin(minIdx + rt, idx); atomicAdd(size + rt, 1u); }      // all of them in one pair of instructions
}

// by sorted position, after the kernel boundary: the listed splat's label and size under its index
__global__ __launch_bounds__(256) void cc_labels_kernel(const gsm::NeighbourRec* __restrict__ recs, const uint32_t* __restrict__ root, const uint32_t* __restrict__ minIdx,
                                                        const uint32_t* __restrict__ size, uint32_t m, uint32_t* __restrict__ labels, uint32_t* __restrict__ sizes) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint32_t idx = recs[i].idx, rt = root[i];
    labels[idx] = minIdx[rt];
    sizes[idx] = size[rt];
}

// by splat index, over buffers the listed splats have been written into and that are zero elsewhere: an alive splat that is not listed (its position is
// not finite) is a component of its own, a splat that is not alive gets 0xFFFFFFFF and 0
__global__ __launch_bounds__(256) void cc_out_kernel(gsm::AssetView a, gsm::EditView e, uint32_t* __restrict__ labels, uint32_t* __restrict__ sizes) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= a.n) return;
    gsm::V3 pos; bool cut;
    if (!export_alive(a, e, idx, blockIdx.x, pos, cut)) { labels[idx] = kNbNotAlive; sizes[idx] = 0u; }
    else if (sizes[idx] == 0u) { labels[idx] = idx; sizes[idx] = 1u; }
}

// island = alive and size < minSize; selected |= island (subtract: &= ~island): nb_apply's shape
__global__ __launch_bounds__(256) void cc_islands_apply_kernel(gsm::AssetView a, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ sizes, uint32_t minSize,
                                                               uint32_t* __restrict__ sel, uint32_t nWords, uint32_t subtract) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    selection_apply(idx < a.n && labels[idx] != kNbNotAlive && sizes[idx] < minSize, idx, lane, sel, nWords, subtract);
}

// a seed is an alive splat (index < N) whose selected bit is set: hit[label] = 1 (every writer stores the same word)
__global__ __launch_bounds__(256) void cc_seed_kernel(uint32_t n, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ sel, uint32_t* __restrict__ hit) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n) return;
    const uint32_t label = labels[idx];
    if (label != kNbNotAlive && bit_set(sel, idx)) hit[label] = 1u;
}

// after the kernel boundary: selected |= alive and hit[label]
__global__ __launch_bounds__(256) void cc_grow_apply_kernel(uint32_t n, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ hit, uint32_t* __restrict__ sel,
                                                            uint32_t nWords) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    bool grow = false;
    if (idx < n) { const uint32_t label = labels[idx]; grow = label != kNbNotAlive && hit[label] != 0u; }
    selection_apply(grow, idx, lane, sel, nWords, 0u);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// everything a call holds: freed when it returns
struct NeighbourRun {
    DevBuf<uint32_t> chunkCounts, base, list, counts;
    DevBuf<float> partial, origin;          // the per-chunk minima of the listed positions and their fold, the grid's origin
    DevBuf<gsm::NeighbourRec> recs;
    DevBuf<unsigned long long> keys, tests;
    TwoWordSort sort;                       // the cell keys as two words, and their order
    uint32_t listed = 0;
};

// what scripts/neighbour_timing.py asks of a call besides its result: events around the stages (all recorded whenever the call succeeds), the
// predicates the walk evaluated, the listed splats
enum { kNbEvCount = 0, kNbEvScan, kNbEvList, kNbEvOrigin, kNbEvSorted, kNbEvRecords, kNbEvWalk, kNbEvApply, kNbEvDone, kNbEvents };
struct NeighbourProbe { hipEvent_t ev[kNbEvents]; unsigned long long tests; uint32_t listed; };
static const char* nb_radius_refusal(float radius) {
    return (std::isfinite(radius) && radius >= 1.0e-15f && radius <= 1.0e15f) ? nullptr : "neighbours: radius must be finite and within [1e-15, 1e15]";
}

// the sorts' error words, read before anything of the renderer's is touched; the stream has drained when this returns GS_OK
static int32_t nb_sort_errors(gs_renderer* r, NeighbourRun& run) {
    hipStream_t st = r->ctx->stream;
    uint32_t err[2] = { 0u, 0u };
    GS_HIP(run.sort.enqueue_error_readback(st, err));
    GS_HIP(hipStreamSynchronize(st));
    if (err[0] | err[1]) return fail(GS_ERR_SORT_TIMEOUT, "neighbours: a bounded look-back spin expired");
    return GS_OK;
}

// steps 1 to 3 on the context's stream, r->n != 0: the list (run.listed splats; the host waits for that number), the origin, the keys, the two sorts
// and the sorted records run.recs / run.keys -- the grid the neighbour walk and the component path (below) both read.  run.listed == 0: nothing but
// the chunk counts was allocated and the stream has drained
static int32_t nb_grid(gs_renderer* r, float radius, NeighbourRun& run, const NeighbourProbe* probe) {
    gs_context* ctx = r->ctx;
    hipStream_t st = ctx->stream;
    const gsm::AssetView a = asset_view(r);
    const gsm::EditView e = edit_view(r);
    const uint32_t chunks = (r->n + 255u) / 256u;
    GS_HIP(run.chunkCounts.alloc((size_t)chunks * 4));
    GS_HIP(run.base.alloc(((size_t)chunks + 1) * 4));
    GS_HIP(mark_events(events_of(probe), kNbEvCount, kNbEvCount, st));
    GS_TRY(enqueue_alive_counts(st, a, e, true, chunks, run.chunkCounts, run.base));
    GS_HIP(mark_events(events_of(probe), kNbEvScan, kNbEvScan, st));
    uint32_t m = 0;
    GS_HIP(hipMemcpyAsync(&m, run.base.get() + chunks, 4, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    run.listed = m;
    if (m == 0u) return mark_events(events_of(probe), kNbEvList, kNbEvRecords, st) == hipSuccess ? GS_OK : fail(GS_ERR_HIP, "neighbours: an event failed");
    const uint32_t blocks = (m + 255u) / 256u;
    GS_HIP(run.list.alloc(((size_t)m + 16) * 4));
    GS_HIP(run.partial.alloc((size_t)chunks * 3 * 4));
    GS_HIP(run.origin.alloc(3 * 4));
    GS_HIP(run.recs.alloc((size_t)m * sizeof(gsm::NeighbourRec)));
    GS_HIP(run.keys.alloc((size_t)m * 8));
    GS_TRY(run.sort.alloc(ctx, m));
    const double h = gsm::NeighbourCellEdge(radius);
    const float* origin = run.origin.get();
    // 1. the list and the origin
    GS_HIP(mark_events(events_of(probe), kNbEvList, kNbEvList, st));
    GS_TRY(enqueue_alive_list(st, a, e, true, true, AliveXform{}, chunks, run.base.get(), run.list.get(), run.partial.get(), run.origin.get()));
    GS_HIP(mark_events(events_of(probe), kNbEvOrigin, kNbEvOrigin, st));
    // 2. keys and sorts
    hipLaunchKernelGGL(nb_keys_kernel, dim3(blocks), dim3(256), 0, st, a, (const uint32_t*)run.list.get(), origin, h, m, run.sort.lo.get(), run.sort.hi.get(),
                       run.sort.rank.get());
    GS_HIP(hipGetLastError());
    GS_TRY(run.sort.enqueue(ctx, m));
    GS_HIP(mark_events(events_of(probe), kNbEvSorted, kNbEvSorted, st));
    // 3. the records
    hipLaunchKernelGGL(nb_records_kernel, dim3(blocks), dim3(256), 0, st, a, (const uint32_t*)run.list.get(), (const uint32_t*)run.sort.rank.get(), origin,
                       h, m, run.recs.get(), run.keys.get());
    GS_HIP(hipGetLastError());
    GS_HIP(mark_events(events_of(probe), kNbEvRecords, kNbEvRecords, st));
    return GS_OK;
}

// steps 1 to 4 on the context's stream: run.counts[idx] = min(count(idx), limit) for the listed splats, 0 for every other index.  The stream has drained
// when this returns GS_OK; the caller drains it otherwise
static int32_t nb_enqueue(gs_renderer* r, float radius, uint32_t limit, NeighbourRun& run, const NeighbourProbe* probe) {
    const bool stats = probe != nullptr;
    hipStream_t st = r->ctx->stream;
    GS_HIP(run.counts.alloc(((size_t)r->n + 16) * 4));
    GS_HIP(hipMemsetAsync(run.counts, 0, (size_t)r->n * 4, st));
    if (stats) {
        GS_HIP(run.tests.alloc(8));
        GS_HIP(hipMemsetAsync(run.tests, 0, 8, st));
    }
    if (r->n == 0u || limit == 0u) {
        GS_HIP(mark_events(events_of(probe), kNbEvCount, kNbEvWalk, st));
        return drain(st, GS_OK, "neighbours");
    }
    GS_TRY(nb_grid(r, radius, run, probe));
    const uint32_t m = run.listed;
    if (m == 0u) {
        GS_HIP(mark_events(events_of(probe), kNbEvWalk, kNbEvWalk, st));
        return GS_OK;
    }
    // 4. the walk
    hipLaunchKernelGGL(nb_walk_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, (const unsigned long long*)run.keys.get(), (const gsm::NeighbourRec*)run.recs.get(), m,
                       radius * radius, limit, run.counts.get(), stats ? run.tests.get() : (unsigned long long*)nullptr);
    GS_HIP(hipGetLastError());
    GS_HIP(mark_events(events_of(probe), kNbEvWalk, kNbEvWalk, st));
    // the sorts' error words, before anything of the renderer's is touched
    return nb_sort_errors(r, run);
}

// the checks both entry points share, and what they do before the first launch: after everything already enqueued, the lanes' frames included -- the sorts
// assume their workgroups have the GPU to themselves, as the bake's do
static int32_t nb_begin(gs_renderer* r, float radius) {
    if (r->laneOf) return fail(GS_ERR_INVALID_ARGUMENT, "a lane holds no edit state: edit its owner");
    if (const char* why = nb_radius_refusal(radius)) return fail(GS_ERR_INVALID_ARGUMENT, why);
    GS_HIP(hipSetDevice(r->ctx->device));
    return gs_context_synchronize(r->ctx);
}

static int32_t nb_counts_impl(gs_renderer* r, float radius, uint32_t cap, uint32_t* counts_out, size_t count, NeighbourProbe* probe) {
    if (!r || !counts_out) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    if (cap == 0u) return fail(GS_ERR_INVALID_ARGUMENT, "neighbour_counts: cap must be at least 1");
    if (count != (size_t)r->n) return fail(GS_ERR_INVALID_ARGUMENT, "neighbour_counts: count must be the renderer's splat count");
    GS_TRY(nb_begin(r, radius));
    hipStream_t st = r->ctx->stream;
    NeighbourRun run;
    int32_t rc = nb_enqueue(r, radius, cap, run, probe);
    if (rc == GS_OK) {
        rc = [&]() -> int32_t {
            GS_HIP(mark_events(events_of(probe), kNbEvApply, kNbEvApply, st));
            if (r->n) hipLaunchKernelGGL(nb_counts_out_kernel, dim3((r->n + 255u) / 256u), dim3(256), 0, st, asset_view(r), edit_view(r), run.counts.get());
            GS_HIP(hipGetLastError());
            GS_HIP(mark_events(events_of(probe), kNbEvDone, kNbEvDone, st));
            if (r->n) GS_HIP(hipMemcpyAsync(counts_out, run.counts.get(), (size_t)r->n * 4, hipMemcpyDeviceToHost, st));
            if (probe) GS_HIP(hipMemcpyAsync(&probe->tests, run.tests.get(), 8, hipMemcpyDeviceToHost, st));
            return GS_OK;
        }();
    }
    if (probe) probe->listed = run.listed;
    return drain(st, rc, "neighbour_counts");
}

static int32_t nb_select_impl(gs_renderer* r, float radius, uint32_t min_neighbours, int32_t subtract, NeighbourProbe* probe) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    GS_TRY(nb_begin(r, radius));
    GS_TRY(edit_ensure(r));
    hipStream_t st = r->ctx->stream;
    NeighbourRun run;
    int32_t rc = nb_enqueue(r, radius, min_neighbours, run, probe);
    if (rc == GS_OK) {
        rc = [&]() -> int32_t {
            hist_mutated(r, true);
            GS_HIP(mark_events(events_of(probe), kNbEvApply, kNbEvApply, st));
            if (r->n && min_neighbours) {
                hipLaunchKernelGGL(nb_apply_kernel, dim3((r->n + 255u) / 256u), dim3(256), 0, st, asset_view(r), edit_view(r), (const uint32_t*)run.counts.get(),
                                   min_neighbours, r->editSelected.get(), (uint32_t)bit_words(r->n), subtract ? 1u : 0u);
                GS_HIP(hipGetLastError());
            }
            GS_HIP(mark_events(events_of(probe), kNbEvDone, kNbEvDone, st));
            if (probe) GS_HIP(hipMemcpyAsync(&probe->tests, run.tests.get(), 8, hipMemcpyDeviceToHost, st));
            return edit_selected_to_lanes(r);
        }();
    }
    if (probe) probe->listed = run.listed;
    return drain(st, rc, "select_sparse");
}

// ---- components: the host side ----------------------------------------------------------------------------------------------------------------
struct ComponentRun {
    NeighbourRun nb;
    DevBuf<uint32_t> parent, root, minIdx, size;    // by sorted position
    DevBuf<uint32_t> labels, sizes, hit;            // by splat index
};

// what scripts/islands_timing.py asks of a call: the grid's events (nb: count .. records) and the ones around the stages that follow
enum { kCcEvLinkStart = 0, kCcEvLink, kCcEvFlatten, kCcEvReduce, kCcEvApply, kCcEvDone, kCcEvents };
struct ComponentProbe { NeighbourProbe nb; hipEvent_t ev[kCcEvents]; };
// run.labels[idx] / run.sizes[idx] for every index < N as gs_renderer_edit_components defines them.  The stream has drained when this returns GS_OK;
// the caller drains it otherwise
static int32_t cc_enqueue(gs_renderer* r, float radius, ComponentRun& run, const ComponentProbe* probe) {
    hipStream_t st = r->ctx->stream;
    const NeighbourProbe* grid = probe ? &probe->nb : nullptr;
    GS_HIP(run.labels.alloc(((size_t)r->n + 16) * 4));
    GS_HIP(run.sizes.alloc(((size_t)r->n + 16) * 4));
    GS_HIP(hipMemsetAsync(run.labels, 0, (size_t)r->n * 4, st));
    GS_HIP(hipMemsetAsync(run.sizes, 0, (size_t)r->n * 4, st));
    if (r->n == 0u) {
        GS_HIP(mark_events(events_of(grid), kNbEvCount, kNbEvRecords, st));
        GS_HIP(mark_events(events_of(probe), kCcEvLinkStart, kCcEvReduce, st));
        return drain(st, GS_OK, "components");
    }
    GS_TRY(nb_grid(r, radius, run.nb, grid));
    const uint32_t m = run.nb.listed, blocks = (m + 255u) / 256u;
    if (m) {
        for (DevBuf<uint32_t>* b : { &run.parent, &run.root, &run.minIdx, &run.size }) GS_HIP(b->alloc(((size_t)m + 16) * 4));
        GS_HIP(hipMemsetAsync(run.minIdx, 0xFF, (size_t)m * 4, st));
        GS_HIP(hipMemsetAsync(run.size, 0, (size_t)m * 4, st));
        hipLaunchKernelGGL(cc_init_kernel, dim3(blocks), dim3(256), 0, st, run.parent.get(), m);
        GS_HIP(hipGetLastError());
        GS_HIP(mark_events(events_of(probe), kCcEvLinkStart, kCcEvLinkStart, st));
        hipLaunchKernelGGL(cc_link_kernel, dim3(blocks), dim3(256), 0, st, (const unsigned long long*)run.nb.keys.get(), (const gsm::NeighbourRec*)run.nb.recs.get(), m,
                           radius * radius, run.parent.get());
        GS_HIP(hipGetLastError());
        GS_HIP(mark_events(events_of(probe), kCcEvLink, kCcEvLink, st));
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks), dim3(256), 0, st, (const uint32_t*)run.parent.get(), m, run.root.get());
        GS_HIP(hipGetLastError());
        GS_HIP(mark_events(events_of(probe), kCcEvFlatten, kCcEvFlatten, st));
        hipLaunchKernelGGL(cc_reduce_kernel, dim3(blocks), dim3(256), 0, st, (const gsm::NeighbourRec*)run.nb.recs.get(), (const uint32_t*)run.root.get(), m,
                           run.minIdx.get(), run.size.get());
        hipLaunchKernelGGL(cc_labels_kernel, dim3(blocks), dim3(256), 0, st, (const gsm::NeighbourRec*)run.nb.recs.get(), (const uint32_t*)run.root.get(),
                           (const uint32_t*)run.minIdx.get(), (const uint32_t*)run.size.get(), m, run.labels.get(), run.sizes.get());
        GS_HIP(hipGetLastError());
    } else {
        GS_HIP(mark_events(events_of(probe), kCcEvLinkStart, kCcEvFlatten, st));
    }
    hipLaunchKernelGGL(cc_out_kernel, dim3((r->n + 255u) / 256u), dim3(256), 0, st, asset_view(r), edit_view(r), run.labels.get(), run.sizes.get());
    GS_HIP(hipGetLastError());
    GS_HIP(mark_events(events_of(probe), kCcEvReduce, kCcEvReduce, st));
    // the sorts' error words, before anything of the renderer's is touched
    if (m) return nb_sort_errors(r, run.nb);
    return drain(st, GS_OK, "components");
}

static int32_t cc_components_impl(gs_renderer* r, float radius, uint32_t* labels_out, uint32_t* sizes_out, size_t count, ComponentProbe* probe) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    if (!labels_out && !sizes_out && !probe) return fail(GS_ERR_INVALID_ARGUMENT, "components: labels_out and sizes_out are both null");
    if (count != (size_t)r->n) return fail(GS_ERR_INVALID_ARGUMENT, "components: count must be the renderer's splat count");
    GS_TRY(nb_begin(r, radius));
    hipStream_t st = r->ctx->stream;
    ComponentRun run;
    int32_t rc = cc_enqueue(r, radius, run, probe);
    if (rc == GS_OK) {
        rc = [&]() -> int32_t {
            GS_HIP(mark_events(events_of(probe), kCcEvApply, kCcEvDone, st));
            if (r->n && labels_out) GS_HIP(hipMemcpyAsync(labels_out, run.labels.get(), (size_t)r->n * 4, hipMemcpyDeviceToHost, st));
            if (r->n && sizes_out) GS_HIP(hipMemcpyAsync(sizes_out, run.sizes.get(), (size_t)r->n * 4, hipMemcpyDeviceToHost, st));
            return GS_OK;
        }();
    }
    if (probe) probe->nb.listed = run.nb.listed;
    return drain(st, rc, "components");
}

// grow == false: gs_renderer_edit_select_islands(min_size, subtract); grow == true: gs_renderer_edit_grow_selection
static int32_t cc_select_impl(gs_renderer* r, float radius, bool grow, uint32_t min_size, int32_t subtract, ComponentProbe* probe) {
    if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "renderer is null");
    GS_TRY(nb_begin(r, radius));
    GS_TRY(edit_ensure(r));
    hipStream_t st = r->ctx->stream;
    ComponentRun run;
    const bool work = r->n != 0u && (grow || min_size > 1u);       // a component has at least one splat: min_size 0 and 1 select nothing
    int32_t rc = (work || probe) ? cc_enqueue(r, radius, run, probe) : GS_OK;
    if (rc == GS_OK) {
        rc = [&]() -> int32_t {
            hist_mutated(r, true);
            GS_HIP(mark_events(events_of(probe), kCcEvApply, kCcEvApply, st));
            const uint32_t blocks = (r->n + 255u) / 256u, nWords = (uint32_t)bit_words(r->n);
            if (work && grow) {
                GS_HIP(run.hit.alloc(((size_t)r->n + 16) * 4));
                GS_HIP(hipMemsetAsync(run.hit, 0, (size_t)r->n * 4, st));
                hipLaunchKernelGGL(cc_seed_kernel, dim3(blocks), dim3(256), 0, st, r->n, (const uint32_t*)run.labels.get(), (const uint32_t*)r->editSelected.get(),
                                   run.hit.get());
                hipLaunchKernelGGL(cc_grow_apply_kernel, dim3(blocks), dim3(256), 0, st, r->n, (const uint32_t*)run.labels.get(), (const uint32_t*)run.hit.get(),
                                   r->editSelected.get(), nWords);
                GS_HIP(hipGetLastError());
            } else if (work) {
                hipLaunchKernelGGL(cc_islands_apply_kernel, dim3(blocks), dim3(256), 0, st, asset_view(r), (const uint32_t*)run.labels.get(),
                                   (const uint32_t*)run.sizes.get(), min_size, r->editSelected.get(), nWords, subtract ? 1u : 0u);
                GS_HIP(hipGetLastError());
            }
            GS_HIP(mark_events(events_of(probe), kCcEvDone, kCcEvDone, st));
            return edit_selected_to_lanes(r);
        }();
    }
    if (probe) probe->nb.listed = run.nb.listed;
    return drain(st, rc, grow ? "grow_selection" : "select_islands");
}

} // namespace gs

using namespace gs;

extern "C" {

int32_t gs_renderer_edit_neighbour_counts(gs_renderer* r, float radius, uint32_t cap, uint32_t* counts_out, size_t count) {
    return nb_counts_impl(r, radius, cap, counts_out, count, nullptr);
}

int32_t gs_renderer_edit_select_sparse(gs_renderer* r, float radius, uint32_t min_neighbours, int32_t subtract) {
    return nb_select_impl(r, radius, min_neighbours, subtract, nullptr);
}

// A measurement aid of scripts/neighbour_timing.py, which binds it itself: not declared in gsplat_c.h, not part of the ABI.  One whole call -- select != 0:
// gs_renderer_edit_select_sparse(radius, limit, 0), else gs_renderer_edit_neighbour_counts(radius, limit) into counts_out (N words) -- with events
// inside it: ms[0..4] = GPU milliseconds of the list + origin (count, scan, list, fold; the host's readback of the list's length between them not
// included), the keys + the two sorts, the records, the walk, the last kernel; *tests = the predicates the walk evaluated; *listed = the listed splats.
__attribute__((visibility("default"))) int32_t gs_neighbour_stage_times_for_scripts(gs_renderer* r, float radius, uint32_t limit, int32_t select, uint32_t* counts_out,
                                                                                   float ms[5], uint64_t* tests, uint32_t* listed) {
    if (!r || !ms || !tests || !listed) return fail(GS_ERR_INVALID_ARGUMENT, "null argument");
    GS_HIP(hipSetDevice(r->ctx->device));
    Event owned[kNbEvents];
    NeighbourProbe probe = {};
    for (int k = 0; k < kNbEvents; ++k) { GS_HIP(owned[k].create(hipEventDefault)); probe.ev[k] = owned[k]; }
    if (select) GS_TRY(nb_select_impl(r, radius, limit, 0, &probe));
    else GS_TRY(nb_counts_impl(r, radius, limit, counts_out, r->n, &probe));
    float head = 0.0f;
    GS_HIP(hipEventElapsedTime(&head, probe.ev[kNbEvCount], probe.ev[kNbEvScan]));
    GS_HIP(hipEventElapsedTime(&ms[0], probe.ev[kNbEvList], probe.ev[kNbEvOrigin]));
    ms[0] += head;
    GS_HIP(hipEventElapsedTime(&ms[1], probe.ev[kNbEvOrigin], probe.ev[kNbEvSorted]));
    GS_HIP(hipEventElapsedTime(&ms[2], probe.ev[kNbEvSorted], probe.ev[kNbEvRecords]));
    GS_HIP(hipEventElapsedTime(&ms[3], probe.ev[kNbEvRecords], probe.ev[kNbEvWalk]));
    GS_HIP(hipEventElapsedTime(&ms[4], probe.ev[kNbEvApply], probe.ev[kNbEvDone]));
    *tests = probe.tests;
    *listed = probe.listed;
    return GS_OK;
}

int32_t gs_renderer_edit_components(gs_renderer* r, float radius, uint32_t* labels_out, uint32_t* sizes_out, size_t count) {
    return cc_components_impl(r, radius, labels_out, sizes_out, count, nullptr);
}

int32_t gs_renderer_edit_select_islands(gs_renderer* r, float radius, uint32_t min_size, int32_t subtract) {
    return cc_select_impl(r, radius, false, min_size, subtract, nullptr);
}

int32_t gs_renderer_edit_grow_selection(gs_renderer* r, float radius) {
    return cc_select_impl(r, radius, true, 0u, 0, nullptr);
}

// A measurement aid of scripts/islands_timing.py, which binds it itself: not declared in gsplat_c.h, not part of the ABI.  One whole call -- op 0:
// gs_renderer_edit_select_islands(radius, min_size, 0); op 1: gs_renderer_edit_grow_selection(radius); op 2: the components, nothing downloaded -- with
// events inside it: ms[0..4] = GPU milliseconds of the grid build (count, scan, list, fold, keys, sorts, records; the host's readback of the list's
// length not included), cc_link, cc_flatten, the reduction with the per-index outputs, the kernels that apply; *listed = the listed splats.
__attribute__((visibility("default"))) int32_t gs_islands_stage_times_for_scripts(gs_renderer* r, float radius, int32_t op, uint32_t min_size, float ms[5], uint32_t* listed) {
    if (!r || !ms || !listed || op < 0 || op > 2) return fail(GS_ERR_INVALID_ARGUMENT, "bad argument");
    GS_HIP(hipSetDevice(r->ctx->device));
    Event ownedNb[kNbEvents], owned[kCcEvents];
    ComponentProbe probe = {};
    for (int k = 0; k < kNbEvents; ++k) { GS_HIP(ownedNb[k].create(hipEventDefault)); probe.nb.ev[k] = ownedNb[k]; }
    for (int k = 0; k < kCcEvents; ++k) { GS_HIP(owned[k].create(hipEventDefault)); probe.ev[k] = owned[k]; }
    if (op == 2) GS_TRY(cc_components_impl(r, radius, nullptr, nullptr, r->n, &probe));
    else GS_TRY(cc_select_impl(r, radius, op == 1, min_size, 0, &probe));
    float head = 0.0f;
    GS_HIP(hipEventElapsedTime(&head, probe.nb.ev[kNbEvCount], probe.nb.ev[kNbEvScan]));
    GS_HIP(hipEventElapsedTime(&ms[0], probe.nb.ev[kNbEvList], probe.nb.ev[kNbEvRecords]));
    ms[0] += head;
    GS_HIP(hipEventElapsedTime(&ms[1], probe.ev[kCcEvLinkStart], probe.ev[kCcEvLink]));
    GS_HIP(hipEventElapsedTime(&ms[2], probe.ev[kCcEvLink], probe.ev[kCcEvFlatten]));
    GS_HIP(hipEventElapsedTime(&ms[3], probe.ev[kCcEvFlatten], probe.ev[kCcEvReduce]));
    GS_HIP(hipEventElapsedTime(&ms[4], probe.ev[kCcEvApply], probe.ev[kCcEvDone]));
    *listed = probe.nb.listed;
    return GS_OK;
}

} // extern "C"
