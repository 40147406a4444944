// gs_common.h -- host-side object layouts and helpers shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <utility>
#include <vector>

#include "../../include/gsplat_c.h"
#include "gs_device_math.h"
#include "gs_handles.h"
#include "gs_params.h"

// Issue priority of the frame's latency-bound kernels (the sort passes, the key / binning / fix-up kernels, resolve): with frames in flight they share their SIMDs
// with another frame's blend, whose heaviest tiles raise their own priority (gs_raster.hip); a chain kernel's few instructions between two waits then queue behind
// the blend's.  -DGS_CHAIN_PRIO=n / -DGS_VIEW_PRIO=n: experiment builds (scripts/build_variants.py).
#ifdef GS_CHAIN_PRIO
#define GS_CHAIN_PRIORITY() __builtin_amdgcn_s_setprio(GS_CHAIN_PRIO)
#else
#define GS_CHAIN_PRIORITY() do { } while (0)
#endif
#ifdef GS_VIEW_PRIO
#define GS_VIEW_PRIORITY() __builtin_amdgcn_s_setprio(GS_VIEW_PRIO)
#else
#define GS_VIEW_PRIORITY() do { } while (0)
#endif

namespace gs {

// thread-local error detail -------------------------------------------------------------------------
void set_error_detail(const char* fmt, ...);
int32_t fail(int32_t code, const char* what);
int32_t fail_hip(hipError_t e, const char* what, const char* file, int line);

#define GS_HIP(call)                                                        \
    do {                                                                    \
        hipError_t _e = (call);                                             \
        if (_e != hipSuccess) return gs::fail_hip(_e, #call, __FILE__, __LINE__); \
    } while (0)

#define GS_TRY(call)                    \
    do {                                \
        int32_t _r = (call);            \
        if (_r != GS_OK) return _r;     \
    } while (0)

// (the compositor's tile is 16x16, 32x16 or 32x32 pixels, picked per draw: pick_tile_shape in gs_raster.hip)
constexpr int kBinThreads = 256;
constexpr int kBinItems = 8;              // sorted positions per thread: 2048 per partition (~3 rounds of partitions over the persistent grid balance better
                                          // than 1.5; 12 / 16 per thread: -5 % at C2 / C4, +6 % at C3 -- r04 calls 7, 8)
constexpr int kBinPart = kBinThreads * kBinItems;
constexpr uint32_t kBinTicketClasses = 16;
constexpr int kEvPerFrame = 28;           // hipEvents per profiled frame: 0..13 stage brackets; 14..21 / 22..27 start + stop of each depth / pair Onesweep launch

// 32-byte per-splat record consumed by the blend kernel (written by calc_view, splat-index order)
struct alignas(16) SplatRec {
    float cx, cy;           // centre, pixels (y down)
    float a1x, a1y;         // axis1, pixels
    float a2x, a2y;         // axis2, pixels
    uint32_t color0;        // f16 r << 16 | f16 g
    uint32_t color1;        // f16 b << 16 | f16 a
};
static_assert(sizeof(SplatRec) == 32, "SplatRec is 32 B");

// everything calc_view writes (all in splat-index order)
struct ViewOutputs {
    gsm::ViewData* view;            // N x 40 B SplatViewData (FULL launches only)
    SplatRec* recs;                 // N x 32 B blend records (visible splats only)
    uint2* rects;                   // N x 8 B tile rectangles
    unsigned long long* visMask;    // 1 bit per splat
};
// 1 byte per 64 splats (a wave of calc_view) behind the visibility bits: nonzero = the wave holds a visible splat -- what bin_emit tests
// first.  It lives in visMask's allocation at an offset that follows from N, so that calc_view_kernel -- whose SGPRs are full of frame
// constants: one more pointer argument spills a dozen of them to VGPR lanes, +4 % -- needs no argument for it.
__host__ __device__ inline size_t vis_mask_words(uint32_t n) { return (((size_t)n + 63) / 64 + 7) & ~(size_t)7; }
__host__ __device__ inline uint8_t* wave_flags_of(unsigned long long* visMask, uint32_t n) { return (uint8_t*)(visMask + vis_mask_words(n)); }
__host__ __device__ inline size_t vis_alloc_bytes(uint32_t n) { return vis_mask_words(n) * 8 + ((size_t)n + 63) / 64 + 64; }

// Onesweep look-back state for one sort (shared by all passes: every pass uses a fresh epoch)
struct SortState {
    DevBuf<uint32_t> altKeys;
    DevBuf<uint32_t> altVals;
    DevBuf<uint32_t> status;                // maxParts x 256 words {epoch:18 | count:14}: a partition's digit counts
    DevBuf<unsigned long long> groupAgg;    // 4 passes x maxGroups x 256 words {members:24 | sum:40}, zeroed per sort
    DevBuf<unsigned long long> groupIncl;   // maxGroups x 256 words {epoch:32 | inclusive prefix:32} through the end of a group
    uint32_t maxGroups = 0;
    uint32_t maxCount = 0;
    uint32_t maxParts = 0;
    uint32_t partMin = 8192;                // keys in the smallest partition a pass may use (gs_sort.hip: shape A, or shape C for a depth sort)
    uint32_t histCopies = 1;                // copies of SortControl::hist the producer of the current histograms spread its flushes over (hist_copies()); the passes sum them
    uint32_t epoch = 0;                     // last epoch used on `status` / `groupIncl` (18 bits, never 0)
};

// The digit histograms of a sort are accumulated by hundreds of workgroups flushing their LDS counts with global atomics; atomics on
// the same 128-byte line queue behind each other at the memory side, and 1024 bins are only 32 lines (visible_keys_kernel: 749 workgroups x
// 512 atomics = 12,000 per line, most of its 26 us).  So there are kHistReplicas copies, 4 KB apart; workgroup b adds to copy b % kHistReplicas
// and the one reader (every Onesweep workgroup, once per pass) sums the copies.
constexpr int kHistReplicas = 8;
constexpr int kHistStride = 4 * 256;      // words between two copies
// how many of the copies a sort's producer spreads its flushes over (and its Onesweep passes sum): a property of the producer's grid
uint32_t hist_copies(int producerBlocks);
// small per-sort control block (zeroed by one memset before each sort)
struct SortControl {
    uint32_t hist[kHistReplicas * kHistStride];   // digit histograms [copy][pass][digit]: raw counts
    uint32_t tickets[4][16 * 32]; // partition tickets: per pass, 16 counters (ticket classes) in separate 128-B lines
    uint32_t error;               // != 0: bounded spin expired
    uint32_t pad[3];
};

// What the host wants to know about a finished draw: stored by the blend's first workgroup (or tile_order_kernel) straight into mapped pinned host memory
struct FrameReport {
    unsigned long long pairCount;
    uint32_t binError, pairSortError, visible, tileShape;   // tileShape: log2 tile width | log2 tile height << 8 of the draw that reported
    uint32_t tieLongRuns, tieLongest;                       // GS_SORT_VISIBLE draws: VisControl::tieLongRuns / tieLongest of the draw's visible sort (else 0)
};

// ---- GS_SORT_VISIBLE (gs_vissort.hip): the depth sort of the VISIBLE splats only --------------------------------------------------
// The reference's order buffer after sorts M_1 .. M_k of a base order B is sorted lexicographically by (key under M_k, ..., key under M_1,
// rank in B).  The mode keeps B in gs_renderer::order (CSSetIndices' identity at first) and the rows of the sorts made SINCE B in
// gs_renderer::visHist, most recent first.  When the history is full the base is CONSOLIDATED: one full sort of B by the most recent row +
// the chain fix-up over all N give the reference's whole buffer, which becomes the new B (history: that one row) -- so the chain is exact at
// any length and its walk is bounded.
constexpr int kVisHistory = 128;           // sort-matrix rows (row 2) kept since the base order, most recent first; kernel argument: 2 KB
constexpr uint32_t kVisMaxBlocks = 1024;   // workgroups of visible_keys_kernel (one status word each)
constexpr uint32_t kVisTieWaveMax = 64;    // longest run of equal keys a wave ranks by counting; longer runs: the workgroup's sorting network
// small per-sort control block, two copies used alternately: each visible_keys launch zeroes the other one for the next sort
struct VisControl {
    uint32_t count;                // V: visible splats compacted this frame (the depth sort's device-side key count)
    uint32_t tieLongRuns;          // statistic: runs of more than kVisTieWaveMax equal keys the fix-up ordered (workgroup path)
    uint32_t tieLongest;           // statistic: the longest of them
    uint32_t error;                // bounded spin expired
    uint32_t pad[28];
    // visible count of block b, + 1 (0 = not published yet), one word per 64 bytes: block b polls the words of ALL blocks before it with
    // agent-scope loads, and loads of one 128-byte line queue behind each other at the memory side (749 blocks: 280,000 loads on 24 lines
    // when the words were packed)
    uint32_t status[kVisMaxBlocks * 16];
};
constexpr uint32_t kVisStatusStride = 16;
struct TieHistory { float row[kVisHistory][4]; uint32_t depth; };   // row[0] = the matrix the keys were made with; depth >= 1
// what ends the chain of a tied pair that no kept row separates: the base order
enum TieBase { TB_INDEX = 0,      // base = identity: the splat index
               TB_RANK = 1,       // base = gs_renderer::order: rank[splat] (its inverse, gs_renderer::visBaseRank)
               TB_POSITION = 2 }; // the input is a stable sort OF the base: the position inside the run (consolidation over all N)

// One pixel of a target's pick output (gs_pick_record of the C ABI): the splat whose blend took the pixel's accumulated alpha from < tau to >= tau, its view
// depth clip.w (splat_depth_kernel's bits) and the tag of the renderer that drew it; { +inf, 0xFFFFFFFF, 0, 0 } = never crossed
struct alignas(16) PickRecord { float depth; uint32_t splat, tag, zero; };
static_assert(sizeof(PickRecord) == 16 && sizeof(PickRecord) == sizeof(gs_pick_record), "PickRecord is 16 B");
constexpr uint32_t kPickNoSplat = 0xFFFFFFFFu;
// what a blend with pick output needs besides the pixels (a kernel argument; all zero for the other instantiations, which never read it)
struct PickOut {
    PickRecord* rec;        // the target's records
    float tau;              // the threshold, as the fp32 accumulator of fast mode compares it
    uint32_t tauHalfHi;     // ... and for exact mode: the smallest fp16 >= tau, << 16 (alpha is the high half of the accumulator's second dword)
    uint32_t tag;           // the drawing renderer's tag
    uint32_t noDepth;       // the target has no depth attachment: the scene-depth test of the depth-carrying form is off
};

// The two words every workgroup hits with an atomic (ticket, visible) sit in their own 128-B lines: same-address
// atomics serialise in one L2 channel (~11 ns each), so they must not also queue behind each other.
struct BinControl {
    unsigned long long pairCount; // P: total pairs this frame (may exceed capacity => overflow)
    uint32_t pairCountClamped;    // min(P, capacity), what the pair sort / ranges / blend see
    uint32_t error;
    uint32_t tieLongRuns, tieLongest;  // copied from the visible sort's VisControl by vis_count (GS_SORT_VISIBLE draws), for the report
    uint32_t pad0[26];
    uint32_t visible;
    uint32_t pad1[31];
    uint32_t tickets[16 * 32];    // kBinTicketClasses partition-ticket counters, one per 128-B line
};

} // namespace gs

struct gs_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    // second in-order queue: the depth sort of a frame (SortPoints) has no data dependence on CalcViewData, so it runs
    // here, forked from / joined to `stream` with events, and the two latency-bound kernels share the GPU
    hipStream_t aux = nullptr;
    bool overlap = false;
    // what puts another stream behind this context's: recorded on `stream` and nowhere else, and only by gs::signal_to (timing disabled)
    gs::Event evOrder;
    // GSPLAT_VIEW_GENERIC=1 at context creation: every calc_view launch takes the kernel that reads the asset's formats at run time, never one
    // with a preset's formats compiled in (gs_view.hip) -- the switch the tests use to compare the two
    bool viewGeneric = false;
    // other kernels that spin on their own workgroups may share this GPU (another process running this library, another context of this process sorting
    // at the same time): the depth sort's gather pass then hands its partitions out in dependency order instead of in XCD blocks (gs_sort.hip)
    // -1 automatic (shared iff the process holds more than one context on the device), 0 / 1 pinned by the host
    int sharedGpu = -1;
    bool counted = false;                 // this context is in the live count of its device
    int cuCount = 0;
    hipDeviceProp_t props;
    // contexts the library made itself for renderers of THIS context (gs_renderer_set_frames_in_flight's lanes): gs_context_synchronize waits for them too
    std::vector<gs_context*> children;
    bool internalLane = false;              // one of those: not in the live count of the device; its own (rare) full sorts -- consolidations -- always take the shared-GPU form
    bool sortBesideSiblings = false;        // set around a consolidation of a renderer that has lanes: they consolidate at the same frame, on their own streams
};
bool gs_shared_gpu(const gs_context* ctx);      // may another kernel that waits on its own workgroups run beside this context's? (gs_api.hip)

struct gs_asset {
    gs_context* ctx = nullptr;
    gsm::AssetView view{};
    void* blobs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // the owned allocations below, or the host's (borrowed)
    gs::DevBuf<uint8_t> ownedBlobs[5];
    uint64_t sizes[5] = {0, 0, 0, 0, 0};
    bool owned = true;
};

struct gs_sorter {
    gs_context* ctx = nullptr;
    gs::SortState st;
    gs::DevBuf<gs::SortControl> control;    // device
    gs::DevBuf<uint32_t> tmpKeys;           // for sort_host
    gs::DevBuf<uint32_t> tmpVals;
};

struct gs_target {
    gs_context* ctx = nullptr;
    uint32_t width = 0, height = 0;
    gs::DevBuf<uint16_t> rgba16f;           // W*H*4 halfs
    bool clearPending = false;              // gs_target_clear was called and nothing has touched the target since: the next
                                            // draw writes every pixel itself (no 8 B/px memset); any other reader clears first
    // optional depth attachment (the camera's depth buffer the reference draws the splats against, GaussianSplatRenderer.cs:195):
    // W*H view depths of the opaque scene; a fragment survives iff the splat's clip.w <= depth
    const float* sceneDepth = nullptr;      // device
    gs::DevBuf<float> sceneDepthOwned;      // the copy made of a host buffer (sceneDepth points at it), or null
    gs::DevBuf<unsigned long long> zbuf;    // W*H x u64 {view depth bits, ~splat index}: the depth buffer of the debug point modes (all ones = empty)
    gs::DevBuf<float> resolved;             // W*H*4 floats, lazily allocated
    gs::DevBuf<uint8_t> resolved8;
    // optional timing of gs_target_resolve: a ring of event pairs on the context's stream
    static constexpr int kResolveRing = 64;
    std::vector<gs::Event> rev;             // 2 x kResolveRing events, or empty (profiling off)
    bool profiling = false;
    int revCount = 0;                       // resolves recorded since the last read (may exceed the ring: the oldest are overwritten)
    // Lanes (gs_renderer_set_frames_in_flight) draw into the target from streams of their own: a lane's blend waits for the target's LAST USE -- the resolve
    // of the frame drawn into it before, a clear, another draw -- not for everything the context's stream holds (the other frames' blends into OTHER targets:
    // a host that alternates two targets lets consecutive blends overlap).  Recorded only while the context has lanes (gs::target_touched).
    // A host that draws every frame into the SAME target would still queue every blend behind the previous frame's composite (which reads the pixels the blend is
    // about to overwrite).  So while the context has lanes the target holds TWO pixel buffers and gs_target_clear -- after which nothing of the old content can be
    // seen -- moves on to the other one: frame k + 1 is blended into one buffer while frame k's is being resolved from the other.  rgba16f is the current one.
    gs::Event evLastUse;                    // of the current buffer (swapped with evLastUseAlt by the flip)
    bool lastUseValid = false;
    gs::DevBuf<uint16_t> rgba16fAlt;        // the other buffer, allocated at the first flip
    gs::Event evLastUseAlt;
    bool lastUseValidAlt = false;
    bool exposed = false;                   // gs_target_device_ptr handed the memory out: the host's own work on the context's stream may touch it (and the pointer stays put)
    // optional pick output (gs_target_set_pick_output): one gs::PickRecord per pixel, written by the splat blend for the pixel
    // whose accumulated alpha it takes across pickTau.  Doubled with the pixels (pickAlt follows rgba16fAlt through gs_target_clear's flip).
    gs::DevBuf<gs::PickRecord> pick;        // W*H records, or null (pick output off)
    gs::DevBuf<gs::PickRecord> pickAlt;     // the other buffer's, allocated at the first flip
    float pickTau = 0.5f;                   // 0 < tau <= 1
};

// A screen mask (gs_mask_*; gs_mask.hip): one bit per pixel, H rows of ceil(W/32) words, row 0 = top.  The outline or stroke of a
// drawing call travels through a pinned shadow copy, as a renderer's cutouts do: the caller's array is only read during the call and the upload is
// stream-ordered behind the kernel that still reads the previous one.
struct gs_mask {
    gs_context* ctx = nullptr;
    uint32_t width = 0, height = 0, rowWords = 0;
    gs::DevBuf<uint32_t> words;             // height x rowWords
    gs::DevBuf<float> xy;                   // the current outline / stroke, xyCap points
    gs::PinnedBuf<float> xyHost;
    gs::Event xyCopied;
    bool xyCopyPending = false;
    uint32_t xyCap = 0;
    gs::PinnedBuf<uint32_t> wordsHost;      // gs_mask_upload's shadow of the same kind, made by the first upload: height x rowWords
    gs::Event wordsCopied;
    bool wordsCopyPending = false;
};

namespace gs {
// The plain values a host sets on a renderer and expects to keep.  One copy, the owner's: a lane reads its owner's through gs::settings(), a resize
// copies the struct.  renderMode and pointDisplaySize are safe to read from the owner too: lanes draw only while the owner's mode is GS_RENDER_SPLATS
// (lanes_on, gs_api.hip), which is a lane's own default.
struct RendererSettings {
    int blendMode = 0;
    int renderMode = 0;                     // gs_render_mode (GaussianSplatRenderer.RenderMode, :126-131)
    float pointDisplaySize = 3.0f;          // m_PointDisplaySize
    bool alwaysWriteView = false;           // gs_renderer_set_view_buffer_mode(1): write the view buffer every frame like the reference
    bool kernelTiming = false;              // gs_renderer_set_kernel_timing: Onesweep launches carry their own start / stop events
    uint32_t tileOverrideWL = 0, tileOverrideHL = 0;   // gs_renderer_set_tile_shape: log2 tile width / height, 0 = automatic
    int visHistLimit = kVisHistory;         // rows kept before the base is consolidated (gs_renderer_set_sort_history_limit; GSPLAT_VIS_HISTORY)
    bool selectionHighlight = false;        // gs_renderer_set_selection_highlight: splat frames draw the selection as the reference does (gs::edit_view)
    uint32_t pickTag = 0;                   // gs_renderer_set_pick_tag: what this renderer's draws write into the pick records they own
    bool rigidTransforms = false;           // gs_renderer_edit_set_rigid_transforms: rotate / scale of the selection also turn orientation and SH, scale splat sizes
};

// ---- the edit history (gs_renderer_edit_history_enable; gs_edit.hip) ----
// One entry = what one gs_renderer_edit_checkpoint captured: the two bit buffers whole, and the records of the k splats selected then (index < N, in
// index order) with their index list.  Undo / redo SWAP an entry's contents with the renderer's state, so an entry is always "the other state".
struct EditHistEntry {
    uint32_t what = 0;                      // GS_HIST_* actually captured (gates applied, GS_HIST_TRANSFORM resolved)
    uint32_t k = 0;                         // journalled splats
    uint64_t bytes = 0;                     // device bytes of the buffers below
    uint64_t selGen = 0;                    // EditHistory::selGen at the checkpoint: still equal = the selection is the one the records were gathered for
    DevBuf<uint32_t> sel, del, idx;         // ceil(N/32) words each / k indices
    DevBuf<uint8_t> pos, other, sh;         // k x 12 / 16 / 192 bytes
};
struct EditHistory {
    bool enabled = false;
    uint64_t maxBytes = 0, bytes = 0;       // the budget; bytes of undo + redo
    std::vector<EditHistEntry> undo, redo;  // back() = the entry the next undo / redo applies
    // entries dropped by a call that may not wait (a mutating edit call drops the redo side): an undo's swap may still be reading them on the stream, so they
    // are only released where the stream is known to have drained -- the next checkpoint, clear, disable, or the renderer's end
    std::vector<EditHistEntry> dead;
    uint32_t evicted = 0, uncovered = 0;
    uint64_t selGen = 0;                    // bumped by every call that may change the selection
    DevBuf<uint32_t> counts, base;          // per 256-splat block: selected splats, and their exclusive prefix (+ the total); made by enable
};
} // namespace gs

// A plain-value setting goes into gs::RendererSettings, and nothing else needs doing.
// A setting that owns memory is forwarded to the lanes by its setter and re-applied in resize_build() (gs_copy.hip).
// A 1-bit-per-splat buffer that the device writes on the owner and a lane reads from a copy of its own (deletedBits, laneSelected) follows the owner's
// through gs::mirror_bits_to_lanes (gs_edit.hip).  None of this needs an event here: one stream is put behind another's with gs::signal_to.
// No member may point into the struct: gs_renderer_edit_set_splat_count builds a second gs_renderer of the new N and std::swap()s the two WHOLE structs.
struct gs_renderer {
    gs_context* ctx = nullptr;
    gs_asset* asset = nullptr;
    uint32_t n = 0;
    // reference buffers (GaussianSplatRenderer.cs:407,431-432)
    gs::DevBuf<gsm::ViewData> view;         // m_GpuView
    gs::DevBuf<uint32_t> keyBySplat;        // N x u32: the frame's sort key of every splat, in splat-index order
    gs::DevBuf<uint32_t> distances;         // m_GpuSortDistances
    gs::DevBuf<uint32_t> order;             // m_GpuSortKeys (_OrderBuffer)
    gs::SortState depthSort;
    gs::DevBuf<gs::SortControl> depthControl;  // two blocks, used alternately: each sort zeroes the other one for the next
    int depthControlIdx = 0;                   // the block the last / current sort uses
    // compositor buffers
    gs::DevBuf<gs::SplatRec> recs;          // N x 32 B, indexed by splat (written by calc_view)
    gs::DevBuf<gsm::BoxRec> boxRecs;        // N x 64 B, debug box modes only (allocated on first use)
    gs::DevBuf<uint32_t> chunkOrder;        // identity order of the chunks (DebugChunkBounds draws them in index order)
    gs::DevBuf<float> recW;                 // N x 4 B: clip.w of the visible splats, filled by the draw only when the target has a depth attachment or pick output
    gs::DevBuf<uint2> rects;                // N x 8 B: x = x0 | y0 << 16, y = (x1 + 1) | (y1 + 1) << 16, pixels (0 = culled): gsm::PackPixelRect
    gs::DevBuf<unsigned long long> visMask; // ceil(N/64) x 8 B: bit s = splat s reaches at least one tile (written by calc_view); + ceil(N/64) B per-wave flags (wave_flags_of)
    // edit state read by calc_view (m_GpuEditDeleted / m_GpuEditCutouts, GaussianSplatRenderer.cs:266,269)
    gs::DevBuf<uint32_t> deletedBits;       // ceil(N/32) words, or null (_SplatBitsValid = 0)
    gs::DevBuf<uint32_t> cutouts;           // GS_MAX_CUTOUTS x 17 dwords
    uint32_t cutoutCount = 0;
    gs::PinnedBuf<uint8_t> cutoutsHost;     // pinned shadow of the last uploaded set
    uint32_t cutoutsHostCount = 0;
    gs::Event cutoutsCopied;
    bool cutoutsCopyPending = false;
    // selection state of the edit kernels (gs_edit.hip; EnsureEditingBuffers, GaussianSplatRenderer.cs:767-786), made at the first edit call; the deleted
    // buffer of that function is deletedBits above.  On the owning renderer only: a lane holds nothing but its copy of deletedBits.
    gs::DevBuf<uint32_t> editSelected;      // m_GpuEditSelected: ceil(N/32) words
    gs::DevBuf<uint32_t> editSelectedMouseDown;  // m_GpuEditSelectedMouseDown
    gs::DevBuf<uint32_t> editCountsBounds;  // m_GpuEditCountsBounds: 3 counts + 6 sortable uints
    // the selection highlight (RendererSettings::selectionHighlight): what calc_view reads is editSelected itself on the owner and, on a lane, its own copy,
    // which follows every change of the selection exactly as a lane's deletedBits follow a delete (gs::edit_selected_to_lanes)
    gs::DevBuf<uint32_t> laneSelected;      // (on a lane) its copy of the owner's editSelected, made while the highlight is on; else null
    bool viewHighlight = false;             // the last calc_view ran with the selected bits: the records carry its marks and the draw launches the highlight blend
    // The renderer's own, writable copy of the two blobs the transform kernels write (CSTranslateSelection / CSRotateSelection / CSScaleSelection): made by
    // the first transform whose format gate can pass, null until then (gs::asset_view).  The asset itself -- shared between contexts, lanes and replicas --
    // is never written; lanes read their owner's copies in place.
    // ... and of the two the merge writes as well (CSCopySplats; gs_copy.hip): made by the first copy INTO this renderer, or -- all four -- by a resize.
    gs::DevBuf<uint8_t> priv[4];            // 0 m_GpuPosData of this renderer, 1 m_GpuOtherData, 2 m_GpuColorData (2048 x CalcTextureSize(N).h texels of four fp32), 3 m_GpuSHData
    uint64_t privBytes[4] = {0, 0, 0, 0};   // bytes of each private blob while it exists: gs::blob_bytes
    gs::DevBuf<uint8_t> editPosMouseDown;   // m_GpuEditPosMouseDown: made only when the position gate can pass
    gs::DevBuf<uint8_t> editOtherMouseDown; // m_GpuEditOtherMouseDown: ... the rotation gate
    gs::DevBuf<uint8_t> editSHMouseDown;    // gs_renderer_edit_store_sh_mouse_down: N x 192 B, made only when the rotation gate can pass (read by the rigid rotate)
    bool editPosStored = false, editOtherStored = false, editSHStored = false;   // the three mouse-down store calls have run since the last release / resize
    bool movedSinceView = false;            // the splats were moved after the last calc_view: lastParams no longer reproduce the view buffer
    float viewW = 0.f, viewH = 0.f, viewNear = 0.f, viewFar = 0.f;   // what the last calc_view was run with
    bool viewValid = false;
    bool viewMaterialised = false;          // the N x 40 B view buffer holds the last calc_view's records (written on demand)
    gs_frame_params lastParams;             // of the last gs_renderer_calc_view (for the on-demand FULL launch)
    gs::DevBuf<uint32_t> pairKeys;          // tile ids
    gs::DevBuf<uint32_t> pairVals;          // sorted positions
    gs::SortState pairSort;
    uint64_t pairCapacity = 0;
    // per-frame zero arena: [BinControl | SortControl(pair) | binStatus | tileStart | tileEnd]
    gs::DevBuf<uint8_t> frameArena;         // two copies, used alternately: each draw zeroes the other one for the next
    int arenaIdx = 0;
    size_t frameArenaBytes = 0;             // of one copy
    size_t offBinStatus = 0, offBinGroupAgg = 0, offBinGroupBase = 0, offTileStart = 0, offTileEnd = 0, offPairControl = 0;
    uint32_t arenaTiles = 0;                // tiles the arena was sized for
    gs::DevBuf<uint32_t> tileCost;          // 2 x arenaTiles x u32: batches each tile walked -- a draw writes copy costIdx and reads (for scheduling) the other
    int costIdx = 0;
    uint32_t costTiles[2] = {0, 0};         // tile count of the draw that wrote each copy (0 = none): a schedule can be made from it for the same count only
    uint32_t costShape[2] = {0, 0};         // ... and the same tile shape (log2 w | log2 h << 8)
    uint32_t lastTileWL = 0, lastTileHL = 0;           // of the last draw (0 x 0: nothing drawn yet)
    bool adaptTall = false;                            // automatic shape: 32x32 instead of 32x16 (large splats; adapt_tile_shape)
    gs::DevBuf<uint32_t> tileOrderBuf;      // arenaTiles x u32: the blend's tile schedule of the draw in flight
    uint32_t binParts = 0;
    gs::RendererSettings set;               // read through gs::settings(): a lane's own copy is never looked at
    // profiling: a ring of per-frame hipEvent sets (slot advances at the end of gs_renderer_draw)
    bool profiling = false;
    std::vector<gs::Event> ev;              // profCapacity x kEvPerFrame
    std::vector<uint8_t> evValid;
    int profCapacity = 0, profCur = 0, profCompleted = 0;
    // host copy of last frame's control (pinned), read lazily
    gs::PinnedBuf<gs::FrameReport> hostReport; // pinned + mapped: written by the last small kernel of a draw (no copy launch) through hostReport.device()
    gs::Event evSortDone;                   // aux -> main join (timing disabled)
    gs::Event evOrderFree;                  // main -> aux fork: the last operation of the main queue that reads or writes order[]
    bool distancesStale = false;      // the last depth pass skipped the sorted-key write: gs_renderer_download_distances gathers them
    bool sortPending = false;               // a sort on ctx->aux has not been joined into ctx->stream yet
    uint32_t lastTilesX = 0, lastTilesY = 0, lastPairPasses = 0, lastDepthPasses = 4;
    bool frameInFlight = false;
    float resolveMs = 0.f;
    // a truncated draw, latched when the next draw notices it (maybe_grow_pairs) and handed out once by gs_renderer_poll_pairs: the
    // report itself is overwritten and the capacity grown before a pipelined host gets to poll
    unsigned long long truncPairs = 0, truncCapacity = 0;
    // ---- GS_SORT_VISIBLE (gs_renderer_set_sort_mode; gs_vissort.hip) ----
    int sortMode = 0;                       // gs_sort_mode
    // order[] is the BASE of the visible-only sort: the reference's order buffer as of the last full sort / consolidation / upload / reset;
    // the reference's buffer NOW = order[] stably sorted by visHist, oldest first
    bool visBaseIdentity = true;            // order[] is CSSetIndices' identity (rank[s] = s: no rank array needed)
    bool visRankValid = false;              // visBaseRank holds the inverse of order[]
    gs::DevBuf<uint32_t> visBaseRank;       // N x u32, allocated when first needed
    bool visOrderValid = false;             // visIdx holds the sorted visible order of the last calc_view under the current history
    bool visDrawn = false;                  // the draw in flight was binned from visIdx
    float visHist[gs::kVisHistory][4];      // sort-matrix rows (m[8..11]) since the base, most recent first, no row twice
    int visHistDepth = 0;
    unsigned long long visConsolidations = 0;
    gs::DevBuf<uint32_t> visKeys;           // N x u32 each, allocated on first use: compacted (key, splat index) of the visible splats, sorted in place
    gs::DevBuf<uint32_t> visIdx;
    gs::DevBuf<uint32_t> visRectX;          // N x u32 each: the pixel rectangle (rects[visIdx[i]].x / .y) by SORTED position (vis_offsets_kernel's gather)
    gs::DevBuf<uint32_t> visRectY;
    gs::DevBuf<uint32_t> visPairOffset;     // N x u32: first (tile, splat) pair slot of every sorted position (vis_offsets_kernel)
    gs::DevBuf<uint32_t> visChunkStart;     // per chunk of 1024 pair slots: the sorted position its first slot belongs to; sized by the pair capacity
    uint32_t visChunkCap = 0;
    gs::DevBuf<gs::VisControl> visControl;  // two blocks, used alternately
    int visControlIdx = 0;
    // ---- frames in flight inside the library (gs_renderer_set_frames_in_flight; gs_api.hip) ----
    // lanes: renderers on contexts (= streams) of their own over this renderer's asset, owned by it; while GS_SORT_VISIBLE draws splats every gs_renderer_calc_view
    // moves on to the next lane and the frame's kernels run there -- one frame's latency-bound chain under another's blend.  Empty: one frame at a time, on ctx.
    std::vector<gs_renderer*> lanes;
    int laneCur = -1;                       // the lane of the frame in progress (-1: none yet)
    gs_renderer* laneOf = nullptr;          // a lane's owner
    // ---- the edit history (gs_renderer_edit_history_enable; gs_edit.hip) ----
    gs::EditHistory hist;                   // undo / redo of the edit state: off (and empty) unless gs_renderer_edit_history_enable was called; the owner's only
};

namespace gs {
// ctx->evOrder is recorded on ctx->stream and nowhere else: the one rule that keeps re-recording it harmless
// (everything enqueued on `waiter` from here on starts after everything `from`'s stream holds now)
inline int32_t signal_to(gs_context* from, hipStream_t waiter) {
    GS_HIP(order_after(waiter, from->stream, from->evOrder));
    return GS_OK;
}
// the renderer itself, or its owner if it is a lane
inline gs_renderer* owner_of(gs_renderer* r) { return r->laneOf ? r->laneOf : r; }
inline const gs_renderer* owner_of(const gs_renderer* r) { return r->laneOf ? r->laneOf : r; }
void prof_record(gs_renderer* r, int k, hipStream_t st = nullptr);   // gs_api.hip: record event k of the current profiling slot (on st, default ctx->stream)
int32_t target_touched(gs_target* t, hipStream_t st);   // gs_raster.hip: the last operation on the target's memory has just been enqueued on st
int32_t join_sort(gs_renderer* r);          // make ctx->stream wait for a sort still running on ctx->aux
int32_t mark_order_use(gs_renderer* r);     // the main queue has just been given work that reads / writes order[]: the next sort waits for it
void prof_end_frame(gs_renderer* r);
// sort entry points (gs_sort.hip)
int32_t sort_state_create(gs_context* ctx, SortState& st, uint32_t maxCount, bool smallPartitions = false);
// keys of all splats in index order (CSCalcDistances' arithmetic) + the four digit histograms; the gather through the
// previous order is done by the first sort pass (enqueue_sort_passes with gatherKeys)
int32_t enqueue_sort_keys(gs_context* ctx, hipStream_t st, const gsm::AssetView& a, const float* matSort, uint32_t* keyBySplat,
                          SortControl* control, SortControl* nextControl, uint32_t n, SortState& sort);
uint32_t sort_group_words(const SortState& st, uint32_t nUpper, int passes);   // 8-byte words of SortState::groupAgg a sort of nUpper keys uses (to be zeroed before the passes)
int32_t enqueue_histogram(gs_context* ctx, hipStream_t st, const uint32_t* keys, uint32_t n, const uint32_t* nPtr, int passes, uint32_t lastMask,
                          SortControl* control, SortState& sort);
// `passes` Onesweep passes.  The raw digit histograms must already be in control->hist and sort.groupAgg zeroed.  Result ends in (keys, vals) when
// passes is even, otherwise it is copied back.
// profR/evFirst: optional hipEvent slots (evFirst = just before the first Onesweep launch, evFirst + 1 = after the last)
// bitsPerPass: digit width (6..8; the histograms in control->hist must have been taken with the same width).
// gatherKeys != null (8-bit passes, an even number of them): the first pass reads its keys as gatherKeys[vals[i]].
int32_t enqueue_sort_passes(gs_context* ctx, hipStream_t stream, SortState& st, SortControl* control, uint32_t* keys, uint32_t* vals,
                            uint32_t nUpper, const uint32_t* nPtr, int passes, uint32_t lastMask = 255u,
                            gs_renderer* profR = nullptr, int evFirst = -1, int bitsPerPass = 8, const uint32_t* gatherKeys = nullptr, bool skipLastKeys = false,
                            uint32_t expected = 0);   // expected: the key count to tune the pass shape for when nUpper is only a bound (0 = nUpper)
int32_t enqueue_gather_keys(gs_context* ctx, const uint32_t* keyBySplat, const uint32_t* order, uint32_t* out, uint32_t n);
constexpr uint32_t kSortMaxCount = 1u << 30;   // 32-bit byte offsets inside the sort kernels
int32_t enqueue_set_indices(gs_context* ctx, uint32_t* order, uint32_t n);
// visible-only depth sort (gs_vissort.hip)
inline bool vis_active(const gs_renderer* r) { return r->sortMode == GS_SORT_VISIBLE; }
int32_t vis_alloc(gs_renderer* r);                                   // visKeys / visIdx / visControl, on first use
int32_t vis_push_matrix(gs_renderer* r, const float* matrixSort);    // gs_renderer_sort in visible mode: history bookkeeping (+ a consolidation when the history is full)
// order[] := the reference's whole order buffer now (one full sort of the base by the most recent row + the chain fix-up over N); the history shrinks
// to that row.  Also what hands the buffer to GS_SORT_FULL / gs_renderer_download_order.  (gs_api.hip)
int32_t vis_consolidate(gs_renderer* r);
// the chain fix-up over a stable sort of the base (keys = sorted keys, idx = the order), rows 1.. of the history
int32_t enqueue_tie_fix_full(gs_renderer* r, const uint32_t* keys, uint32_t* idx);
// visMask (calc_view's or box_setup's visibility bits) -> r->visIdx = the visible items in the reference's depth order, count in visControl
int32_t enqueue_visible_sort(gs_renderer* r);
inline const VisControl* vis_control(const gs_renderer* r) { return r->visControl + r->visControlIdx; }
// view (gs_view.hip)
int32_t enqueue_calc_view(gs_context* ctx, const gsm::AssetView& a, const gs_frame_params* p, const gsm::EditView& e, const ViewOutputs& out, bool full);
ViewOutputs view_outputs(gs_renderer* r);
// raster (gs_raster.hip)
int32_t renderer_alloc_raster(gs_renderer* r);
int32_t enqueue_draw(gs_renderer* r, const gs_frame_params* p, gs_target* rt);
void auto_tile_shape(uint32_t width, uint32_t height, uint32_t& wl, uint32_t& hl);                       // the automatic tile shape for a target size
void pick_tile_shape(const gs_renderer* r, uint32_t width, uint32_t height, uint32_t& wl, uint32_t& hl);  // ... or the renderer's override
int32_t enqueue_debug_points(gs_renderer* r, const gs_frame_params* p, gs_target* rt);   // RenderMode.DebugPoints / DebugPointIndices
int32_t enqueue_debug_boxes(gs_renderer* r, const gs_frame_params* p, gs_target* rt, bool chunks);   // RenderMode.DebugBoxes / DebugChunkBounds
int32_t enqueue_resolve(gs_target* t, const float bg[4], bool want8);
int32_t flush_clear(gs_target* t);          // perform a pending gs_target_clear now
int32_t enqueue_pick_fill(gs_target* t, PickRecord* rec);   // every record of a target's pick buffer := "none", on the context's stream
// edit (gs_edit.hip)
void edit_free(gs_renderer* r);             // the selection buffers and the mouse-down copies (not deletedBits, not the private blobs)
int32_t edit_ensure(gs_renderer* r);        // EnsureEditingBuffers: the zeroed selection buffers, made once
int32_t edit_make_private(gs_renderer* r, int k);   // copy-on-write of blob k (0 pos, 1 other, 2 color, 3 sh) on the context's stream
int32_t edit_deleted_to_lanes(gs_renderer* r);      // the lanes' copies of the deleted bits follow the owner's, stream-ordered (mirror_bits_to_lanes)
int32_t edit_selected_to_lanes(gs_renderer* r);     // ... and, while the highlight is on, their copies of the selection
int32_t ensure_deleted_bits(gs_renderer* r, hipStream_t st);   // a renderer without a deleted buffer gets one, zero-filled on st
// the edit history's hooks (host bookkeeping only, nothing is launched; all of them do nothing while the history is off):
void hist_mutated(gs_renderer* r, bool selection);   // a call is about to change journalable state: the redo side goes; selection: the selection may change
void hist_transform(gs_renderer* r);                 // ... a transform: hist_mutated + the uncovered_transforms count
int32_t hist_clear(gs_renderer* r);                  // every entry released (waits for the stream first)
void hist_forget(gs_renderer* r);                    // ... without waiting: every entry dropped now, its memory released at the next call of the history's that waits
void hist_carry(gs_renderer* to, const gs_renderer* from);   // a resize: the switch, the budget and the counters move on to the new state, the entries do not
// gs_compact.hip: base[i] = counts[0] + .. + counts[i - 1] for i in [0, n] on st (export_scan_kernel, one workgroup)
int32_t enqueue_scan(hipStream_t st, const uint32_t* counts, uint32_t* base, uint32_t n);
// what brackets a kernel that rewrites positions (the transforms, the merge): ordering against sorts, GS_SORT_VISIBLE's history and the lanes
int32_t edit_before_move(gs_renderer* r);
int32_t edit_after_move(gs_renderer* r);
// gs_api.hip: a renderer of n splats over `asset` (n != the asset's: a lane of a resized renderer, or the new state of a resize itself)
int32_t renderer_create_n(gs_context* ctx, gs_asset* asset, uint32_t n, gs_renderer** out);
// gs_api.hip: order[] stops being the visible-only mode's base / the lanes take over the owner's order
void vis_base_changed(gs_renderer* r, bool identity);
int32_t lanes_resync(gs_renderer* r);
// The asset as THIS renderer sees it: the asset's view with the blobs replaced by the renderer's private copies where they exist and N the renderer's
// (a resize changes it).  A lane sees what its owner sees.  Every launch that reads the blobs takes its view from here.
inline gsm::AssetView asset_view(const gs_renderer* r) {
    const gs_renderer* o = owner_of(r);
    gsm::AssetView v = r->asset->view;
    if (o->priv[0]) v.pos = o->priv[0];
    if (o->priv[1]) v.other = o->priv[1];
    if (o->priv[2]) v.color = o->priv[2];
    if (o->priv[3]) v.sh = o->priv[3];
    v.n = o->n;
    return v;
}
// bytes of blob k (0 pos, 1 other, 2 color, 3 sh) as this renderer sees it
inline uint64_t blob_bytes(const gs_renderer* r, int k) {
    const gs_renderer* o = owner_of(r);
    return o->priv[k] ? o->privBytes[k] : r->asset->sizes[k];
}
inline const uint8_t* blob_ptr(const gs_renderer* r, int k) {
    const gsm::AssetView a = asset_view(r);
    return k == 0 ? a.pos : (k == 1 ? a.other : (k == 2 ? a.color : a.sh));
}
// the settings this renderer draws with: its own, or its owner's if it is a lane
inline const RendererSettings& settings(const gs_renderer* r) { return owner_of(r)->set; }
// the edit state calc_view and the edit kernels consult, of THIS renderer: a lane reads its own copy of the deleted bits -- and of the selected bits,
// which are there only for a splat frame of a renderer whose highlight is on and whose edit buffers exist (_SplatBitsValid, GaussianSplatRenderer.cs:518-520)
inline gsm::EditView edit_view(const gs_renderer* r) {
    gsm::EditView e;
    e.deletedBits = r->deletedBits; e.cutouts = r->cutouts; e.cutoutCount = r->cutoutCount;
    const RendererSettings& s = settings(r);
    if (s.selectionHighlight && s.renderMode == GS_RENDER_SPLATS) e.selectedBits = r->laneOf ? r->laneSelected.get() : r->editSelected.get();
    return e;
}
inline size_t bit_words(uint32_t n) { return ((size_t)n + 31) / 32; }   // words of a 1-bit-per-splat buffer
// ---- the compaction of the alive splats and the sort of a two-word key (gs_compact.hip): what the export, the bake, the imports and the neighbour grid share ----
// counts[c] = alive splats of chunk c (export_alive, gs_block.h; finiteOnly: and every component of the position finite -- the neighbour grid's list),
// base[0 .. chunks] = their exclusive prefix and the total.  enqueue_alive_chunk_counts is its first launch alone (enqueue_scan, above, the second)
int32_t enqueue_alive_counts(hipStream_t st, const gsm::AssetView& a, const gsm::EditView& e, bool finiteOnly, uint32_t chunks, uint32_t* counts, uint32_t* base);
int32_t enqueue_alive_chunk_counts(hipStream_t st, const gsm::AssetView& a, const gsm::EditView& e, bool finiteOnly, uint32_t chunks, uint32_t* counts);
// after enqueue_alive_counts with the same finiteOnly: alive[j] = source index of the j-th such splat (total + 16 words), partial = chunks x 6 floats,
// bounds[0..2 / 3..5] = min / max of their positions -- as stored, or with X.through != 0 moved through the rows 0..2 of X.m first (what a baked export
// does to them).  minOnly: the minima alone -- partial = chunks x 3 floats, bounds = 3 floats; nothing is reduced, stored or folded for the maxima
struct AliveXform { uint32_t through = 0; float m[12] = {}; };
int32_t enqueue_alive_list(hipStream_t st, const gsm::AssetView& a, const gsm::EditView& e, bool finiteOnly, bool minOnly, const AliveXform& X, uint32_t chunks,
                           const uint32_t* base, uint32_t* alive, float* partial, float* bounds);
// bounds[0..2 / 3..5] = min / max over `count` x 6 partials, or (minOnly) bounds[0..2] = min over `count` x 3 (one workgroup; min / max: exact in any order)
int32_t enqueue_bounds_fold(hipStream_t st, const float* partial, uint32_t count, float* bounds, bool minOnly);
// The stable sort of m 63-bit keys given as two words: the caller fills lo, hi and rank = identity; enqueue() sorts the low word over 32 bits with rank as
// the payload, gathers the high word through it into hi2 and sorts that over 31 bits: rank is then the (key, index) order.  Each of the two sorts has a
// control block, and so an error word, of its own: enqueue_histogram zeroes the block it is given
struct TwoWordSort {
    DevBuf<uint32_t> lo, hi, hi2, rank;
    SortState sort;
    DevBuf<SortControl> control;            // two blocks
    int32_t alloc(gs_context* ctx, uint32_t m);
    int32_t enqueue(gs_context* ctx, uint32_t m);                  // on ctx->stream
    // err[0 .. 1] := the two sorts' error words (!= 0: a bounded look-back spin expired), valid after the caller's next synchronisation of st
    hipError_t enqueue_error_readback(hipStream_t st, uint32_t err[2]) const;
};
// records ev[from .. to] on st; a null ev (no probe) does nothing.  events_of: the events of a timing script's probe, which may be null
template <class Probe> inline const hipEvent_t* events_of(const Probe* probe) { return probe ? probe->ev : nullptr; }
inline hipError_t mark_events(const hipEvent_t* ev, int from, int to, hipStream_t st) {
    for (int k = from; ev && k <= to; ++k) { const hipError_t e = hipEventRecord(ev[k], st); if (e != hipSuccess) return e; }
    return hipSuccess;
}
// how a call that enqueued on st ends, whatever rc it got so far: nothing in flight outlives the call's buffers, and the stream's own error is reported
// only if nothing failed before -- with the caller's file and line, as GS_HIP reports its own
inline int32_t drain(hipStream_t st, int32_t rc, const char* what, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    const hipError_t hs = hipStreamSynchronize(st);
    return rc == GS_OK && hs != hipSuccess ? fail_hip(hs, what, file, line) : rc;
}
// the Cluster* SH palette on device pointers (gs_cluster.hip): what one run of the Lloyd loop holds besides the points, the means and the indices
struct ClusterRun {
    DevBuf<float> sub;                      // the stride-sampled training subset (only when n > 200,000)
    DevBuf<double> c2;
    DevBuf<uint32_t> keys, pts, range;      // (cluster, point) pairs of the subset and, per cluster, where its run of the sorted pairs starts / ends
    SortState sort;
    DevBuf<SortControl> control;            // zeroed before every sort, its error word included:
    DevBuf<uint32_t> error;                 // != 0 after the loop: the look-back spin of ANY of its sorts expired (kept across the passes)
};
int32_t cluster_run_alloc(gs_context* ctx, ClusterRun& run, uint64_t n, uint32_t K);
int32_t enqueue_cluster_shs(gs_context* ctx, ClusterRun& run, const float* x, uint64_t n, uint32_t K, float* means, uint32_t* index, const hipEvent_t* ev);
} // namespace gs
