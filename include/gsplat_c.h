/* gsplat_c.h -- C-ABI of libgsplat_hip.so: the MI355X (gfx950) splat render hot path.
 *
 * The reference (aras-p/UnityGaussianSplatting) has no FFI: its "operator boundary" is Unity's
 * ComputeShader / CommandBuffer / GraphicsBuffer API, driven from C# in
 *   package/Runtime/GaussianSplatRenderer.cs  (buffers :373-445, constants :487-510,597-606,624-631,
 *                                              dispatch order :108-211, :579-639)
 *   package/Runtime/GpuSorting.cs             (Args / SupportResources / Dispatch :32-87,142-198)
 * This header is that binding contract restated as plain C: one entry point per thing the C# records
 * into its CommandBuffer.  A .NET host binds it with [DllImport("gsplat_hip")] (see INTEGRATION.md and
 * unitygaussiansplatting_amd/dotnet/GaussianSplatNative.cs); the tests bind it with ctypes.
 *
 * Conventions
 *  - every function returns int32: 0 = GS_OK, < 0 = gs_error.  Nothing throws, nothing calls back.
 *  - handles are opaque.  One gs_context = one GPU + one HIP stream.  All work of a context is enqueued
 *    on that stream in call order (like one Unity CommandBuffer; see gs_context_set_overlap for the one opt-in exception,
 *    which is not observable through this API); calls on one context are NOT thread
 *    safe (Unity records on its single render thread); different contexts are independent.
 *  - host pointers passed in are only read during the call (data is copied); the caller keeps ownership.
 *  - matrices are float[16], row-major m[row*4+col], column vectors (HLSL mul(M, v) with Unity's layout).
 *  - the *_download / *_synchronize functions block; everything else is asynchronous.
 */
#ifndef GSPLAT_C_H
#define GSPLAT_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 9

typedef enum gs_error {
    GS_OK = 0,
    GS_ERR_INVALID_ARGUMENT = -1,   /* null handle, bad size, bad enum (C#: ArgumentOutOfRangeException, GaussianSplatAsset.cs:47,66) */
    GS_ERR_HIP = -2,                /* a HIP runtime call failed; gs_last_error_string() has the detail */
    GS_ERR_UNSUPPORTED_FORMAT = -3, /* a format this build does not implement (none at present: kept for ABI stability) */
    GS_ERR_OUT_OF_MEMORY = -4,
    GS_ERR_INVALID_ASSET = -5,      /* blob sizes do not match splat_count/formats (C#: HasValidAsset, GaussianSplatRenderer.cs:361-368) */
    GS_ERR_PAIR_OVERFLOW = -6,      /* tile-pair buffer too small for this frame; the renderer grew it -- draw again */
    GS_ERR_SORT_TIMEOUT = -7,       /* a bounded spin in the sort's look-back expired (never expected; reported instead of hanging) */
    GS_ERR_NO_DEVICE = -8,
    GS_ERR_COMM = -9                /* RCCL: library not loadable, or a collective failed; gs_last_error_string() has the detail */
    /* (-10 was GS_ERR_TIE_OVERFLOW of ABI 7: GS_SORT_VISIBLE no longer has a case it cannot order) */
} gs_error;

/* GaussianSplatAsset.cs:31-37 / :51-57 / :70-81 */
typedef enum gs_vector_format { GS_VECTOR_FLOAT32 = 0, GS_VECTOR_NORM16 = 1, GS_VECTOR_NORM11 = 2, GS_VECTOR_NORM6 = 3 } gs_vector_format;
typedef enum gs_color_format { GS_COLOR_FLOAT32X4 = 0, GS_COLOR_FLOAT16X4 = 1, GS_COLOR_NORM8X4 = 2, GS_COLOR_BC7 = 3 } gs_color_format;
typedef enum gs_sh_format {
    GS_SH_FLOAT32 = 0, GS_SH_FLOAT16 = 1, GS_SH_NORM11 = 2, GS_SH_NORM6 = 3,
    GS_SH_CLUSTER64K = 4, GS_SH_CLUSTER32K = 5, GS_SH_CLUSTER16K = 6, GS_SH_CLUSTER8K = 7, GS_SH_CLUSTER4K = 8
} gs_sh_format;

/* GaussianSplatRenderer.RenderMode (GaussianSplatRenderer.cs:217-223) */
typedef enum gs_render_mode {
    GS_RENDER_SPLATS = 0, GS_RENDER_DEBUG_POINTS = 1, GS_RENDER_DEBUG_POINT_INDICES = 2, GS_RENDER_DEBUG_BOXES = 3, GS_RENDER_DEBUG_CHUNK_BOUNDS = 4
} gs_render_mode;

/* What gs_renderer_sort sorts (gs_renderer_set_sort_mode).  The reference sorts all N splats every frame because its sort precedes
 * its cull (GaussianSplatRenderer.cs:612-639 then :579-610); only the order among the splats that are DRAWN is ever observable. */
typedef enum gs_sort_mode {
    GS_SORT_FULL = 0,      /* SortPoints as the reference runs it: keys of all N splats through the previous order, stable sort of all N */
    GS_SORT_VISIBLE = 1    /* cull first: only the splats gs_renderer_calc_view found visible are keyed and sorted, every frame, with the matrix of
                              the last gs_renderer_sort; ties are ordered as the reference's stable sort history orders them */
} gs_sort_mode;

typedef struct gs_context gs_context;
typedef struct gs_asset gs_asset;
typedef struct gs_renderer gs_renderer;
typedef struct gs_target gs_target;
typedef struct gs_sorter gs_sorter;
typedef struct gs_comm gs_comm;

/* The five blobs of a GaussianSplatAsset (GaussianSplatAsset.cs:205-229), as uploaded by
 * GaussianSplatRenderer.CreateResourcesForAsset (GaussianSplatRenderer.cs:373-405). */
typedef struct gs_asset_desc {
    uint32_t splat_count;
    uint32_t pos_format;      /* gs_vector_format */
    uint32_t scale_format;    /* gs_vector_format */
    uint32_t color_format;    /* gs_color_format  */
    uint32_t sh_format;       /* gs_sh_format     */
    uint32_t memory_kind;     /* 0: pointers are host memory, copied.  1: pointers are device memory on the
                                 context's GPU, BORROWED (must outlive the asset; e.g. buffers filled by an RCCL broadcast):
                                 every blob base 16-byte aligned (the kernels use 16-byte vector loads; hipMalloc gives 256)
                                 and pos / other / sh declared with >= 4 readable bytes after their last record (the
                                 2-byte-aligned dword stitching of the decoder may touch the next dword; owned uploads
                                 are padded by the library).  Violations: GS_ERR_INVALID_ARGUMENT / GS_ERR_INVALID_ASSET. */
    const void* pos_data;    uint64_t pos_size;
    const void* other_data;  uint64_t other_size;
    const void* color_data;  uint64_t color_size;
    const void* sh_data;     uint64_t sh_size;
    const void* chunk_data;  uint64_t chunk_size;   /* NULL / 0 => _SplatChunkCount = 0 (all-fp32 asset) */
} gs_asset_desc;

/* Per-frame constants of CSCalcViewData (GaussianSplatRenderer.cs:597-606; SplatUtilities.compute:40-45,86-89)
 * plus the two Unity built-ins the shader reads (UNITY_MATRIX_VP, UNITY_MATRIX_P) and the camera clip range
 * the fixed-function rasteriser applies to the splat quads. */
typedef struct gs_frame_params {
    float matrix_mv[16];             /* _MatrixMV = worldToCameraMatrix * localToWorld */
    float matrix_object_to_world[16];/* _MatrixObjectToWorld */
    float matrix_world_to_object[16];/* _MatrixWorldToObject */
    float matrix_vp[16];             /* UNITY_MATRIX_VP (clip.w must be view depth: perspective camera) */
    float proj_m00, proj_m11;        /* UNITY_MATRIX_P._m00 / ._m11 */
    float screen_w, screen_h;        /* _VecScreenParams.xy */
    float cam_pos_world[3];          /* _VecWorldSpaceCameraPos.xyz */
    float splat_scale;               /* m_SplatScale   [0.1, 2]   */
    float opacity_scale;             /* m_OpacityScale [0.05, 20] */
    uint32_t sh_order;               /* m_SHOrder 0..3 */
    uint32_t sh_only;                /* m_SHOnly */
    float near_clip, far_clip;       /* camera near/far: a splat whose centre depth (clip.w) is outside is clipped */
} gs_frame_params;

/* One element of _SplatCutouts (SplatUtilities.compute:91-100 GaussianCutoutShaderData, filled by
 * GaussianCutout.GetShaderData, GaussianCutout.cs:24-40): `matrix` = cutout.worldToLocal * renderer.localToWorld
 * (row-major like every matrix of this ABI), type_and_flags = type (0 ellipsoid, 1 box, 0xFF.. = null cutout, ignored)
 * | 0x100 if inverted. */
typedef struct gs_cutout {
    float matrix[16];
    uint32_t type_and_flags;
} gs_cutout;

typedef struct gs_frame_stats {
    uint64_t tile_pairs;        /* P: (tile, splat) overlaps emitted by the binning kernel this frame, tiles of tile_w x tile_h pixels */
    uint64_t pair_capacity;     /* current capacity of the pair buffers */
    uint32_t visible_splats;    /* splats that survived culling (emitted >= 1 pair) */
    uint32_t tiles_x, tiles_y;
    uint32_t sort_error;        /* != 0 => GS_ERR_SORT_TIMEOUT was raised */
    uint32_t tile_w, tile_h;    /* the compositor tile of the last draw, pixels (16x16, 32x16 or 32x32: gs_renderer_set_tile_shape); 0 x 0 before the first draw */
    uint32_t sort_mode;         /* gs_sort_mode the last draw's order came from */
    uint32_t tie_long_runs;     /* GS_SORT_VISIBLE, statistics only: runs of more than 64 visible splats with equal sort keys in the last draw (ordered by the
                                   fix-up's workgroup-wide sorting network instead of a thread / a wave) ... */
    uint32_t tie_longest_run;   /* ... and the longest of them (0 if none) */
} gs_frame_stats;

/* hipEvent-timed stage durations of the last frame, ms (the four ProfilerMarkers of
 * GaussianSplatRenderer.cs:20-22,287 split further), averaged over the frames recorded since the last call.
 * Only valid after gs_renderer_set_profiling(r, frames > 0). */
typedef struct gs_stage_times {
    float calc_distances_ms;   /* CSCalcDistances (+ fused digit histograms) */
    float sort_ms;             /* 4 Onesweep passes */
    float calc_view_ms;        /* CSCalcViewData */
    float bin_ms;              /* tile binning: count + scan + emit */
    float pair_sort_ms;        /* stable sort of (tile, i) pairs by tile */
    float blend_ms;            /* per-tile front-to-back composite (RenderGaussianSplats.shader) */
    float resolve_ms;          /* GaussianComposite.shader */
    float total_ms;
    uint32_t frames;           /* number of frames the averages cover */
    /* the Onesweep launches alone (the kernel with the largest time share): sort_ms / pair_sort_ms minus the
     * histogram-scan, copy-back and tile-range kernels that share those stages */
    float onesweep_depth_ms;   /* sum of the depth-sort launches of one frame */
    float onesweep_pairs_ms;   /* sum of the pair-sort launches of one frame */
    uint32_t onesweep_pair_launches;   /* of the last draw, by tile count: 1 (<= 256 tiles), 2 (<= 65,536), 3 (up to 2^24) */
    /* the same launches by their OWN start / stop timestamps (the dispatch's completion signal, as rocprofv3 --kernel-trace reports
     * them): no event packets and no kernel boundaries inside, so <= the bracketed figures above.  0 unless the frames were recorded
     * with gs_renderer_set_kernel_timing(r, 1). */
    float onesweep_depth_kernel_ms;    /* sum over the depth-sort launches */
    float onesweep_pairs_kernel_ms;    /* sum over the pair-sort launches */
    uint32_t onesweep_depth_launches;  /* of the last frame: 4 (8-bit passes), or 0 when the frame made no depth sort (GS_SORT_VISIBLE with no sort recorded on an identity base: drawn in index order) */
} gs_stage_times;

int32_t gs_abi_version(void);
const char* gs_error_string(int32_t err);
const char* gs_last_error_string(void);          /* thread-local detail of the last failure */

/* ---- context ------------------------------------------------------------------------------------ */
/* `hip_stream` may be NULL (the context creates its own non-blocking stream) or a hipStream_t owned by
 * the caller (e.g. torch.cuda.current_stream().cuda_stream) on `device`. */
int32_t gs_context_create(int32_t device, void* hip_stream, gs_context** out);
int32_t gs_context_destroy(gs_context* ctx);
int32_t gs_context_synchronize(gs_context* ctx);
/* The depth sort of a frame depends on nothing else the frame computes, and only the draw's binning reads its result.
 * With overlap on, gs_renderer_sort (keys + the four passes) is enqueued on a second in-order queue owned by the context:
 * it is released by the previous draw's binning (the last reader of the order on the main queue) and joined by the next
 * consumer of the order (gs_renderer_draw or a readback), so with frames in flight it runs beside the previous draw's
 * blend / resolve and this frame's gs_renderer_calc_view.  Results are identical either way.  Default OFF: on MI355X every
 * kernel of the frame already fills the chip and the frame is not shorter.  Blocks until both queues are idle. */
int32_t gs_context_set_overlap(gs_context* ctx, int32_t enabled);
/* May OTHER kernels that wait on their own workgroups run on this GPU at the same time as this context's sorts and binning -- another process using this
 * library, or another context of this process working concurrently?  By default every kernel of the library takes its partitions in dependency order -- a running
 * workgroup only ever waits on workgroups that were started before it or on partitions a RUNNING workgroup holds, so it makes progress whatever holds the other
 * wave slots.  TWO forms are kept for speed for a context that has the GPU to itself; both are only deadlock-free if the workgroups still waiting for a slot get
 * one eventually (true beside any number of kernels of the default form, which finish with whatever workgroups they have -- not beside a second kernel of these forms):
 *   - the first pass of the full depth sort (GS_SORT_FULL) deals blocks of partitions to the XCDs (its random key gather then meets in one L2: 25 us per sort
 *     of 6 M keys);
 *   - a persistent grid that walks more partitions than it has workgroups (bin_emit of GS_SORT_FULL; a pair sort of more than ~6.3 M pairs in either sort mode)
 *     gives its FIRST partitions out statically, workgroup b taking partition b, instead of drawing every one from a single counter (whose ~1,000 simultaneous
 *     requests at the head of the kernel are served 12 ns apart: 16 us per frame at 6 M splats, 0.1 ms at 50 M).
 * shared > 0 selects the dependency-ordered forms everywhere, 0 keeps the two fast forms, < 0 (the default) decides per launch: shared while this process holds
 * more than one context on the device (the lanes of gs_renderer_set_frames_in_flight always use the dependency-ordered forms).  Another PROCESS on the GPU is
 * something only the host knows: set 1 (or GSPLAT_SHARED_GPU=1 in the environment) there.  (A stall is never a hang: every spin is bounded and surfaces as
 * GS_ERR_SORT_TIMEOUT.) */
int32_t gs_context_set_shared_gpu(gs_context* ctx, int32_t shared);
int32_t gs_context_device_info(gs_context* ctx, char* name_out, size_t name_cap, int32_t* cu_count, uint64_t* hbm_bytes);

/* ---- asset (replaces CreateResourcesForAsset's buffer uploads, GaussianSplatRenderer.cs:373-405) - */
int32_t gs_asset_create(gs_context* ctx, const gs_asset_desc* desc, gs_asset** out);
int32_t gs_asset_destroy(gs_asset* asset);                         /* DisposeResourcesForAsset :527-565 */
int32_t gs_asset_splat_count(const gs_asset* asset, uint32_t* out);
/* device addresses + sizes of pos, other, color, sh, chunk (for an RCCL broadcast by the host) */
int32_t gs_asset_device_blobs(const gs_asset* asset, void* ptrs[5], uint64_t sizes[5]);

/* splat_count, pos_format, scale_format, color_format, sh_format, chunk count (what a rank that received the asset by
 * gs_asset_broadcast needs to know about it) */
int32_t gs_asset_info(const gs_asset* asset, uint32_t out[6]);

/* ---- multi-GPU: view-parallel rendering, one context (= one GPU) per rank ------------------------------------------
 * The path shards by camera: every GPU holds a replica of the immutable asset and renders its own view, so the only
 * exchange is the load-time broadcast of the five blobs -- ncclBroadcast over xGMI, called directly from this library
 * (librccl is dlopen'ed on first use; GSPLAT_RCCL_LIB overrides its path).  The reference is single-GPU: nothing to cite.
 * Usage: one rank calls gs_comm_unique_id and hands the 128 bytes to every rank over any host channel; every rank then
 * calls gs_comm_create (collective) with its own context, the same id and its rank; the rank that loaded the asset is
 * `root` of gs_asset_broadcast (collective), after which every rank creates its renderer on the asset it got. */
#define GS_COMM_ID_BYTES 128
int32_t gs_comm_unique_id(uint8_t id_out[GS_COMM_ID_BYTES]);                                   /* ncclGetUniqueId */
int32_t gs_comm_create(gs_context* ctx, int32_t nranks, int32_t rank, const uint8_t id[GS_COMM_ID_BYTES], gs_comm** out);   /* ncclCommInitRank */
int32_t gs_comm_destroy(gs_comm* comm);
int32_t gs_comm_info(const gs_comm* comm, int32_t* nranks, int32_t* rank);
/* On `root`: asset_on_root = the asset to replicate (of the comm's context), *out = the same handle.  Elsewhere:
 * asset_on_root is ignored, *out = a new asset owning device copies of the blobs (destroy it with gs_asset_destroy).  Blocks. */
int32_t gs_asset_broadcast(gs_comm* comm, gs_asset* asset_on_root, int32_t root, gs_asset** out);
/* Single-process hosts (one gs_context per GPU, as a Unity player would hold them): a replica of `src` owned by `dst_ctx`, blobs
 * moved by a peer device copy -- the receive half of gs_asset_broadcast without a communicator.  Blocks. */
int32_t gs_asset_replicate(gs_context* dst_ctx, const gs_asset* src, gs_asset** out);

/* ---- renderer (per GaussianSplatRenderer component) ---------------------------------------------- */
/* allocates m_GpuView (N x 40 B), m_GpuSortDistances, m_GpuSortKeys, the sorter's SupportResources and the
 * tile-binning buffers; runs CSSetIndices (GaussianSplatRenderer.cs:407,423-445).  `asset` may belong to another context of the SAME GPU
 * (its blobs are immutable): several renderers on several contexts = several frames / views in flight on several streams over one copy
 * of the asset (in GS_SORT_VISIBLE every such renderer is told every SortPoints matrix -- gs_renderer_sort is bookkeeping there -- and draws
 * the frames dealt to it: each draws from the reference's order).  The asset must outlive its renderers. */
int32_t gs_renderer_create(gs_context* ctx, gs_asset* asset, gs_renderer** out);
int32_t gs_renderer_destroy(gs_renderer* r);
/* CSSetIndices (SplatUtilities.compute:59-67): order[i] = i */
int32_t gs_renderer_reset_order(gs_renderer* r);
/* SortPoints (GaussianSplatRenderer.cs:612-639): CSCalcDistances with _MatrixMV = `matrix_sort`
 * (= worldToCameraMatrix with m20,m21,m22 negated, times localToWorld -- the host builds it exactly as
 * the C# does), then GpuSorting.Dispatch on (distances, order). */
int32_t gs_renderer_sort(gs_renderer* r, const float matrix_sort[16]);
/* GS_SORT_FULL (default) or GS_SORT_VISIBLE.  In visible mode gs_renderer_sort only records the matrix; the sort itself runs inside
 * gs_renderer_draw over the splats gs_renderer_calc_view found visible (V of N): keys of those splats in index order, Onesweep passes over
 * V pairs, then a fix-up of runs of equal keys -- the reference's sort is stable through EVERY earlier sort, so after sorts M_1 .. M_k of a
 * base order B its buffer is sorted lexicographically by (key under M_k, ..., key under M_1, rank in B), and the fix-up orders tied splats by
 * exactly that chain: their keys under the recorded matrices, most recent first, then the base order.  What is drawn is the visible
 * subsequence of the reference's order buffer, bit for bit, BY CONSTRUCTION: no matrix is ever dropped (when 128 are recorded the library
 * carries them out on all N once -- one reference-shaped sort + the same fix-up over N, ~0.25 ms for 6 M splats -- and that buffer becomes
 * the new base), and a run of equal keys of any length is ordered (2..4 by a thread, ..64 by a wave, longer ones by a workgroup-wide sorting
 * network).  The base is whatever the order buffer holds when the mode is set or gs_renderer_upload_order / gs_renderer_reset_order is
 * called; the mode is active whenever it is set.  A frame that skips gs_renderer_sort (m_SortNthFrame > 1) orders its own visible set with
 * the stale matrix, as the reference's stale order buffer does.  Switching back to GS_SORT_FULL, gs_renderer_download_order and
 * gs_renderer_download_distances carry the recorded sorts out first and so see the reference's buffers. */
int32_t gs_renderer_set_sort_mode(gs_renderer* r, int32_t mode);
/* *mode = what was set; *active != 0 = the visible-only path is what the next draw uses (ABI 8: whenever it is set) */
int32_t gs_renderer_sort_mode(const gs_renderer* r, int32_t* mode, int32_t* active);
/* GS_SORT_VISIBLE tuning / introspection.  rows in [2, 128]: matrices recorded before the library carries them out on all N (default 128;
 * a smaller limit shortens the longest possible tie chain and consolidates more often -- the drawn order is the same either way).
 * gs_renderer_sort_history: any pointer may be NULL; *rows = matrices recorded since the base, *consolidations = how often they were carried out. */
int32_t gs_renderer_set_sort_history_limit(gs_renderer* r, uint32_t rows);
int32_t gs_renderer_sort_history(const gs_renderer* r, uint32_t* rows, uint32_t* limit, uint64_t* consolidations);
/* Frames (or the views of a multi-view batch) in flight INSIDE the library, behind one renderer: frames > 1 makes that many lanes -- renderers on contexts
 * (= HIP streams) of their own over this renderer's asset, owned by it.  While the renderer is in GS_SORT_VISIBLE and draws splats, every
 * gs_renderer_calc_view moves on to the next lane and that frame's kernels (calc_view, the visible-only sort, the binning, the pair sort, the blend) run on
 * the lane's stream: one frame's latency-bound chain under another frame's blend (C2: 0.56 -> 0.45 ms per frame with two).  The calls stay the
 * reference's -- SortPoints, CalcViewData, the draw, the composite on ONE GaussianSplatRenderer (GaussianSplatRenderer.cs:108-169) -- and so do the results:
 * gs_renderer_sort is bookkeeping in that mode and every lane is told every matrix, so each frame is drawn from the reference's order,
 * the same bits as with one frame at a time.  The target stays the context's: a lane's blend waits for what the context's stream holds for the target when
 * gs_renderer_draw is called -- its last use: a clear, a resolve, another draw; everything the stream holds once the host has taken the device pointers -- and the stream waits for the
 * blend, so gs_target_resolve / _download and anything the host enqueues afterwards see the finished frame.  (A target of a context with lanes holds two pixel
 * buffers and gs_target_clear moves on to the other one: drawing every frame into the same target does not queue a blend behind the previous frame's composite.)
 * What is NOT ordered against the context's stream any more is the rest of the frame (it reads the asset and the renderer's settings only): change those through
 * this API.  It is throughput, not latency; a host that blocks after every frame gains nothing.  GS_SORT_FULL and the debug render modes run on the renderer's
 * own context as before (the reference's sort has one order buffer that every frame mutates; dealing its frames to lanes with the sorts on a second queue was
 * built and measured slower -- the big sorts find no wave slots beside a blend: docs/experiments.md).  frames = 1 (the default) frees the lanes.  Costs the per-frame buffers once more per lane (about 100 B per splat). */
#define GS_MAX_FRAMES_IN_FLIGHT 4
int32_t gs_renderer_set_frames_in_flight(gs_renderer* r, int32_t frames);
/* *frames = what was set; *active != 0 = the next gs_renderer_calc_view goes to a lane */
int32_t gs_renderer_frames_in_flight(const gs_renderer* r, int32_t* frames, int32_t* active);
/* CalcViewData (GaussianSplatRenderer.cs:579-610): CSCalcViewData.  The reference's output, the N x 40 B m_GpuView
 * buffer, is only read by its own vertex shader; here the compositor reads compact per-splat records instead, so by
 * default the kernel evaluates colour (SH) only for the splats that reach the screen and does not write m_GpuView.
 * gs_renderer_download_view materialises it on demand (re-running the frame's launch as the reference's full kernel), so
 * what that function returns is the reference's buffer either way. */
int32_t gs_renderer_calc_view(gs_renderer* r, const gs_frame_params* p);
/* 1: run the full CSCalcViewData every frame (all colours, m_GpuView written), exactly like the reference; 0 (default): on demand */
int32_t gs_renderer_set_view_buffer_mode(gs_renderer* r, int32_t every_frame);
/* the DrawProcedural of SortAndRenderSplats (GaussianSplatRenderer.cs:156-166): blends all splats in
 * order[] front-to-back into `rt` (RGBA16F, premultiplied; "Blend OneMinusDstAlpha One"). rt is NOT cleared. */
int32_t gs_renderer_draw(gs_renderer* r, const gs_frame_params* p, gs_target* rt);
/* convenience: sort (if do_sort) + calc_view + clear + draw, one call */
int32_t gs_renderer_render(gs_renderer* r, const float matrix_sort[16], const gs_frame_params* p, gs_target* rt, int32_t do_sort);
/* UpdateCutoutsBuffer (GaussianSplatRenderer.cs:742-764) + _SplatCutoutsCount (:508): the cutouts CSCalcViewData tests
 * every splat against (IsSplatCut, SplatUtilities.compute:164-187; a cut splat gets clip.w = 0).  Copied; count 0 /
 * NULL removes them.  At most GS_MAX_CUTOUTS. */
#define GS_MAX_CUTOUTS 64
int32_t gs_renderer_set_cutouts(gs_renderer* r, const gs_cutout* cutouts, uint32_t count);
/* m_GpuEditDeleted + _SplatBitsValid (GaussianSplatRenderer.cs:497,501; SplatUtilities.compute:204-214): one bit per
 * splat, bit set = deleted (clip.w = 0).  `words` = ceil(N/32) host uint32s, copied; NULL => _SplatBitsValid = 0. */
int32_t gs_renderer_set_deleted_bits(gs_renderer* r, const uint32_t* words, size_t word_count);

/* ---- selection and deletion: GaussianSplatRenderer.Edit* (GaussianSplatRenderer.cs:705-740,767-840,896-934) ----------
 * (additions to ABI 9)  The half of the reference's editor that never writes the asset: the selection set, rectangle selection
 * through a camera, counts and bounds, deletion.  The seven kernels behind it -- CSInitEditData, CSUpdateEditData, CSClearBuffer,
 * CSInvertSelection, CSSelectAll, CSOrBuffers, CSSelectionUpdate (SplatUtilities.compute:266-423) -- leave in memory, word for word,
 * what the reference's leave.  The buffers are made at the first edit call (EnsureEditingBuffers, :767-786): `selected` and its
 * mouse-down copy, ceil(N/32) zeroed words each; the deleted buffer is the one gs_renderer_set_deleted_bits fills -- made (zeroed) by
 * the first delete, and read as zeros while it does not exist.  Every kernel tests the splats against the renderer's current
 * gs_renderer_set_cutouts list (IsSplatCut), as the reference's do.
 * Selection is DRAWN -- the reference's highlight of selected splats, RenderGaussianSplats.shader:63-73,87-101 -- once
 * gs_renderer_set_selection_highlight (below) is on; by default it is off and only deletion, the transforms and the merge below change a
 * frame.  Exporting only reads the blobs: see below.
 * Two literal quirks of the reference are kept: select-all / invert set the bits of the last word beyond N and the counts include them
 * (N = 33: select all reports 64 selected), and a splat whose pixel position is NaN is inside every rectangle.
 * The mutating calls are asynchronous on the context's stream like every other call; the info / download calls block.  Selection lives
 * on the renderer it was made on; with frames in flight the lanes' deleted bits follow a delete by a device-to-device copy on each
 * lane's own stream (no host synchronisation), so a frame already dealt to a lane keeps the bits of the time it was dealt. */
typedef struct gs_edit_info {          /* m_GpuEditCountsBounds decoded; 36 bytes */
    uint32_t selected, deleted, cut;    /* editSelectedSplats, editDeletedSplats, editCutSplats: deleted splats count as neither selected nor cut */
    float bounds_min[3], bounds_max[3]; /* object space, of the selected splats; raw: +1e38 / -1e38 when nothing is selected */
} gs_edit_info;
int32_t gs_renderer_edit_select_all(gs_renderer* r);                /* EditSelectAll :906-915: every bit but the cut splats' */
int32_t gs_renderer_edit_deselect_all(gs_renderer* r);              /* EditDeselectAll :917-922 */
int32_t gs_renderer_edit_invert_selection(gs_renderer* r);          /* EditInvertSelection :924-934 */
int32_t gs_renderer_edit_store_selection(gs_renderer* r);           /* EditStoreSelectionMouseDown :788-792 */
/* EditUpdateSelection (:811-840): selected = mouse-down copy, then CSSelectionUpdate with p's matrix_object_to_world / matrix_vp / screen_w,h;
 * selection_rect = _SelectionRect (x_min, y_min, x_max, y_max), pixels, x right, y UP from the bottom edge.  A splat that is not cut, has
 * clip.w > 0 and whose centre projects inside the rectangle is added to the selection, or with subtract != 0 removed from it. */
int32_t gs_renderer_edit_update_selection(gs_renderer* r, const gs_frame_params* p, const float selection_rect[4], int32_t subtract);
int32_t gs_renderer_edit_delete_selected(gs_renderer* r);           /* EditDeleteSelected :896-904: deleted |= selected; selected = 0 */
/* UpdateEditCountsAndBounds (:705-740): CSInitEditData + CSUpdateEditData; blocks.  All zeros while the renderer has no edit buffers. */
int32_t gs_renderer_edit_info(gs_renderer* r, gs_edit_info* out);
/* the selected words from the host (ceil(N/32) of them, copied), e.g. a selection the host computed or saved */
int32_t gs_renderer_edit_upload_selected_bits(gs_renderer* r, const uint32_t* words, size_t word_count);
/* ceil(N/32) words each; any may be NULL; a buffer that does not exist reads as zeros; blocks */
int32_t gs_renderer_edit_download_bits(gs_renderer* r, uint32_t* selected, uint32_t* selected_mouse_down, uint32_t* deleted, size_t word_count);
int32_t gs_renderer_edit_release(gs_renderer* r);                   /* frees selected + mouse-down (bits, pos, other, sh); deleted bits and moved splats stay */
/* The reference's highlight of the selection (RenderGaussianSplats.shader:63-73,87-101; _SplatBitsValid, GaussianSplatRenderer.cs:518-520)
 * (addition to ABI 9).  enabled != 0: every GS_RENDER_SPLATS frame whose gs_renderer_calc_view runs while the edit buffers exist draws the splats
 * selected at that call as the reference does: tinted magenta (rgb = lerp(rgb, (1, 0, 1), 0.5)), with raised opacity (alpha = saturate(e + 0.3)
 * where e = exp(-|q|^2) > 7/255, else e) and a solid magenta outline ring where 7/255 < e < 10/255.  The splat's own opacity plays no part: a
 * selected splat of opacity 0 is drawn, with the footprint of an opacity-1 splat, so a large selection of faint splats raises the pair count
 * (the pair buffers grow as for any other frame).  Deleted, cut and behind-the-camera splats are not drawn, selected or not; the debug render
 * modes do not show the selection.  gs_renderer_download_view is unchanged (the reference marks the splat in the vertex stage, not in the view
 * buffer); gs_renderer_download_raster_records shows the mark (alpha half = -1, 0xBC00) and the larger rectangles.  Default 0: frames are what
 * they are without this call, and cost the same.  With no edit buffers (no edit call yet, or after gs_renderer_edit_release) the switch changes
 * nothing.  A plain setting: kept by gs_renderer_edit_set_splat_count, shared by the lanes of gs_renderer_set_frames_in_flight, whose copies of
 * the selected bits follow every selection change like the deleted bits follow a delete (a frame already dealt keeps the selection of the time
 * it was dealt).  A host that wants the reference's editor behaviour sets it to 1 once. */
int32_t gs_renderer_set_selection_highlight(gs_renderer* r, int32_t enabled);

/* ---- moving the selection: EditTranslateSelection / EditRotateSelection / EditScaleSelection (GaussianSplatRenderer.cs:794-809,842-894;
 * CSTranslateSelection, CSRotateSelection, CSScaleSelection, SplatUtilities.compute:425-521)  (additions to ABI 9) ----
 * The three kernels rewrite positions and rotation words.  An asset's blobs stay immutable and shared: the first transform that can write
 * gives THIS renderer a private device copy of the pos and / or other blob (copy-on-write), which every later call on the renderer and its
 * lanes reads -- frames, sorts, selection, bounds, export.  The asset, its replicas and other renderers over it never see an edit; a renderer
 * that is never transformed allocates nothing.  The reference's format gates are kept literally: positions are written only in a chunk-less
 * asset with GS_VECTOR_FLOAT32 positions, rotation words only in a chunk-less asset with fp32 scales and fp32 SH; where no gate passes a call
 * returns GS_OK and changes nothing.  Rotate reads pos and other from their mouse-down copies, scale reads pos from its copy, both write
 * the current blobs; translate reads and writes the current positions.  Rotate without both store calls (scale: without the pos one) is
 * GS_ERR_INVALID_ARGUMENT.  SHs are not rotated and splat scales not scaled (the reference's own TODOs) unless
 * gs_renderer_edit_set_rigid_transforms (below) is on.  Arithmetic: DESIGN.md section 4.7;
 * one deviation -- the fields of a re-encoded rotation word are clamped to their ranges, which only matters for a delta quaternion that is
 * not of unit length.  Asynchronous on the context's stream and ordered against sorts, GS_SORT_VISIBLE's history (the order buffer as the
 * reference holds it at the call becomes the new base) and frames in flight (a frame already dealt to a lane finishes with the old
 * positions).  Until the next calc_view the frame is drawn from the old view records, as in the reference, and a view download that would
 * have to materialise them fails with GS_ERR_INVALID_ARGUMENT.  Matrices are row-major, quaternions x y z w. */
int32_t gs_renderer_edit_store_pos_mouse_down(gs_renderer* r);     /* EditStorePosMouseDown   :794-801 */
int32_t gs_renderer_edit_store_other_mouse_down(gs_renderer* r);   /* EditStoreOtherMouseDown :802-809 */
int32_t gs_renderer_edit_translate_selection(gs_renderer* r, const float delta[3]);                       /* :842-854 */
int32_t gs_renderer_edit_rotate_selection(gs_renderer* r, const float center[3], const float local_to_world[16],
                                          const float world_to_local[16], const float rotation_xyzw[4]);   /* :856-874 */
int32_t gs_renderer_edit_scale_selection(gs_renderer* r, const float center[3], const float local_to_world[16],
                                         const float world_to_local[16], const float scale[3]);            /* :877-894 */
/* Rigid rotate and scale (additions to ABI 9).  Off by default: every call above is then what it is without these two.
 * enabled != 0: a rotated selection turns as one object and a uniformly scaled one grows as one -- what the reference's three @TODOs leave out.
 * The format gates stay the reference's: positions as above; rotation word, scale and SH are written only in a chunk-less asset with fp32 scales
 * and fp32 SH; where no gate passes a call returns GS_OK and launches nothing.
 *   rotate   positions as above.  With L = W2O3 . R(delta) . O2W3 the linear part of the position map (delta normalised; all in fp64, rounded to
 *            fp32 once), every selected splat's rotation word becomes QuatMul(q_L, rot) re-encoded and its 15 SH coefficients go through the band
 *            matrices of L -- the arithmetic of the merge and the baked export, from the mouse-down state.  q_L and the bands are taken from L
 *            with its rows normalised, the reference's answer for a matrix that is not a pure rotation.  Of a 192-byte SH record the first 180
 *            bytes are rewritten.  Needs all three store calls, a delta of finite non-zero norm and a local_to_world without a zero or
 *            non-finite row: otherwise GS_ERR_INVALID_ARGUMENT (checked before the gates).  The first such call makes the SH blob private.
 *   scale    positions as above.  If the three components of `scale` are equal as floats (s s s: the uniform handle) the three fp32 scales of
 *            every selected splat become their mouse-down values times |s| -- 12 bytes of the other record; this needs the `other` store call
 *            (else GS_ERR_INVALID_ARGUMENT).  A non-uniform scale leaves splat sizes alone, as the reference does: the image of a rotated
 *            ellipsoid under an anisotropic scale is not an ellipsoid with the same axes, and finding its axes takes an eigen-decomposition per
 *            splat -- not done.  s < 0 multiplies by |s| and does not touch the SH (the odd bands would change sign) -- not done either.
 *   translate is unchanged.
 * A plain setting: kept by gs_renderer_edit_set_splat_count, read by the lanes of gs_renderer_set_frames_in_flight through their owner.
 * gs_renderer_edit_store_sh_mouse_down is the third mouse-down copy: the renderer's CURRENT SH blob, device to device on the context's stream,
 * allocated only where the rotation gate passes; that it was called is remembered either way.  gs_renderer_edit_release frees it, a resize drops
 * it (with the other two), a lane handle is GS_ERR_INVALID_ARGUMENT.  Memory: the copy and the private SH blob are 192 bytes per splat EACH --
 * about 2.4 GB together for a 6.1 M-splat VeryHigh asset -- and exist only on a renderer that stored / rotated with the setting on. */
int32_t gs_renderer_edit_set_rigid_transforms(gs_renderer* r, int32_t enabled);
int32_t gs_renderer_edit_store_sh_mouse_down(gs_renderer* r);
/* the renderer's CURRENT pos / other blobs (the private copy if there is one, else the asset's); either may be NULL; blocks */
int32_t gs_renderer_edit_download_pos_other(gs_renderer* r, void* pos, size_t pos_bytes, void* other, size_t other_bytes);

/* ---- export: EditExportData (GaussianSplatRenderer.cs:936-958), CSExportData (SplatUtilities.compute:523-673) and the editor's
 * ExportPlyFile (GaussianSplatRendererEditor.cs:394-445)  (additions to ABI 9) ----
 * A record is the reference's ExportSplatData = InputSplatData = one PLY vertex: 62 floats -- pos, nor, f_dc, 45 f_rest (15 R, 15 G, 15 B),
 * opacity (logit), scale (log), rot (w x y z) -- decoded from the asset in whatever formats it has.  log() is LogDet, the project's fixed
 * member of HLSL's family, so the bytes are the same on every machine.  With bake_transform != 0 the record is
 * moved into world space as the reference does: position by the matrix, rotation by `rotation` (x y z w) after the axis flips of a
 * negative `scale`, scale by |scale|, SH rotated by the matrix' rotation.  The calls read the renderer's current deleted bits (none = all
 * zero) and gs_renderer_set_cutouts list, run on the context's stream and BLOCK until the output is complete.  Output that goes to the
 * host is produced in batches of whole 256-splat chunks through a fixed device buffer and two pinned buffers, never N x 248 bytes at once
 * (GSPLAT_EXPORT_BATCH = splats per batch, read at every call). */
#define GS_EXPORT_RECORD_BYTES 248
typedef struct gs_export_params {
    float matrix_object_to_world[16];   /* transform.localToWorldMatrix, row-major */
    float rotation[4];                  /* transform.localRotation x y z w */
    float scale[3];                     /* transform.localScale */
    uint32_t bake_transform;            /* _ExportTransformFlags */
} gs_export_params;
/* EditExportData: all N records in index order, nor = 1 for cut splats (deleted ones are written like any other: the editor skips them).
 * out: host memory (memory_kind 0) or device memory (1, 8-byte aligned: GS_ERR_INVALID_ARGUMENT otherwise) of at least N x 248 bytes. */
int32_t gs_renderer_edit_export_data(gs_renderer* r, const gs_export_params* p, void* out, size_t bytes, int32_t memory_kind);
/* the records of the alive splats only (not deleted, not cut), index order, nor = 0; *alive = their number; out (host memory,
 * capacity_records records) may be NULL to get the count alone. */
int32_t gs_renderer_edit_export_alive(gs_renderer* r, const gs_export_params* p, void* out, size_t capacity_records, uint32_t* alive);
/* ExportPlyFile: the reference's header + the alive records.  On an error the partially written file is removed. */
int32_t gs_renderer_edit_export_ply(gs_renderer* r, const gs_export_params* p, const char* path, uint32_t* alive);

/* ---- export to SPZ (no counterpart in the reference, which only reads the format: SPZFileReader.cs:26-198)  (additions to ABI 9) ----
 * The alive splats as an SPZ version 2 file, 64 bytes per splat before gzip at SH level 3: the inverse of what gs_spz_open /
 * gs_splat_file_open read, packed on the GPU column by column from the same records the PLY export writes (after bake_transform), except
 * alpha, which is the decoded linear opacity x 255.  DESIGN.md section 4.13 states every byte operation by operation (fp32, round to
 * nearest even, clamped; SH codes are plain roundings).  The body is the gunzipped stream: a 16-byte header (magic, version 2, count,
 * sh_level | fract_bits << 8), then the columns positions (n x 9), alpha (n), colour (n x 3), scale (n x 3), rotation (n x 3),
 * SH (n x 3 x {0, 3, 8, 15}).  Both calls read the current deleted bits and cutout list, run on the context's stream and BLOCK.  The
 * columns reach the host through two pinned slices of slice_bytes that fill alternately; the file call deflates each slice as it
 * arrives (gzip wrapper) and removes a partially written file on any error.  Refused with GS_ERR_INVALID_ARGUMENT, nothing written:
 * a NULL r, p or s; a lane; sh_level > 3; fract_bits > 24 other than GS_SPZ_FRACT_AUTO; compression_level outside -1..9; slice_bytes
 * 1..4095; a too-small capacity_bytes; no alive splat, or more than 10,000,000 (the readers refuse both). */
#define GS_SPZ_FRACT_AUTO 0xffffffffu
typedef struct gs_spz_params {
    uint32_t sh_level;                  /* 0..3: 0, 3, 8 or 15 SH coefficients per splat */
    uint32_t fract_bits;                /* 0..24 fractional bits of the 24-bit positions, or GS_SPZ_FRACT_AUTO: the largest value up
                                         * to 12 at which the largest |coordinate| of the exported positions still fits */
    int32_t compression_level;          /* -1..9, handed to zlib as given (the file call only) */
    uint32_t slice_bytes;               /* 0 = 64 MiB; else at least 4096 */
} gs_spz_params;
/* the gunzipped stream (header + six columns) of the alive splats to host memory; out may be NULL to get the sizes alone */
int32_t gs_renderer_edit_export_spz_body(gs_renderer* r, const gs_export_params* p, const gs_spz_params* s, void* out, size_t capacity_bytes,
                                         uint64_t* body_bytes, uint32_t* alive, uint32_t* fract_bits_used);
int32_t gs_renderer_edit_export_spz(gs_renderer* r, const gs_export_params* p, const gs_spz_params* s, const char* path, uint32_t* alive);

/* ---- merge: EditSetSplatCount / EditCopySplatsInto / EditCopySplats (GaussianSplatRenderer.cs:960-1075), CSCopySplats
 * (SplatUtilities.compute:675-758); the editor's MergeSplatObjects (GaussianSplatRendererEditor.cs:213-235) is host code over the two
 * (additions to ABI 9) ----
 * The kernel decodes source splats of any format, applies the copy transform (position by the matrix, rotation by `rotation` after the axis
 * flips of a negative `scale`, scale by |scale|, SH rotated by the matrix' rotation: the export's bake) and writes records in the fixed
 * VeryHigh layout: pos 12 B, other 16 B (Norm10 rotation word + fp32 scale), an fp32 RGBA texel at the Morton position of the destination
 * index, a 192-byte SH record whose last 12 bytes are not written.  The library takes matrix, rotation and scale as given
 * (_CopyTransformMatrix / Rotation / Scale); it does not derive them.  Kept literally: the kernel bounds-checks src_start + i and reads ITS
 * deleted bit but loads splat i (both callers of the reference pass src_start = 0); cut splats are copied like any other; a deleted source bit
 * is OR-ed into the destination's word and never cleared.  count is clamped at either renderer's end.
 * The destination must be chunk-less with GS_VECTOR_FLOAT32 pos / scale, fp32 SH and GS_COLOR_FLOAT32X4 colour (the reference tests only
 * chunkData != null, which its importer makes equivalent), else GS_ERR_INVALID_ARGUMENT with nothing changed.  The asset stays immutable:
 * the destination's four blobs become private to the renderer on its first copy (copy-on-write), all four at once on a resize.
 * gs_renderer_edit_set_splat_count: new zero-filled blobs, deleted and selection buffers of new_count splats, the old splats copied into
 * them (p == NULL: the exact identity), and every per-N buffer replaced: afterwards the renderer is in the state of a freshly created one of
 * new_count splats over those blobs with the same deleted bits -- identity order, no valid view, an empty sort history, no mouse-down copies --
 * and its settings (blend / render / sort mode, tile shape, history limit, cutouts, profiling, reserved pairs, frames in flight) kept.  It
 * synchronises the context and its lanes and BLOCKS.  A count outside [1, 2^30], a lane handle or a failed gate: GS_ERR_INVALID_ARGUMENT;
 * new_count == the current count: GS_OK, nothing done.  Everything new is allocated before anything old is released: on
 * GS_ERR_OUT_OF_MEMORY the renderer is unchanged (but for lanes that could not be made again).
 * gs_renderer_edit_copy_splats_into: asynchronous on the destination's stream, ordered like a transform (sorts, GS_SORT_VISIBLE's history,
 * frames in flight) and, where the two renderers live on different contexts of one GPU, against the source's stream by events in both
 * directions.  src == dst, a lane handle or renderers on different GPUs: GS_ERR_INVALID_ARGUMENT. */
typedef struct gs_copy_params {
    float matrix[16];                   /* _CopyTransformMatrix = dst.worldToLocal x src.localToWorld, row-major */
    float rotation[4];                  /* _CopyTransformRotation x y z w (Matrix4x4.rotation of it) */
    float scale[3];                     /* _CopyTransformScale (Matrix4x4.lossyScale of it) */
} gs_copy_params;
int32_t gs_renderer_splat_count(const gs_renderer* r, uint32_t* out);           /* m_SplatCount: the asset's until a resize */
int32_t gs_renderer_edit_set_splat_count(gs_renderer* r, uint32_t new_count, const gs_copy_params* p);          /* :960-1031 */
int32_t gs_renderer_edit_copy_splats_into(gs_renderer* src, gs_renderer* dst, const gs_copy_params* p,
                                          uint32_t src_start, uint32_t dst_start, uint32_t count);               /* :1033-1075 */
/* the renderer's CURRENT four blobs (private copies where they exist, else the asset's); any pointer may be NULL; blocks */
int32_t gs_renderer_edit_download_splat_data(gs_renderer* r, void* pos, size_t pos_bytes, void* other, size_t other_bytes,
                                             void* color, size_t color_bytes, void* sh, size_t sh_bytes);

/* ---- undo and redo of the edit state: a sparse journal kept on the GPU (no counterpart in the reference, which has no undo:
 * docs/splat-editing.md)  (additions to ABI 9) ----
 * Off by default: a renderer that never calls gs_renderer_edit_history_enable allocates nothing, launches nothing new and behaves as without
 * these calls.  gs_renderer_edit_history_enable(r, max_bytes): max_bytes > 0 switches the history on (or changes the budget of one that is
 * on, evicting the oldest entries that no longer fit); 0 switches it off and frees every entry.
 * gs_renderer_edit_checkpoint(r, what) is called BEFORE a gesture, where the reference's tools call EditStore*MouseDown, and captures what
 * the gesture may change:
 *   GS_HIST_SELECTION / GS_HIST_DELETED   the bit buffer, whole: whatever changes it before the next checkpoint is undone,
 *                                         gs_renderer_edit_upload_selected_bits and gs_renderer_set_deleted_bits included;
 *   GS_HIST_POS / OTHER / SH              the 12 / 16 / 192-byte records of the splats selected AT THE CALL (index < N: the tail bits select-all
 *                                         sets are never gathered), in index order, with their index list;
 *   GS_HIST_TRANSFORM                     POS | OTHER, and SH iff gs_renderer_edit_set_rigid_transforms is on.
 * The format gates are the transforms': POS only in a chunk-less asset with fp32 positions, OTHER and SH only in a chunk-less asset with fp32
 * scales and fp32 SH.  A flag whose gate fails is dropped silently (top_what reports what was kept); if nothing is left the call returns GS_OK
 * and pushes nothing.  The call BLOCKS: one 4-byte readback of the selected count sizes the entry, and everything is allocated before the
 * stack changes.  A checkpoint drops all redo entries.  If the entry does not fit into the budget the oldest entries are evicted until it does
 * (`evicted` counts them); an entry that alone exceeds max_bytes: GS_ERR_OUT_OF_MEMORY, history and renderer unchanged.
 * An entry costs 4 ceil(N/32) bytes per captured bit buffer + k x (4 + 12 + 16 + 192) bytes for k journalled splats (less without a kind).
 * gs_renderer_edit_undo / _redo are one operation: the entry's contents are SWAPPED with the renderer's current state -- bit buffers word for
 * word, records through the index list -- so the entry then holds the state it replaced; undo moves it to the redo side, redo moves it back.
 * Both are asynchronous on the context's stream and ordered like the call they undo: a record swap like a transform (sorts on the second
 * queue, GS_SORT_VISIBLE's base and history, frames in flight; gs_renderer_download_view needs a new gs_renderer_calc_view afterwards), a swap
 * of the deleted / selected bits like a delete / a selection call (the lanes' copies follow).  Buffers that were released in between
 * (gs_renderer_edit_release, gs_renderer_set_deleted_bits(NULL)) are made again, zeroed, first.  A blob the renderer has no private copy of at
 * that time cannot have been written since the checkpoint and is skipped.  With nothing to undo / redo: GS_OK, nothing done.
 * CONTRACT FOR RECORDS: an entry restores exactly the splats that were selected at its checkpoint.  While the history is on, every call that
 * changes journalable state -- every selection call, delete, the bit uploads, the three transforms, gs_renderer_edit_copy_splats_into on its
 * destination -- drops the redo entries first (host bookkeeping, no kernel).  gs_renderer_edit_set_splat_count and
 * gs_renderer_edit_copy_splats_into clear the WHOLE history of the renderer they resize / write into (the copy writes index ranges, not the
 * selection); the switch, the budget and the counters survive a resize.  uncovered_transforms counts the transforms issued while there is
 * nothing to undo, while the entry an undo would apply captured no records, or after the selection may have changed since that entry (judged
 * by any selection-changing call, an undo / redo of GS_HIST_SELECTION included: conservative, a pure subtraction counts too) -- gestures an
 * undo would not fully take back.  gs_renderer_edit_release keeps the history.  The mouse-down copies are not touched by any of this.
 * A lane handle, a NULL argument, `what` zero or with unknown bits, and checkpoint / undo / redo while the history is off:
 * GS_ERR_INVALID_ARGUMENT, nothing changed. */
#define GS_HIST_SELECTION 1u            /* editSelected, all ceil(N/32) words */
#define GS_HIST_DELETED   2u            /* deletedBits, all words (absent buffer = zeros) */
#define GS_HIST_POS       4u            /* 12-byte positions of the splats selected now */
#define GS_HIST_OTHER     8u            /* 16-byte other records of the same splats */
#define GS_HIST_SH        16u           /* 192-byte SH records of the same splats */
#define GS_HIST_TRANSFORM 0x80000000u   /* POS|OTHER, plus SH iff rigid transforms are on */
typedef struct gs_edit_history_info {
    uint32_t enabled, undo_depth, redo_depth, top_what;  /* top_what: flags actually captured by the entry an undo would apply */
    uint64_t bytes, max_bytes;                           /* device bytes held by all entries; the budget */
    uint64_t top_bytes; uint32_t top_splats;             /* of the entry an undo would apply (0 if none) */
    uint32_t evicted, uncovered_transforms;              /* counters since enable */
} gs_edit_history_info;
int32_t gs_renderer_edit_history_enable(gs_renderer* r, uint64_t max_bytes);  /* 0 = disable and free */
int32_t gs_renderer_edit_checkpoint(gs_renderer* r, uint32_t what);
int32_t gs_renderer_edit_undo(gs_renderer* r);
int32_t gs_renderer_edit_redo(gs_renderer* r);
int32_t gs_renderer_edit_history_clear(gs_renderer* r);
int32_t gs_renderer_edit_history_info(const gs_renderer* r, gs_edit_history_info* out);

/* m_RenderMode + m_PointDisplaySize (GaussianSplatRenderer.cs:241-242; material choice :126-131).  DebugPoints / DebugPointIndices
 * (GaussianDebugRenderPoints.shader) draw every splat as an opaque screen-space square of `point_display_size` pixels, nearest
 * wins (ZWrite On), colour = saturate(DC colour) or an index code; gs_renderer_draw then neither needs gs_renderer_sort nor
 * gs_renderer_calc_view.  DebugBoxes (GaussianDebugRenderBoxes.shader) draws one box per splat -- half axes 2 x rotation x scale x
 * splat_scale, colour saturate(DC colour), alpha saturate(opacity x opacity_scale) -- through the order buffer (so it needs
 * gs_renderer_sort, not gs_renderer_calc_view), DebugChunkBounds one box per 256-splat chunk (position bounds, palette colour,
 * alpha 0.1, chunk order); both are blended like the splats and honour the depth attachment.  A box draw overwrites the
 * per-splat tile rectangles: call gs_renderer_calc_view again before the next Splats draw. */
int32_t gs_renderer_set_render_mode(gs_renderer* r, int32_t mode, float point_display_size);
/* 0 (default): "exact" -- accumulate in fp16 (RTNE after every blend, like the RGBA16F ROP).
 * 1: "fast" -- accumulate in fp32, stop a pixel when 1-A < 1/4096. */
int32_t gs_renderer_set_blend_mode(gs_renderer* r, int32_t mode);
/* The compositor's tile, pixels: 16x16, 32x16 or 32x32; 0, 0 (default) = chosen per target size.  The reference has no such
 * parameter (its rasteriser is fixed-function); here it trades (tile, splat) pairs to list and sort against records each wave
 * tests per pixel block.  A performance knob only: the frame is bit-identical whatever the shape.  gs_renderer_tile_shape
 * reports what a draw into a width x height target uses (the override, else the automatic choice, which GSPLAT_TILE=WxH pins). */
int32_t gs_renderer_set_tile_shape(gs_renderer* r, uint32_t tile_w, uint32_t tile_h);
int32_t gs_renderer_tile_shape(const gs_renderer* r, uint32_t width, uint32_t height, uint32_t* tile_w, uint32_t* tile_h);
/* frames = 0: off.  frames > 0: keep a ring of `frames` per-frame hipEvent sets (no host sync while rendering);
 * a frame ends at gs_renderer_draw.  gs_renderer_stage_times averages over the ring and resets it. */
int32_t gs_renderer_set_profiling(gs_renderer* r, int32_t frames);
/* With profiling on: enabled != 0 makes every Onesweep launch carry its OWN start / stop timestamps (gs_stage_times.onesweep_*_kernel_ms:
 * the dispatch's completion signal, what rocprofv3 --kernel-trace reports).  Those launches cost a few us each, so the stage brackets of
 * frames recorded in this mode (sort_ms, pair_sort_ms, total_ms) read high: use it in a pass of its own.  Default off. */
int32_t gs_renderer_set_kernel_timing(gs_renderer* r, int32_t enabled);
int32_t gs_renderer_reserve_pairs(gs_renderer* r, uint64_t pair_capacity);
/* Non-blocking: the (tile, splat) pair count reported by the most recent draw whose compositing has STARTED on the GPU (its first
 * workgroup stores the count into host-visible memory; 0 before any) and the capacity of the pair buffers.  tile_pairs > pair_capacity:
 * that draw dropped its farthest pairs (the next gs_renderer_draw grows the buffers; gs_renderer_frame_stats reports the frame). */
int32_t gs_renderer_poll_pairs(gs_renderer* r, uint64_t* tile_pairs, uint64_t* pair_capacity);
/* blocking readbacks (parity hooks; synchronise the stream) */
int32_t gs_renderer_download_order(gs_renderer* r, uint32_t* out, size_t count);        /* _OrderBuffer / m_GpuSortKeys */
int32_t gs_renderer_download_distances(gs_renderer* r, uint32_t* out, size_t count);    /* m_GpuSortDistances: the sorted keys of the last gs_renderer_sort
                                                                                           (also after a later upload_order / reset_order, as in the reference) */
int32_t gs_renderer_upload_order(gs_renderer* r, const uint32_t* in, size_t count);
/* GS_SORT_VISIBLE parity hook: the depth-ordered splat indices the last draw was binned from (the visible subsequence of the reference's
 * _OrderBuffer); *count = V, at most `capacity` entries are written.  (gs_renderer_download_order in this mode carries the recorded sorts
 * out on all N first: one full sort + the chain fix-up.)  Blocks. */
int32_t gs_renderer_download_visible_order(gs_renderer* r, uint32_t* out, size_t capacity, uint32_t* count);
int32_t gs_renderer_download_view(gs_renderer* r, void* out, size_t bytes);             /* N x 40 B SplatViewData */
/* What the last gs_renderer_calc_view left for the compositor (the per-frame launch, NOT the on-demand full kernel), in
 * splat-index order; any pointer may be NULL:
 *   recs      N x 32 B  {cx, cy, axis1.xy, axis2.xy (float, pixels, y down), f16 r<<16|g, f16 b<<16|a}; only meaningful where visible
 *   rects     N x 2 u32 {x0 | y0 << 16, (x1 + 1) | (y1 + 1) << 16}: the footprint's inclusive pixel rectangle clamped to the screen; 0,0 = not drawn
 *   vis_mask  ceil(N/64) u64, bit s = splat s reaches at least one tile */
int32_t gs_renderer_download_raster_records(gs_renderer* r, void* recs, uint32_t* rects, uint64_t* vis_mask);
int32_t gs_renderer_frame_stats(gs_renderer* r, gs_frame_stats* out);                   /* blocks; reports + clears overflow/timeouts */
int32_t gs_renderer_stage_times(gs_renderer* r, gs_stage_times* out);                   /* blocks; resets the ring */
/* per-frame GPU durations (first kernel of the frame to the end of the blend, ms) of the frames in the profiling ring;
 * call before gs_renderer_stage_times.  Blocks. */
int32_t gs_renderer_frame_times(gs_renderer* r, float* out_ms, int32_t capacity, int32_t* count);

/* ---- render target: the _GaussianSplatRT temporary (GaussianSplatRenderer.cs:194-196) ------------- */
int32_t gs_target_create(gs_context* ctx, uint32_t width, uint32_t height, gs_target** out);
int32_t gs_target_destroy(gs_target* t);
int32_t gs_target_clear(gs_target* t);                                  /* ClearRenderTarget(Color, (0,0,0,0)) */
/* The depth attachment of the splat RT: the reference binds the camera's depth buffer next to it (SetRenderTarget(
 * GaussianSplatRT, CurrentActive), GaussianSplatRenderer.cs:195; URP: activeDepthTexture, GaussianSplatURPFeature.cs:54-66)
 * and draws the splats with ZTest LEqual, ZWrite Off (RenderGaussianSplats.shader:10), so opaque scene geometry occludes
 * them.  `depth` = W*H floats, row 0 = top: the VIEW depth (clip.w, in world units along the camera axis) of the opaque
 * scene at each pixel (+inf where there is none); a splat fragment survives iff the splat's centre depth <= it (all four
 * vertices of a splat quad share the centre's depth).  memory_kind 0: host memory, copied (stream-ordered);
 * 1: device memory, BORROWED until the next call.  NULL: no depth attachment (default). */
int32_t gs_target_set_scene_depth(gs_target* t, const float* depth, int32_t memory_kind);
int32_t gs_target_download(gs_target* t, void* out_rgba16f, size_t bytes);   /* W*H*8 B, row 0 = top; blocks */
/* GaussianComposite.shader:25-39 + its "Blend SrcAlpha OneMinusSrcAlpha": out = lerp(bg, GammaToLinearSpace(C/A), A).
 * Writes W*H*4 floats (linear RGBA; out.a = A*A + bg.a*(1-A): the pass has no separate alpha blend factors) into a device buffer owned by the target, then
 * optionally copies it to `out_rgba32f` (may be NULL) and/or an sRGB-encoded 8-bit image `out_rgba8` (may be NULL). */
int32_t gs_target_resolve(gs_target* t, const float background_rgba[4], float* out_rgba32f, uint8_t* out_rgba8);
int32_t gs_target_device_ptr(gs_target* t, void** rgba16f_dev, void** resolved_rgba32f_dev);
/* enabled != 0: every gs_target_resolve is bracketed by hipEvents on the context's stream (a ring of 64);
 * gs_target_resolve_time blocks, returns the mean GPU duration (ms) of the resolves recorded since the last call and resets. */
int32_t gs_target_set_profiling(gs_target* t, int32_t enabled);
int32_t gs_target_resolve_time(gs_target* t, float* mean_ms, int32_t* count);

/* ---- pick output: per-pixel surface depth and splat id from the blend  (additions to ABI 9) ------------------------
 * The reference draws the splats with ZWrite Off: nothing after the draw knows where the splat surface is.  With pick output on, the splat
 * blend also leaves one 16-byte record per pixel of the target.  The ACCUMULATED ALPHA of a pixel is the blend's own accumulator (the fp16
 * alpha after every ROP step in exact mode, the fp32 one in fast mode); a pixel is CROSSED by the first live fragment whose blend takes it
 * from < threshold to >= threshold; the record holds that fragment's splat index in the asset, that splat's view depth clip.w (the bits
 * gs_renderer_calc_view culled and drew it with) and the tag of the renderer that drew it.  A pixel never crossed holds
 * { +inf, 0xFFFFFFFF, 0, 0 }.  gs_target_clear resets every record (folded into the next draw like the pixel clear).  A draw into a target
 * that already holds pixels starts from the stored alpha: it leaves an existing record alone and writes a pixel's record only if it is the
 * draw that crosses it, so several renderers (distinct tags) can share one target.  Pixels are the same bits with pick output on or off.
 * Only GS_RENDER_SPLATS draws write records: gs_renderer_draw in a debug render mode into a target with pick output on returns
 * GS_ERR_INVALID_ARGUMENT. */
typedef struct gs_pick_record {
    float depth;        /* view depth (clip.w) of the crossing splat; +inf = none */
    uint32_t splat;     /* its index in the asset; 0xFFFFFFFF = none */
    uint32_t tag;       /* gs_renderer_set_pick_tag of the renderer that drew it */
    uint32_t zero;
} gs_pick_record;
/* enabled != 0: allocates the records (all "none") and sets the threshold, 0 < threshold <= 1 (else GS_ERR_INVALID_ARGUMENT, nothing changed);
 * a target that is already on only takes the new threshold.  0: frees them.  A target of a context with lanes
 * (gs_renderer_set_frames_in_flight) doubles the records exactly as it doubles its pixels. */
int32_t gs_target_set_pick_output(gs_target* t, int32_t enabled, float threshold);
int32_t gs_target_download_pick(gs_target* t, void* out, size_t bytes);   /* exactly W*H*16 B, row 0 = top; blocks */
int32_t gs_target_pick_at(gs_target* t, uint32_t x, uint32_t y, gs_pick_record* record_out);   /* one record; blocks; x >= W or y >= H: invalid argument */
/* the device pointer of the records (W*H x 16 B); marks the target exposed, as gs_target_device_ptr does */
int32_t gs_target_pick_device_ptr(gs_target* t, void** pick_dev);
/* the tag this renderer's draws write (default 0); a plain setting, shared by the lanes of gs_renderer_set_frames_in_flight */
int32_t gs_renderer_set_pick_tag(gs_renderer* r, uint32_t tag);
/* Select what one SEES: for every pixel of the inclusive rectangle (x0, y0) .. (x1, y1) (pixels, y down, clipped to the target) whose record
 * carries this renderer's tag and a splat < N that is neither deleted nor cut by the renderer's current cutouts, set that splat's bit in
 * `selected` (subtract != 0: clear it).  A click is a 1x1 rectangle.  Asynchronous on the context's stream, ordered after the target's last
 * use; gs_renderer_edit_info then reports the new counts and bounds.  x0 > x1 or y0 > y1, or a target without pick output: invalid argument. */
int32_t gs_renderer_edit_select_surface(gs_renderer* r, gs_target* t, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t subtract);

/* ---- floaters: splats with few neighbours, counted on a grid on the GPU  (additions to ABI 9) -----------------------------
 * The isolated splats training leaves in empty space lie in front of and behind everything: neither selection tool above reaches them.
 * The contract, operation by operation:
 *   ALIVE      a splat whose index is < N, that is not deleted and not cut by the renderer's current cutouts (the test of every edit call).
 *   POSITIONS  object-space positions as the renderer decodes them, any preset; the renderer's private copy where a transform or a merge
 *              made one.  `radius` is in that space.
 *   N(i, j)    all in fp32, nothing fused: dx = xj - xi, dy, dz likewise; d2 = (dx dx + dy dy) + dz dz; r2 = radius radius; N holds when
 *              d2 <= r2 (the boundary included).  Every comparison with NaN is false: a splat whose position is not finite is nobody's
 *              neighbour and has none.
 *   count(i)   the alive j != i for which N(i, j) holds.  Splats at identical positions are neighbours of one another.
 * gs_renderer_edit_neighbour_counts writes min(count(i), cap) for every alive splat and 0xFFFFFFFF for every other one into counts_out
 * (`count` words, which must be N) and changes nothing on the renderer.
 * gs_renderer_edit_select_sparse: splat i is SPARSE if it is alive and count(i) < min_neighbours (so an alive splat with a non-finite position
 * is sparse whenever min_neighbours > 0, and min_neighbours = 0 selects nothing).  subtract == 0: selected |= sparse; else selected &= ~sparse
 * -- on the current selection, as gs_renderer_edit_select_surface.  No bit at or beyond N is ever set.  It makes the edit buffers if there
 * are none, is a selection change to the edit history (undo and redo cover it) and keeps a highlighted selection's lanes in step.  The walk
 * stops counting for a splat at min_neighbours (at cap): a dense core is cheap.
 * Refused with GS_ERR_INVALID_ARGUMENT, nothing changed and nothing left allocated: a NULL argument, a lane, a radius that is not finite or
 * outside [1e-15, 1e15], cap == 0, count != N.  A renderer without an alive splat is no error (all 0xFFFFFFFF; nothing selected).
 * Both calls BLOCK, as the bake does: they wait for everything enqueued on the context (their sorts want the GPU to themselves), allocate
 * transient buffers and free them before they return.  A sort whose bounded look-back spin expired: GS_ERR_SORT_TIMEOUT, selection unchanged. */
int32_t gs_renderer_edit_neighbour_counts(gs_renderer* r, float radius, uint32_t cap, uint32_t* counts_out, size_t count);
int32_t gs_renderer_edit_select_sparse(gs_renderer* r, float radius, uint32_t min_neighbours, int32_t subtract);

/* ---- islands: the connected components of the neighbour graph, on the GPU  (additions to ABI 9) ---------------------------------
 * A clump of floaters has plenty of neighbours inside itself: no min_neighbours above selects it.  It is a SMALL CONNECTED COMPONENT of
 * the graph whose vertices are the alive splats and whose edges are N(i, j); a whole object is a large one.  ALIVE, POSITIONS, N(i, j)
 * and the radius refusals are the floater block's, word for word; N is symmetric in fp32.
 *   COMPONENT  a class of the transitive closure of N over the alive splats.  An alive splat whose position is not finite has no edges
 *              and is a component of its own.
 *   label(i)   the smallest splat index in i's component.
 *   size(i)    the number of splats in i's component.
 * Both are unique whatever order the GPU links in.
 * gs_renderer_edit_components writes label(i) into labels_out and size(i) into sizes_out for every alive splat, 0xFFFFFFFF and 0 for
 * every other one (`count` words each, which must be N; either pointer may be NULL, not both) and changes nothing on the renderer.
 * gs_renderer_edit_select_islands: splat i is an ISLAND if it is alive and size(i) < min_size.  subtract == 0: selected |= island; else
 * selected &= ~island -- on the current selection.  min_size 0 or 1 selects nothing and is no error (as min_neighbours == 0 above);
 * min_size 2 sets exactly the words gs_renderer_edit_select_sparse(radius, 1) sets.
 * gs_renderer_edit_grow_selection: a SEED is an alive splat with index < N whose selected bit is set; every alive splat of a component
 * that holds a seed is added to the selection.  It never clears a bit and never sets one at or beyond N; an empty selection stays empty.
 * Both selecting calls make the edit buffers if there are none, are one selection change to the edit history (undo and redo cover them)
 * and keep a highlighted selection's lanes in step.
 * Refused with GS_ERR_INVALID_ARGUMENT, nothing changed and nothing left allocated: a NULL renderer, both outputs NULL, a lane, a radius
 * that is not finite or outside [1e-15, 1e15], count != N.  A renderer without an alive splat is no error.
 * All three calls BLOCK exactly as the two above do; a sort whose bounded look-back spin expired: GS_ERR_SORT_TIMEOUT, selection unchanged. */
int32_t gs_renderer_edit_components(gs_renderer* r, float radius, uint32_t* labels_out, uint32_t* sizes_out, size_t count);
int32_t gs_renderer_edit_select_islands(gs_renderer* r, float radius, uint32_t min_size, int32_t subtract);
int32_t gs_renderer_edit_grow_selection(gs_renderer* r, float radius);

/* ---- select by attribute: opacity, size, position and colour ranges, and the numbers a histogram panel shows  (additions to ABI 9) ----
 * The tools above select by where a splat is or what is seen; these select by what a splat IS.  The contract, operation by operation
 * (DESIGN.md section 4.19); every result is an exact integer or an exact float bit pattern:
 *   ALIVE      a splat whose index is < N, that is not deleted and not cut by the renderer's current cutouts (the floater block's definition).
 *   FIELDS     LoadSplatData's decoded fields of the renderer's CURRENT blobs, any preset (the private copies where a transform or a merge
 *              made them): the object-space position p; the linear scale s, after the chunk de-normalisation and the three squarings; the
 *              linear opacity o, after InvSquareCentered01; the DC colour c, the de-normalised texel rgb.
 *   value      fp32 throughout, nothing fused, denormals kept, every comparison with NaN false:
 *                GS_ATTR_OPACITY    o
 *                GS_ATTR_SCALE_MAX  fmaxf(fmaxf(s.x, s.y), s.z)      GS_ATTR_SCALE_MIN  fminf(fminf(s.x, s.y), s.z)
 *                                   (a NaN operand is ignored; of +0 and -0 the first operand is returned)
 *                GS_ATTR_VOLUME     (s.x * s.y) * s.z
 *                GS_ATTR_POS_X, _Y, _Z   p.x, p.y, p.z
 *                GS_ATTR_DIST2      dx = p.x - q.x, dy, dz likewise; (dx dx + dy dy) + dz dz -- the sphere tool, N(i, j)'s d2 form.  q = point,
 *                                   in object space: read for this attribute only, where it must be non-NULL and finite; otherwise ignored
 *                GS_ATTR_COLOR_R, _G, _B   c.x, c.y, c.z
 *                GS_ATTR_LUMA       (0.299f c.x + 0.587f c.y) + 0.114f c.z: three products and two sums, each rounded
 *              The sign and payload of a NaN value carry no meaning.
 *   KEY        FloatToSortableUint of the value (the bits with the sign bit flipped, or all of them for a negative value): a total order, -0 before +0.
 *   SCOPE      GS_SCOPE_ALIVE: the alive splats.  GS_SCOPE_SELECTED: those of them whose selected bit is set (index < N: the tail bits that
 *              select-all sets beyond N never count); empty for a renderer without edit buffers.
 * gs_renderer_edit_attribute_values writes the value's bits for every alive splat and the word 0xFFFFFFFF for every other one into values_out
 * (`count` floats, which must be N).  Changes nothing; blocks.
 * gs_renderer_edit_select_range: splat i is IN if it is alive and lo <= v && v <= hi.  subtract == 0: selected |= in; else selected &= ~in --
 * on the current selection.  lo = -inf and hi = +inf are allowed; lo > hi selects nothing and is no error.  No bit at or beyond N is ever
 * set.  It makes the edit buffers if there are none, is one selection change to the edit history (undo and redo cover it), keeps a
 * highlighted selection's lanes in step, needs no sort and is asynchronous on the context's stream, like gs_renderer_edit_update_selection.
 * gs_renderer_edit_attribute_stats: members = the size of the scope, nans = its members whose value is NaN, vmin / vmax = the values that
 * are not NaN with the smallest / largest KEY; +inf / -inf if there is none.  Blocks.
 * gs_renderer_edit_attribute_histogram: hist_out takes bins + 3 words (`count` must be that).  With w = hi - lo and s = (float) bins / w, both
 * in fp32 and computed once: a NaN member is counted in hist[bins + 2], one with v < lo in hist[bins], one with v > hi in hist[bins + 1], every
 * other in hist[min(bins - 1, (uint32_t) ((v - lo) * s))] -- one subtraction and one product, each rounded, then truncation.  The words sum
 * to the scope's members.  Refused unless 1 <= bins <= 4096, lo and hi are finite, lo < hi and w and s are finite.  Blocks.
 * gs_renderer_edit_attribute_ranks: the POPULATION is the scope's members whose value is not NaN; *population is their number.  Their KEYs
 * sorted ascending (unique: keys alone), values_out[k] is the value at position ranks[k], the word 0xFFFFFFFF where ranks[k] >= population.
 * rank_count <= 4096; rank_count == 0 with NULL arrays returns the population alone.  It BLOCKS exactly as the floater calls do (it waits
 * for the context, takes transient buffers and frees them before it returns); a sort whose bounded look-back spin expired:
 * GS_ERR_SORT_TIMEOUT, nothing written.
 * All five are refused with GS_ERR_INVALID_ARGUMENT, nothing changed and nothing left allocated: a NULL renderer or a NULL required output,
 * a lane, an unknown attribute or scope, a wrong count, a NaN lo or hi, a NULL or non-finite point for GS_ATTR_DIST2.  A renderer without an
 * alive splat is no error. */
typedef enum gs_splat_attribute {
    GS_ATTR_OPACITY = 0,
    GS_ATTR_SCALE_MAX = 1,
    GS_ATTR_SCALE_MIN = 2,
    GS_ATTR_VOLUME = 3,
    GS_ATTR_POS_X = 4,
    GS_ATTR_POS_Y = 5,
    GS_ATTR_POS_Z = 6,
    GS_ATTR_DIST2 = 7,
    GS_ATTR_COLOR_R = 8,
    GS_ATTR_COLOR_G = 9,
    GS_ATTR_COLOR_B = 10,
    GS_ATTR_LUMA = 11
} gs_splat_attribute;
typedef enum gs_attribute_scope { GS_SCOPE_ALIVE = 0, GS_SCOPE_SELECTED = 1 } gs_attribute_scope;
typedef struct gs_attribute_stats { uint32_t members, nans; float vmin, vmax; } gs_attribute_stats;
int32_t gs_renderer_edit_attribute_values(gs_renderer* r, int32_t attr, const float point[3], float* values_out, size_t count);
int32_t gs_renderer_edit_select_range(gs_renderer* r, int32_t attr, const float point[3], float lo, float hi, int32_t subtract);
int32_t gs_renderer_edit_attribute_stats(gs_renderer* r, int32_t attr, const float point[3], int32_t scope, gs_attribute_stats* out);
int32_t gs_renderer_edit_attribute_histogram(gs_renderer* r, int32_t attr, const float point[3], int32_t scope, float lo, float hi, uint32_t bins,
                                             uint32_t* hist_out, size_t count);
int32_t gs_renderer_edit_attribute_ranks(gs_renderer* r, int32_t attr, const float point[3], int32_t scope, const uint32_t* ranks, uint32_t rank_count,
                                         float* values_out, uint32_t* population);

/* ---- lasso, polygon and brush: selecting through a screen mask  (additions to ABI 9) ---------------------------------------------------
 * A MASK is one bit per pixel of a W x H screen, 1 <= W, H <= 65535, owned by a context.  Row 0 = top, y down, x right: the convention of the
 * pick records.  A row is ceil(W/32) words; bit x & 31 of word x >> 5 is pixel x; the bits beyond W in a row's last word are zero after every
 * call.  Every call that changes a mask -- clear, upload, the drawing calls -- and the two selecting calls are asynchronous on the context's
 * stream, and a caller's array is only read during the call (it is copied); the download blocks.  word_count is H * ceil(W/32), exactly.
 * The contract of the two drawing calls, operation by operation.  All arithmetic is fp32 and every + - x / rounds
 * once; the centre of pixel (x, y) is c = ((float)x + 0.5f, (float)y + 0.5f).  `xy` is a host array of pixel coordinates in the mask's frame
 * (x0 y0 x1 y1 ...), copied by the call.  subtract == 0: the covered pixels are set; else they are cleared.
 *   POLYGON  3 <= vertices <= 65536; edge i runs from vertex i to vertex (i + 1) mod V; the lasso is filled by the even-odd rule.  On the row
 *            with yc = y + 0.5f the edge (a -> b) CROSSES iff (a.y <= yc) != (b.y <= yc); its crossing abscissa is
 *            xs = a.x + ((yc - a.y) * (b.x - a.x)) / (b.y - a.y); a crossing toggles every pixel of the row with c.x < xs; a pixel is covered
 *            iff it was toggled an odd number of times.  A vertex on a row's centre line belongs to the half plane above it, and a horizontal
 *            edge never crosses.
 *   STROKE   1 <= points <= 65536, 0 < radius <= 65536: the round-capped polyline through the points, one point being a disc.  For a segment
 *            (a -> b), a == b for a single point:  d = b - a, e = c - a, len2 = d.x d.x + d.y d.y;  t = 0 if len2 == 0, else
 *            min(max((e.x d.x + e.y d.y) / len2, 0), 1);  q = e - t d (the product rounds, then the difference);  d2 = q.x q.x + q.y q.y.
 *            The pixel is covered iff d2 <= radius radius for any segment.
 * Refused with GS_ERR_INVALID_ARGUMENT and nothing changed: a NULL argument, a coordinate that is NaN, infinite or beyond 65536 in magnitude,
 * a count outside the limits above, a radius that is not in (0, 65536], a wrong word_count. */
typedef struct gs_mask gs_mask;
int32_t gs_mask_create(gs_context* ctx, uint32_t width, uint32_t height, gs_mask** out);      /* every bit zero */
int32_t gs_mask_destroy(gs_mask* m);
int32_t gs_mask_clear(gs_mask* m);
int32_t gs_mask_upload(gs_mask* m, const uint32_t* words, size_t word_count);                 /* bits beyond W are masked off */
int32_t gs_mask_download(gs_mask* m, uint32_t* words, size_t word_count);                     /* blocks */
int32_t gs_mask_fill_polygon(gs_mask* m, const float* xy, uint32_t vertices, int32_t subtract);
int32_t gs_mask_stroke(gs_mask* m, const float* xy, uint32_t points, float radius, int32_t subtract);
/* The lasso counterpart of gs_renderer_edit_update_selection, with the same gesture contract: selected = the mouse-down copy, plus (subtract != 0:
 * minus) the splats the mask hits, every word written once; the host calls gs_renderer_edit_store_selection at mouse-down and this on every
 * mouse move.  The test of one splat is the rectangle tool's up to its pixel position (not cut, clip w > 0, px and py from the same
 * expressions, py counting up from the bottom edge); then it is a hit iff px >= 0 && px < W && py >= 0 && py < H and bit
 * ((uint)px, H - 1 - (uint)py) of the mask is set.  A splat whose pixel position is NaN therefore hits NOTHING: deliberately not the quirk of
 * the rectangle tool, where such a splat is inside every rectangle.  Deleted bits play no part, as there.
 * Refused with GS_ERR_INVALID_ARGUMENT, nothing changed and no edit buffers made: a NULL argument, p->screen_w != (float)W or
 * p->screen_h != (float)H, a mask of another context. */
int32_t gs_renderer_edit_update_selection_mask(gs_renderer* r, const gs_frame_params* p, gs_mask* m, int32_t subtract);
/* gs_renderer_edit_select_surface over every pixel whose mask bit is set, in place of a rectangle: the same record test (tag, splat < N, not
 * deleted, not cut), on the current selection, ordered after the target's last use.  The mask must have the target's size and context; a
 * target without pick output is refused as there. */
int32_t gs_renderer_edit_select_surface_mask(gs_renderer* r, gs_target* t, gs_mask* m, int32_t subtract);

/* ---- native importer (host code; no GPU needed, one optional GPU stage): GaussianSplatAssetCreator.CreateAsset minus the Unity asset database -- */
/* InputSplatData (GaussianFileReader.cs:17-26) as separate arrays, in the PLY domain after ReorderSHs: */
typedef struct gs_import_input {
    uint32_t splat_count;
    const float* pos;       /* N x 3 */
    const float* dc0;       /* N x 3   f_dc_0..2 (raw SH0) */
    const float* sh;        /* N x 45  15 coefficients x rgb (ReorderSHs layout, GaussianFileReader.cs:186-208) */
    const float* opacity;   /* N       logit */
    const float* scale;     /* N x 3   log-scale */
    const float* rot;       /* N x 4   rot_0..3 = (w, x, y, z) */
} gs_import_input;
typedef struct gs_import_formats {
    uint32_t pos_format, scale_format, color_format, sh_format;   /* gs_vector_format x2, gs_color_format, gs_sh_format */
    uint32_t linearize;     /* 1: apply LinearizeData (GaussianFileReader.cs:211-233); 0: the arrays are already linear
                               (dc0 = colour, opacity in 0..1, scale linear, rot = packed smallest-3 + index/3) */
    uint32_t morton;        /* 1: reorder by the 63-bit Morton code of the position (GaussianSplatAssetCreator.cs:362-429) */
} gs_import_formats;
/* byte sizes of the pos, other, color, sh, chunk blobs (chunk = 0 for an all-fp32 asset; every format incl. BC7 and Cluster*) */
int32_t gs_import_blob_sizes(uint32_t splat_count, const gs_import_formats* formats, uint64_t sizes[5]);
/* encodes into caller-owned host buffers of at least those sizes (blobs[4] may be NULL when sizes[4] == 0);
 * bounds_min/max (may be NULL) receive the position bounds (GaussianSplatAsset.boundsMin/Max). */
int32_t gs_import_encode(const gs_import_input* in, const gs_import_formats* formats, void* const blobs[5], const uint64_t sizes[5],
                         float bounds_min[3], float bounds_max[3]);
/* The one stage of the importer that can run on a GPU: the nearest-mean assignment of the Cluster* SH palette
 * (GaussianSplatAssetCreator.cs:476-518), n x k x 45 multiply-adds in double, five passes per import.  Host and GPU perform the same
 * operations in the same order -- dot = dot + (double)x[i][c] * (double)means[j][c] for c = 0..44, product and sum each rounded to double
 * (no FMA), d_j = |means[j]|^2 - 2 dot, index = 0 if d_0 is NaN, else the smallest j attaining the minimum over the non-NaN d_j -- so the
 * indices, and with them the asset's bytes, are identical wherever the assignment ran.  There is no host fallback: a HIP failure is
 * GS_ERR_HIP / GS_ERR_OUT_OF_MEMORY.  The work goes on the context's stream; the means are uploaded once per call and the points pass through
 * a device buffer of fixed size in batches (GSPLAT_IMPORT_BATCH = points per batch, read at every call, overrides the size). */
/* nearest-mean assignment of n 45-float vectors to k means; ctx NULL = the host loop, else the context's GPU. Blocks. */
int32_t gs_import_assign_clusters(gs_context* ctx, const float* x, uint64_t n, const float* means, uint32_t k, uint32_t* index_out);
/* The whole palette of the Cluster* SH formats for n 45-float vectors (cluster_shs of the importer: GaussianSplatAssetCreator.cs:476-518 minus its
 * RNG): seeds means[j] = x[(j n) / k]; training subset = all of x when n <= 200,000, else x[(i n) / 200,000]; four Lloyd passes on the subset --
 * the assignment above, then for every cluster with points and every coefficient sum = sum + (double)x[p][c] over its points in ascending point
 * index from 0.0, mean = (float)(sum / (double)count), an empty cluster keeping its mean; one assignment pass over all n.  means_out: k x 45,
 * index_out: n.  ctx NULL: the host loop.  Otherwise the whole loop runs on the context's GPU (points up once, means and indices down at the end;
 * csrc/gs_cluster.hip) and gives the same bits for finite input: a NaN a sum produces has no fixed sign or payload across the two.
 * k in [1, 65536], n >= 1; n <= k is allowed (the seeds repeat).  Blocks. */
int32_t gs_import_cluster_shs(gs_context* ctx, const float* x, uint64_t n, uint32_t k, float* means_out, uint32_t* index_out);
/* gs_import_encode with the Cluster* assignment passes on ctx's GPU (ctx NULL: identical to gs_import_encode) */
int32_t gs_import_encode_on(gs_context* ctx, const gs_import_input* in, const gs_import_formats* formats,
                            void* const blobs[5], const uint64_t sizes[5], float bounds_min[3], float bounds_max[3]);

/* ---- bake: an edited renderer back into a compressed asset, on the GPU (EditExportData + CreateAsset in one step) ----------------------
 * The alive splats of r -- idx < N, not deleted, not cut by the current cutout list: ExportPlyFile's rule, GaussianSplatRendererEditor.cs:414-442 --
 * decoded from whatever r holds (any preset, private blobs or the asset's) and encoded in `formats`, Morton-reordered and chunked as
 * GaussianSplatAssetCreator does it: the five blobs are the bytes gs_import_encode (linearize = 0) makes of the same splats in index order.
 * Runs on the context's stream after everything already enqueued there and on the lanes; only reads the renderer.
 * A GS_SH_CLUSTER* target gets the importer's palette of the alive splats' SH, computed on the GPU (gs_import_cluster_shs' loop on device
 * pointers); those bytes are the importer's for finite SH values.
 * Refused with GS_ERR_INVALID_ARGUMENT, nothing allocated and *out NULL: a NULL argument, a lane, a format enum out of range, linearize != 0,
 * no alive splat, a GS_SH_CLUSTER* target with no more alive splats than table entries (gs_import_blob_sizes' rule), a GS_COLOR_BC7 target --
 * hence the preset VeryLow as a whole; VeryLow with another colour format is accepted (any preset is accepted as the source). */
/* formats->linearize must be 0 (the renderer's data is linear); formats->morton 0 or 1.  BLOCKS.  *out is a new asset owned by r's
 * context (gs_asset_destroy); *alive its splat count; bounds as GaussianSplatAsset.boundsMin/Max (may be NULL). */
int32_t gs_renderer_edit_bake_asset(gs_renderer* r, const gs_import_formats* formats, gs_asset** out, uint32_t* alive,
                                    float bounds_min[3], float bounds_max[3]);
/* ---- import on the GPU: raw splat arrays to a device-resident asset, every preset (GaussianSplatAssetCreator's whole pipeline on the context's GPU) --
 * The six arrays of `in` -- memory_kind 0: host memory, copied into transient device buffers (N x 236 bytes); memory_kind 1: device memory on the
 * context's GPU, 4-byte aligned, read during the call only and not modified -- linearised (formats->linearize = 1), bounded, Morton-reordered
 * (formats->morton = 1), chunked and encoded into a new immutable asset owned by ctx: exactly what gs_renderer_edit_bake_asset returns, for
 * gs_renderer_create, gs_asset_download_blobs, gs_asset_info and gs_asset_destroy.  Nothing but the upload of memory_kind 0 is host work.
 * THE IMPORTER'S BYTES: the five blobs, over gs_import_blob_sizes bytes each, are what gs_import_encode(in, formats, ...) writes for the same input --
 * pad bytes, texels past N, the last chunk's tail and every BC7 block of the colour texture included (GS_COLOR_BC7 is accepted here: mode-6 blocks,
 * the tiles past the last chunk holding the encoding of an all-zero block) -- and the bounds match bit for bit, for every value of the four format
 * enums, linearize 0 and 1, morton 0 and 1.  Premises: the input is finite; with linearize = 0 the rot values lie inside their field ranges
 * ([0, 1]: the host's conversion of anything else is undefined); no -0 is an extreme of a chunk column or of a bounds axis (fmin / fmax do not
 * pin the sign of zero among equal values); a GS_SH_CLUSTER* palette has finite SH (gs_import_cluster_shs' limit).
 * Runs on the context's stream after gs_context_synchronize: its sorts need the GPU the way the bake's do.  BLOCKS.
 * Refused with GS_ERR_INVALID_ARGUMENT, *out NULL and nothing left allocated: a NULL ctx, in, formats or out; a NULL array; splat_count == 0; a
 * format enum out of range; linearize > 1 or morton > 1; memory_kind > 1; a GS_SH_CLUSTER* target with no more splats than table entries
 * (gs_import_blob_sizes' rule).  bounds_min / bounds_max may be NULL. */
int32_t gs_import_encode_to_asset(gs_context* ctx, const gs_import_input* in, uint32_t memory_kind, const gs_import_formats* formats, gs_asset** out,
                                  float bounds_min[3], float bounds_max[3]);
/* the five blobs of any asset to host memory: sizes[k] bytes of blob k, at most what the asset holds (blobs[k] NULL or sizes[k] 0: skipped).  BLOCKS. */
int32_t gs_asset_download_blobs(const gs_asset* asset, void* const blobs[5], const uint64_t sizes[5]);

/* PLY input (PLYFileReader.cs:25-76 header rules; GaussianFileReader.cs:80-208 attribute mapping + ReorderSHs): binary
 * little-endian, float properties; x y z f_dc_0..2 opacity scale_0..2 rot_0..3 required, f_rest_* optional (0 if absent).
 * The arrays gs_ply_arrays points `out` at are owned by the handle and valid until gs_ply_close. */
typedef struct gs_ply gs_ply;
int32_t gs_ply_open(const char* path, gs_ply** out, uint32_t* splat_count);
/* SPZ input (Niantic / Scaniverse .spz; SPZFileReader.cs:26-198): gzip stream, version 2, <= 10 M points.  Same handle type
 * and accessors as the PLY reader, but the arrays are ALREADY LINEAR (UnpackDataJob applies LinearScale, SH0ToColor and
 * PackSmallest3Rotation): pass them to gs_import_encode with formats.linearize = 0. */
int32_t gs_spz_open(const char* path, gs_ply** out, uint32_t* splat_count);
int32_t gs_ply_arrays(const gs_ply* ply, gs_import_input* out);
int32_t gs_ply_close(gs_ply* ply);

/* ---- a PLY or SPZ file straight into a device asset on the GPU (additions to ABI 9) ------------------------------------------------------
 * gs_splat_file_open reads and checks the file the way gs_ply_open / gs_spz_open do -- the same header rules, the same error code and the same
 * gs_last_error_string text for every file either of them refuses -- but builds no arrays: of a PLY it keeps the stream, positioned at the vertex
 * rows, after holding the file's length against splat_count x stride; of an SPZ the gunzipped stream in host memory.  Host only: no GPU is touched.
 * The kind is chosen by the path's extension, .ply / .spz in any letter case (GaussianFileReader.ReadFile); any other is GS_ERR_INVALID_ASSET.
 * offsets[]: where in a vertex row each float property lies, in bytes: x y z, f_dc_0..2, opacity, scale_0..2, rot_0..3, f_rest_0..44 -- the 59 the
 * importer reads -- then nx ny nz, which it does not; -1 = absent (a f_rest_k then reads as 0).  The file's own order: properties may come in any
 * order with foreign ones between them.  An SPZ has stride 0 and every offset -1. */
#define GS_SPLAT_FILE_PLY 1u
#define GS_SPLAT_FILE_SPZ 2u
typedef struct gs_splat_file gs_splat_file;
typedef struct gs_splat_file_info {
    uint32_t kind;          /* GS_SPLAT_FILE_PLY / GS_SPLAT_FILE_SPZ */
    uint32_t splat_count;
    uint32_t stride;        /* PLY: bytes per vertex row */
    uint32_t sh_level;      /* SPZ: 0..3 */
    uint32_t fract_bits;    /* SPZ: 0..24 */
    uint32_t reserved;
    uint64_t body_bytes;    /* what goes to the GPU: PLY splat_count x stride; SPZ the header + the six columns of the gunzipped stream */
    int32_t offsets[62];
} gs_splat_file_info;
int32_t gs_splat_file_open(const char* path, gs_splat_file** out, gs_splat_file_info* info /* may be NULL */);
int32_t gs_splat_file_close(gs_splat_file* file);
/* The file's bytes to the GPU and from there to a new asset owned by ctx, with the rows / columns themselves as the importer's source: the asset --
 * five blobs and bounds -- that gs_import_encode_to_asset makes of gs_ply_open / gs_spz_open + gs_ply_arrays of the same file, byte for byte, under
 * that function's premises.  formats->linearize must be the kind's value, 1 for a PLY and 0 for an SPZ.
 * A PLY's rows go to one transient device buffer of body_bytes through two pinned slices of slice_bytes (0 = 64 MiB; never more than the body
 * needs), filled alternately: the file is read into one while the other's copy is in flight, so the host holds two slices whatever the file's
 * size.  An SPZ's gunzipped stream is uploaded as it is.  A file that ends early is gs_ply_open's "fewer data bytes" error.
 * The handle may be imported any number of times.  BLOCKS; runs on the context's stream after gs_context_synchronize.
 * Refused with GS_ERR_INVALID_ARGUMENT, *out NULL and nothing left allocated: a NULL ctx, file, formats or out; a handle that is not open; a
 * linearize of the other kind; morton > 1; slice_bytes in 1..4095; whatever gs_import_blob_sizes refuses. */
int32_t gs_import_file_to_asset(gs_context* ctx, gs_splat_file* file, const gs_import_formats* formats, uint32_t slice_bytes, gs_asset** out,
                                float bounds_min[3], float bounds_max[3]);

/* ---- stand-alone sorter: GpuSorting (GpuSorting.cs) ----------------------------------------------- */
/* SupportResources.Load(count) :48-63 */
int32_t gs_sorter_create(gs_context* ctx, uint32_t max_count, gs_sorter** out);
int32_t gs_sorter_destroy(gs_sorter* s);
/* Dispatch :142-198 -- stable ascending sort of (uint32 key, uint32 payload) pairs in DEVICE buffers, in place
 * (KEY_UINT PAYLOAD_UINT SHOULD_ASCEND SORT_PAIRS).  key_bits in [1,32]: only the low key_bits take part. */
int32_t gs_sorter_dispatch(gs_sorter* s, void* keys_dev, void* values_dev, uint32_t count, uint32_t key_bits);
/* same on host arrays (upload, sort, download); blocks */
int32_t gs_sorter_sort_host(gs_sorter* s, uint32_t* keys, uint32_t* values, uint32_t count, uint32_t key_bits);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_C_H */
