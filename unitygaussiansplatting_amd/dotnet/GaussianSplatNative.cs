// SPDX-License-Identifier: MIT
// GaussianSplatNative.cs -- the reference-side binding a maintainer adds to use libgsplat_hip.so from the C# host.
//
// This is SOURCE ONLY in this repository: the build image has no dotnet/mono, so it is not compiled here.  It mirrors
// include/gsplat_c.h 1:1 (the same table is bound and exercised through ctypes in unitygaussiansplatting_amd/_lib.py).
// Usage inside GaussianSplatRenderer.cs is shown in INTEGRATION.md: each block that records ComputeShader dispatches
// into a CommandBuffer (CreateResourcesForAsset :373-445, SortPoints :612-639, CalcViewData :579-610, the
// DrawProcedural of SortAndRenderSplats :156-166, the composite :206-209) becomes one call below.
using System;
using System.Runtime.InteropServices;

namespace GaussianSplatting.Runtime
{
    public static class GaussianSplatNative
    {
        const string Lib = "gsplat_hip";

        public enum Error { Ok = 0, InvalidArgument = -1, Hip = -2, UnsupportedFormat = -3, OutOfMemory = -4, InvalidAsset = -5, PairOverflow = -6, SortTimeout = -7, NoDevice = -8, Comm = -9 }
        public enum SortMode { Full = 0, Visible = 1 }       // gs_sort_mode: Full = SortPoints as the reference runs it; Visible = cull first, sort what is drawn

        [StructLayout(LayoutKind.Sequential)]
        public struct AssetDesc
        {
            public uint splatCount, posFormat, scaleFormat, colorFormat, shFormat, memoryKind;
            public IntPtr posData;   public ulong posSize;
            public IntPtr otherData; public ulong otherSize;
            public IntPtr colorData; public ulong colorSize;
            public IntPtr shData;    public ulong shSize;
            public IntPtr chunkData; public ulong chunkSize;
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct FrameParams
        {
            public fixed float matrixMV[16];
            public fixed float matrixObjectToWorld[16];
            public fixed float matrixWorldToObject[16];
            public fixed float matrixVP[16];
            public float projM00, projM11;
            public float screenW, screenH;
            public fixed float camPosWorld[3];
            public float splatScale, opacityScale;
            public uint shOrder, shOnly;
            public float nearClip, farClip;
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct FrameStats { public ulong tilePairs, pairCapacity; public uint visibleSplats, tilesX, tilesY, sortError, tileW, tileH, sortMode, tieLongRuns, tieLongestRun; }

        [StructLayout(LayoutKind.Sequential)]
        public struct StageTimes { public float calcDistancesMs, sortMs, calcViewMs, binMs, pairSortMs, blendMs, resolveMs, totalMs; public uint frames; public float onesweepDepthMs, onesweepPairsMs; public uint onesweepPairLaunches; public float onesweepDepthKernelMs, onesweepPairsKernelMs; public uint onesweepDepthLaunches; }

        [DllImport(Lib)] public static extern int gs_abi_version();
        [DllImport(Lib)] public static extern IntPtr gs_error_string(int err);
        [DllImport(Lib)] public static extern IntPtr gs_last_error_string();

        [DllImport(Lib)] public static extern int gs_context_create(int device, IntPtr hipStream, out IntPtr ctx);
        [DllImport(Lib)] public static extern int gs_context_destroy(IntPtr ctx);
        [DllImport(Lib)] public static extern int gs_context_synchronize(IntPtr ctx);
        [DllImport(Lib)] public static extern int gs_context_set_overlap(IntPtr ctx, int enabled);
        [DllImport(Lib)] public static extern int gs_context_set_shared_gpu(IntPtr ctx, int shared);
        [DllImport(Lib)] public static extern int gs_context_device_info(IntPtr ctx, byte[] nameOut, UIntPtr nameCap, out int cuCount, out ulong hbmBytes);

        [DllImport(Lib)] public static extern int gs_asset_create(IntPtr ctx, ref AssetDesc desc, out IntPtr asset);
        [DllImport(Lib)] public static extern int gs_asset_destroy(IntPtr asset);
        [DllImport(Lib)] public static extern int gs_asset_splat_count(IntPtr asset, out uint count);
        [DllImport(Lib)] public static extern int gs_asset_device_blobs(IntPtr asset, [Out] IntPtr[] ptrs5, [Out] ulong[] sizes5);
        [DllImport(Lib)] public static extern int gs_asset_info(IntPtr asset, [Out] uint[] out6);

        // multi-GPU (view-parallel): one context per GPU, the asset broadcast once over RCCL
        public const int GS_COMM_ID_BYTES = 128;
        [DllImport(Lib)] public static extern int gs_comm_unique_id([Out] byte[] id128);
        [DllImport(Lib)] public static extern int gs_comm_create(IntPtr ctx, int nranks, int rank, byte[] id128, out IntPtr comm);
        [DllImport(Lib)] public static extern int gs_comm_destroy(IntPtr comm);
        [DllImport(Lib)] public static extern int gs_comm_info(IntPtr comm, out int nranks, out int rank);
        [DllImport(Lib)] public static extern int gs_asset_broadcast(IntPtr comm, IntPtr assetOnRoot, int root, out IntPtr asset);
        [DllImport(Lib)] public static extern int gs_asset_replicate(IntPtr dstContext, IntPtr srcAsset, out IntPtr asset);

        [DllImport(Lib)] public static extern int gs_renderer_create(IntPtr ctx, IntPtr asset, out IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_destroy(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_reset_order(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_sort(IntPtr renderer, float[] matrixSort16);
        [DllImport(Lib)] public static extern int gs_renderer_calc_view(IntPtr renderer, ref FrameParams p);
        [DllImport(Lib)] public static extern int gs_renderer_draw(IntPtr renderer, ref FrameParams p, IntPtr target);
        [DllImport(Lib)] public static extern int gs_renderer_render(IntPtr renderer, float[] matrixSort16, ref FrameParams p, IntPtr target, int doSort);
        // GaussianCutout.ShaderData (GaussianCutout.cs:19-23), matrix transposed to this ABI's row-major convention
        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct Cutout { public fixed float matrix[16]; public uint typeAndFlags; }
        [DllImport(Lib)] public static extern int gs_renderer_set_cutouts(IntPtr renderer, Cutout[] cutouts, uint count);
        [DllImport(Lib)] public static extern int gs_renderer_set_deleted_bits(IntPtr renderer, uint[] words, UIntPtr wordCount);
        // selection and deletion (GaussianSplatRenderer.Edit*, GaussianSplatRenderer.cs:705-740,767-840,896-934); the selection is drawn once gs_renderer_set_selection_highlight(r, 1) is set
        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct EditInfo { public uint selected, deleted, cut; public fixed float boundsMin[3]; public fixed float boundsMax[3]; }
        [DllImport(Lib)] public static extern int gs_renderer_edit_select_all(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_deselect_all(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_invert_selection(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_store_selection(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_update_selection(IntPtr renderer, ref FrameParams p, float[] selectionRect4, int subtract);
        [DllImport(Lib)] public static extern int gs_renderer_edit_delete_selected(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_info(IntPtr renderer, out EditInfo info);
        [DllImport(Lib)] public static extern int gs_renderer_edit_upload_selected_bits(IntPtr renderer, uint[] words, UIntPtr wordCount);
        [DllImport(Lib)] public static extern int gs_renderer_edit_download_bits(IntPtr renderer, uint[] selected, uint[] selectedMouseDown, uint[] deleted, UIntPtr wordCount);
        [DllImport(Lib)] public static extern int gs_renderer_edit_release(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_set_selection_highlight(IntPtr renderer, int enabled);
        // moving the selection (copy-on-write of the renderer's pos / other blobs); matrices row-major, quaternion x y z w
        [DllImport(Lib)] public static extern int gs_renderer_edit_store_pos_mouse_down(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_store_other_mouse_down(IntPtr renderer);
        // rigid rotate / scale (off by default): orientation and SH follow a rotation, splat sizes a uniform scale; the third mouse-down copy
        [DllImport(Lib)] public static extern int gs_renderer_edit_set_rigid_transforms(IntPtr renderer, int enabled);
        [DllImport(Lib)] public static extern int gs_renderer_edit_store_sh_mouse_down(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_translate_selection(IntPtr renderer, float[] delta3);
        [DllImport(Lib)] public static extern int gs_renderer_edit_rotate_selection(IntPtr renderer, float[] center3, float[] localToWorld16, float[] worldToLocal16, float[] rotationXyzw4);
        [DllImport(Lib)] public static extern int gs_renderer_edit_scale_selection(IntPtr renderer, float[] center3, float[] localToWorld16, float[] worldToLocal16, float[] scale3);
        [DllImport(Lib)] public static extern int gs_renderer_edit_download_pos_other(IntPtr renderer, IntPtr pos, UIntPtr posBytes, IntPtr other, UIntPtr otherBytes);
        // export (EditExportData, GaussianSplatRenderer.cs:936-958; ExportPlyFile, GaussianSplatRendererEditor.cs:394-445): records of 62 floats = InputSplatData
        public const int ExportRecordBytes = 248;
        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct ExportParams { public fixed float matrixObjectToWorld[16]; public fixed float rotation[4]; public fixed float scale[3]; public uint bakeTransform; }
        [DllImport(Lib)] public static extern int gs_renderer_edit_export_data(IntPtr renderer, ref ExportParams p, IntPtr dst, UIntPtr bytes, int memoryKind);
        [DllImport(Lib)] public static extern int gs_renderer_edit_export_alive(IntPtr renderer, ref ExportParams p, IntPtr dst, UIntPtr capacityRecords, out uint alive);
        [DllImport(Lib)] public static extern int gs_renderer_edit_export_ply(IntPtr renderer, ref ExportParams p, [MarshalAs(UnmanagedType.LPStr)] string path, out uint alive);
        // export to SPZ: the gunzipped stream (header + six columns) to host memory, or the gzip file; fractBits 0..24 or SpzFractAuto, level -1..9
        public const uint SpzFractAuto = 0xffffffffu;
        [StructLayout(LayoutKind.Sequential)]
        public struct SpzParams { public uint shLevel; public uint fractBits; public int compressionLevel; public uint sliceBytes; }
        [DllImport(Lib)] public static extern int gs_renderer_edit_export_spz_body(IntPtr renderer, ref ExportParams p, ref SpzParams s, IntPtr dst, UIntPtr capacityBytes, out ulong bodyBytes, out uint alive, out uint fractBitsUsed);
        [DllImport(Lib)] public static extern int gs_renderer_edit_export_spz(IntPtr renderer, ref ExportParams p, ref SpzParams s, [MarshalAs(UnmanagedType.LPStr)] string path, out uint alive);
        // merge (EditSetSplatCount / EditCopySplatsInto, GaussianSplatRenderer.cs:960-1075; MergeSplatObjects, GaussianSplatRendererEditor.cs:213-235)
        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct CopyParams { public fixed float matrix[16]; public fixed float rotation[4]; public fixed float scale[3]; }
        [DllImport(Lib)] public static extern int gs_renderer_splat_count(IntPtr renderer, out uint count);
        [DllImport(Lib)] public static extern int gs_renderer_edit_set_splat_count(IntPtr renderer, uint newCount, IntPtr copyParamsOrZero);
        [DllImport(Lib)] public static extern int gs_renderer_edit_copy_splats_into(IntPtr src, IntPtr dst, ref CopyParams p, uint srcStart, uint dstStart, uint count);
        [DllImport(Lib)] public static extern int gs_renderer_edit_download_splat_data(IntPtr renderer, IntPtr pos, UIntPtr posBytes, IntPtr other, UIntPtr otherBytes, IntPtr color, UIntPtr colorBytes, IntPtr sh, UIntPtr shBytes);
        // undo / redo of the edit state: a checkpoint before a gesture journals the two bit buffers and the records of the selected splats; undo / redo swap them back in
        public const uint HistSelection = 1u, HistDeleted = 2u, HistPos = 4u, HistOther = 8u, HistSH = 16u, HistTransform = 0x80000000u;
        [StructLayout(LayoutKind.Sequential)]
        public struct EditHistoryInfo { public uint enabled, undoDepth, redoDepth, topWhat; public ulong bytes, maxBytes, topBytes; public uint topSplats, evicted, uncoveredTransforms; }
        [DllImport(Lib)] public static extern int gs_renderer_edit_history_enable(IntPtr renderer, ulong maxBytes);
        [DllImport(Lib)] public static extern int gs_renderer_edit_checkpoint(IntPtr renderer, uint what);
        [DllImport(Lib)] public static extern int gs_renderer_edit_undo(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_redo(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_history_clear(IntPtr renderer);
        [DllImport(Lib)] public static extern int gs_renderer_edit_history_info(IntPtr renderer, out EditHistoryInfo info);
        [DllImport(Lib)] public static extern int gs_renderer_set_view_buffer_mode(IntPtr renderer, int everyFrame);
        [DllImport(Lib)] public static extern int gs_renderer_set_blend_mode(IntPtr renderer, int mode);
        [DllImport(Lib)] public static extern int gs_renderer_set_tile_shape(IntPtr renderer, uint tileW, uint tileH);
        [DllImport(Lib)] public static extern int gs_renderer_tile_shape(IntPtr renderer, uint width, uint height, out uint tileW, out uint tileH);
        [DllImport(Lib)] public static extern int gs_renderer_set_profiling(IntPtr renderer, int frames);
        [DllImport(Lib)] public static extern int gs_renderer_set_kernel_timing(IntPtr renderer, int enabled);
        [DllImport(Lib)] public static extern int gs_renderer_reserve_pairs(IntPtr renderer, ulong pairCapacity);
        [DllImport(Lib)] public static extern int gs_renderer_poll_pairs(IntPtr renderer, out ulong tilePairs, out ulong pairCapacity);
        [DllImport(Lib)] public static extern int gs_renderer_download_order(IntPtr renderer, uint[] dst, UIntPtr count);
        [DllImport(Lib)] public static extern int gs_renderer_download_distances(IntPtr renderer, uint[] dst, UIntPtr count);
        [DllImport(Lib)] public static extern int gs_renderer_upload_order(IntPtr renderer, uint[] src, UIntPtr count);
        // gs_sort_mode: 0 = GS_SORT_FULL (SortPoints as the reference runs it), 1 = GS_SORT_VISIBLE (cull first, sort what is drawn)
        [DllImport(Lib)] public static extern int gs_renderer_set_sort_mode(IntPtr renderer, int mode);
        [DllImport(Lib)] public static extern int gs_renderer_sort_mode(IntPtr renderer, out int mode, out int active);
        [DllImport(Lib)] public static extern int gs_renderer_set_sort_history_limit(IntPtr renderer, uint rows);
        [DllImport(Lib)] public static extern int gs_renderer_sort_history(IntPtr renderer, out uint rows, out uint limit, out ulong consolidations);
        [DllImport(Lib)] public static extern int gs_renderer_set_frames_in_flight(IntPtr renderer, int frames);
        [DllImport(Lib)] public static extern int gs_renderer_frames_in_flight(IntPtr renderer, out int frames, out int active);
        [DllImport(Lib)] public static extern int gs_renderer_download_visible_order(IntPtr renderer, uint[] dst, UIntPtr capacity, out uint count);
        [DllImport(Lib)] public static extern int gs_renderer_set_render_mode(IntPtr renderer, int mode, float pointDisplaySize);
        [DllImport(Lib)] public static extern int gs_renderer_download_view(IntPtr renderer, IntPtr dst, UIntPtr bytes);
        [DllImport(Lib)] public static extern int gs_renderer_download_raster_records(IntPtr renderer, IntPtr recs, IntPtr rects, IntPtr visMask);
        [DllImport(Lib)] public static extern int gs_renderer_frame_stats(IntPtr renderer, out FrameStats stats);
        [DllImport(Lib)] public static extern int gs_renderer_frame_times(IntPtr renderer, [Out] float[] ms, int capacity, out int count);
        [DllImport(Lib)] public static extern int gs_renderer_stage_times(IntPtr renderer, out StageTimes times);

        [DllImport(Lib)] public static extern int gs_target_create(IntPtr ctx, uint width, uint height, out IntPtr target);
        [DllImport(Lib)] public static extern int gs_target_destroy(IntPtr target);
        [DllImport(Lib)] public static extern int gs_target_clear(IntPtr target);
        [DllImport(Lib)] public static extern int gs_target_download(IntPtr target, IntPtr dstRgba16f, UIntPtr bytes);
        [DllImport(Lib)] public static extern int gs_target_resolve(IntPtr target, float[] backgroundRgba4, IntPtr dstRgba32f, IntPtr dstRgba8);
        [DllImport(Lib)] public static extern int gs_target_set_scene_depth(IntPtr target, IntPtr depth, int memoryKind);
        [DllImport(Lib)] public static extern int gs_target_device_ptr(IntPtr target, out IntPtr rgba16fDev, out IntPtr resolvedDev);
        [DllImport(Lib)] public static extern int gs_target_set_profiling(IntPtr target, int enabled);
        [DllImport(Lib)] public static extern int gs_target_resolve_time(IntPtr target, out float meanMs, out int count);
        // pick output: one GsPickRecord per pixel from the splat blend -- the splat that took the pixel's accumulated alpha across the threshold, its view depth, the drawing renderer's tag
        [StructLayout(LayoutKind.Sequential)] public struct GsPickRecord { public float depth; public uint splat; public uint tag; public uint zero; }   // none: +inf, 0xFFFFFFFF, 0, 0
        [DllImport(Lib)] public static extern int gs_target_set_pick_output(IntPtr target, int enabled, float threshold);
        [DllImport(Lib)] public static extern int gs_target_download_pick(IntPtr target, IntPtr dstRecords, UIntPtr bytes);
        [DllImport(Lib)] public static extern int gs_target_pick_at(IntPtr target, uint x, uint y, out GsPickRecord record);
        [DllImport(Lib)] public static extern int gs_target_pick_device_ptr(IntPtr target, out IntPtr pickDev);
        [DllImport(Lib)] public static extern int gs_renderer_set_pick_tag(IntPtr renderer, uint tag);
        [DllImport(Lib)] public static extern int gs_renderer_edit_select_surface(IntPtr renderer, IntPtr target, int x0, int y0, int x1, int y1, int subtract);
        // floaters: min(count, cap) of the alive splats within radius (object space) of every alive splat, 0xFFFFFFFF for the others; and the selection of those with fewer than minNeighbours.  Both block
        [DllImport(Lib)] public static extern int gs_renderer_edit_neighbour_counts(IntPtr renderer, float radius, uint cap, [Out] uint[] countsOut, UIntPtr count);
        [DllImport(Lib)] public static extern int gs_renderer_edit_select_sparse(IntPtr renderer, float radius, uint minNeighbours, int subtract);
        // islands: the connected components of the neighbour graph at that radius -- per alive splat the smallest index and the size of its component (0xFFFFFFFF and 0 for the others; either array may be null); the selection of the components smaller than minSize; and the selection grown to every component that holds a selected splat.  All block
        [DllImport(Lib)] public static extern int gs_renderer_edit_components(IntPtr renderer, float radius, [Out] uint[] labelsOut, [Out] uint[] sizesOut, UIntPtr count);
        [DllImport(Lib)] public static extern int gs_renderer_edit_select_islands(IntPtr renderer, float radius, uint minSize, int subtract);
        [DllImport(Lib)] public static extern int gs_renderer_edit_grow_selection(IntPtr renderer, float radius);
        // select by attribute: one fp32 value per alive splat from the decoded fields (0xFFFFFFFF for the others); the selection of a value range (asynchronous); the scope's size, NaN count and extreme values; a histogram of bins + 3 words (bins, below, above, NaN); order statistics of the sorted values.  point: float[3] in object space, read for Dist2 only (else null).  All but the range selection block
        public enum SplatAttribute { Opacity = 0, ScaleMax = 1, ScaleMin = 2, Volume = 3, PosX = 4, PosY = 5, PosZ = 6, Dist2 = 7, ColorR = 8, ColorG = 9, ColorB = 10, Luma = 11 }
        public enum AttributeScope { Alive = 0, Selected = 1 }
        [StructLayout(LayoutKind.Sequential)] public struct GsAttributeStats { public uint members; public uint nans; public float vmin; public float vmax; }
        [DllImport(Lib)] public static extern int gs_renderer_edit_attribute_values(IntPtr renderer, int attr, float[] point, [Out] float[] valuesOut, UIntPtr count);
        [DllImport(Lib)] public static extern int gs_renderer_edit_select_range(IntPtr renderer, int attr, float[] point, float lo, float hi, int subtract);
        [DllImport(Lib)] public static extern int gs_renderer_edit_attribute_stats(IntPtr renderer, int attr, float[] point, int scope, out GsAttributeStats stats);
        [DllImport(Lib)] public static extern int gs_renderer_edit_attribute_histogram(IntPtr renderer, int attr, float[] point, int scope, float lo, float hi, uint bins, [Out] uint[] histOut, UIntPtr count);
        [DllImport(Lib)] public static extern int gs_renderer_edit_attribute_ranks(IntPtr renderer, int attr, float[] point, int scope, uint[] ranks, uint rankCount, [Out] float[] valuesOut, out uint population);
        // lasso, polygon and brush: a screen mask of one bit per pixel (row 0 = top; a row is ceil(W/32) words, bit x & 31 of word x >> 5), filled on the GPU by the even-odd rule or by a round-capped polyline; xy = x0 y0 x1 y1 ... in pixels.  The selection through it: the gesture contract of gs_renderer_edit_update_selection (a splat whose pixel position is NaN hits nothing), and gs_renderer_edit_select_surface over the pixels whose bit is set.  The download blocks
        [DllImport(Lib)] public static extern int gs_mask_create(IntPtr ctx, uint width, uint height, out IntPtr mask);
        [DllImport(Lib)] public static extern int gs_mask_destroy(IntPtr mask);
        [DllImport(Lib)] public static extern int gs_mask_clear(IntPtr mask);
        [DllImport(Lib)] public static extern int gs_mask_upload(IntPtr mask, uint[] words, UIntPtr wordCount);
        [DllImport(Lib)] public static extern int gs_mask_download(IntPtr mask, [Out] uint[] words, UIntPtr wordCount);
        [DllImport(Lib)] public static extern int gs_mask_fill_polygon(IntPtr mask, float[] xy, uint vertices, int subtract);
        [DllImport(Lib)] public static extern int gs_mask_stroke(IntPtr mask, float[] xy, uint points, float radius, int subtract);
        [DllImport(Lib)] public static extern int gs_renderer_edit_update_selection_mask(IntPtr renderer, ref FrameParams p, IntPtr mask, int subtract);
        [DllImport(Lib)] public static extern int gs_renderer_edit_select_surface_mask(IntPtr renderer, IntPtr target, IntPtr mask, int subtract);

        // native importer (host code): GaussianSplatAssetCreator.CreateAsset without the asset database
        [StructLayout(LayoutKind.Sequential)]
        public struct ImportInput { public uint splatCount; public IntPtr pos, dc0, sh, opacity, scale, rot; }
        [StructLayout(LayoutKind.Sequential)]
        public struct ImportFormats { public uint posFormat, scaleFormat, colorFormat, shFormat, linearize, morton; }
        [DllImport(Lib)] public static extern int gs_import_blob_sizes(uint splatCount, ref ImportFormats formats, [Out] ulong[] sizes5);
        [DllImport(Lib)] public static extern int gs_import_encode(ref ImportInput input, ref ImportFormats formats, IntPtr[] blobs5, ulong[] sizes5, float[] boundsMin3, float[] boundsMax3);
        // the Cluster* palette assignment on a context's GPU (ctx = IntPtr.Zero: the host loop); the same indices and asset bytes either way
        [DllImport(Lib)] public static extern int gs_import_assign_clusters(IntPtr ctx, float[] x, ulong n, float[] means, uint k, [Out] uint[] indexOut);
        [DllImport(Lib)] public static extern int gs_import_cluster_shs(IntPtr ctx, float[] x, ulong n, uint k, [Out] float[] meansOut, [Out] uint[] indexOut);
        [DllImport(Lib)] public static extern int gs_import_encode_on(IntPtr ctx, ref ImportInput input, ref ImportFormats formats, IntPtr[] blobs5, ulong[] sizes5, float[] boundsMin3, float[] boundsMax3);
        [DllImport(Lib)] public static extern int gs_renderer_edit_bake_asset(IntPtr renderer, ref ImportFormats formats, out IntPtr asset, out uint alive, [Out] float[] boundsMin3, [Out] float[] boundsMax3);
        [DllImport(Lib)] public static extern int gs_import_encode_to_asset(IntPtr ctx, ref ImportInput input, uint memoryKind, ref ImportFormats formats, out IntPtr asset, [Out] float[] boundsMin3, [Out] float[] boundsMax3);
        [DllImport(Lib)] public static extern int gs_asset_download_blobs(IntPtr asset, IntPtr[] blobs5, ulong[] sizes5);

        [DllImport(Lib)] public static extern int gs_ply_open([MarshalAs(UnmanagedType.LPStr)] string path, out IntPtr ply, out uint splatCount);
        [DllImport(Lib)] public static extern int gs_spz_open([MarshalAs(UnmanagedType.LPStr)] string path, out IntPtr ply, out uint splatCount);
        [DllImport(Lib)] public static extern int gs_ply_arrays(IntPtr ply, out ImportInput arrays);
        [DllImport(Lib)] public static extern int gs_ply_close(IntPtr ply);
        // a .ply / .spz file straight into a device asset: the file's own bytes are the GPU importer's source (kind: 1 PLY, 2 SPZ)
        [StructLayout(LayoutKind.Sequential)]
        public struct SplatFileInfo
        {
            public uint kind, splatCount, stride, shLevel, fractBits, reserved;
            public ulong bodyBytes;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 62)] public int[] offsets;
        }
        [DllImport(Lib)] public static extern int gs_splat_file_open([MarshalAs(UnmanagedType.LPStr)] string path, out IntPtr file, out SplatFileInfo info);
        [DllImport(Lib)] public static extern int gs_splat_file_close(IntPtr file);
        [DllImport(Lib)] public static extern int gs_import_file_to_asset(IntPtr ctx, IntPtr file, ref ImportFormats formats, uint sliceBytes, out IntPtr asset, [Out] float[] boundsMin3, [Out] float[] boundsMax3);

        [DllImport(Lib)] public static extern int gs_sorter_create(IntPtr ctx, uint maxCount, out IntPtr sorter);
        [DllImport(Lib)] public static extern int gs_sorter_destroy(IntPtr sorter);
        [DllImport(Lib)] public static extern int gs_sorter_dispatch(IntPtr sorter, IntPtr keysDev, IntPtr valuesDev, uint count, uint keyBits);
        [DllImport(Lib)] public static extern int gs_sorter_sort_host(IntPtr sorter, uint[] keys, uint[] values, uint count, uint keyBits);

        public static void Check(int rc, string where)
        {
            if (rc != 0)
                throw new InvalidOperationException($"{where}: {(Error)rc} ({Marshal.PtrToStringAnsi(gs_last_error_string())})");
        }
    }
}
