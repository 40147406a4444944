"""Host-side mirror of the reference's renderer API over the C-ABI (include/gsplat_c.h).

Same class, field and method names as /root/reference/package/Runtime/GaussianSplatRenderer.cs
(GaussianSplatRenderSystem :17-212, GaussianSplatRenderer :214-680) and GpuSorting.cs, minus the Unity
plumbing (MonoBehaviour, CommandBuffer, materials): where the C# records a dispatch into a CommandBuffer,
these methods enqueue the corresponding HIP kernels on the context's stream.  A .NET host would be the same
thin layer over [DllImport("gsplat_hip")] (unitygaussiansplatting_amd/dotnet/GaussianSplatNative.cs).
"""
from __future__ import annotations

import atexit
import ctypes as C
import enum
import os
import weakref
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._abi import (GS_ERR_INVALID_ARGUMENT, GS_ERR_PAIR_OVERFLOW, GS_SCOPE_ALIVE, GS_SCOPE_SELECTED, GS_SORT_FULL, GS_SORT_VISIBLE, GS_SPZ_FRACT_AUTO, PICK_DTYPE, VIEW_DTYPE, gs_attribute_stats,
                   gs_copy_params, gs_edit_history_info, gs_edit_info,
                   gs_export_params, gs_frame_params, gs_frame_stats, gs_import_formats, gs_pick_record, gs_spz_params, gs_stage_times, make_asset_desc)
from ._lib import GsError, check
from .asset import CalcTextureSize, ColorFormat, GaussianSplatAsset, SHFormat, VectorFormat, kCurrentVersion, kMaxSplats
from .camera import Camera, Transform, frame_params, mat_mul, matrix_rotation_scale, sort_matrix
from .cutout import GaussianCutout, shader_data_array


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# Contexts still alive at interpreter exit are disposed (children first) BEFORE the HIP runtime's own static
# destructors run; a late __del__ calling into a torn-down runtime aborts the process.
_live_contexts = weakref.WeakSet()


@atexit.register
def _dispose_all_contexts():
    for ctx in list(_live_contexts):
        try:
            ctx.Dispose()
        except Exception:
            pass


class RenderMode(enum.IntEnum):          # GaussianSplatRenderer.RenderMode (:217-223)
    Splats = 0
    DebugPoints = 1
    DebugPointIndices = 2
    DebugBoxes = 3
    DebugChunkBounds = 4


class SortMode(enum.IntEnum):            # gs_sort_mode: what SortPoints sorts (no counterpart in the reference, whose sort precedes its cull)
    Full = GS_SORT_FULL                  # all N splats, every SortPoints, like GaussianSplatRenderer.SortPoints (:612-639)
    Visible = GS_SORT_VISIBLE            # cull first: only the splats CalcViewData found visible, inside Draw


class SplatAttribute(enum.IntEnum):      # gs_splat_attribute: one fp32 value per splat from its decoded fields
    Opacity = 0                          # linear opacity
    ScaleMax = 1                         # the largest / smallest of the three linear scales
    ScaleMin = 2
    Volume = 3                           # their product
    PosX = 4                             # object-space position
    PosY = 5
    PosZ = 6
    Dist2 = 7                            # squared distance to `point` (object space): the sphere tool
    ColorR = 8                           # DC colour
    ColorG = 9
    ColorB = 10
    Luma = 11                            # 0.299 r + 0.587 g + 0.114 b


class EditHistoryFlags(enum.IntFlag):    # GS_HIST_*: what an EditCheckpoint captures
    Selection = 1                        # the selected bits, whole
    Deleted = 2                          # the deleted bits, whole
    Pos = 4                              # the records of the splats selected at the checkpoint ...
    Other = 8
    SH = 16
    Transform = 0x80000000               # Pos | Other, and SH while EditSetRigidTransforms is on


class Bounds:
    """UnityEngine.Bounds as UpdateEditCountsAndBounds uses it (GaussianSplatRenderer.cs:735-739): center + extents, float32."""

    def __init__(self):
        self.center = np.zeros(3, np.float32)
        self.extents = np.zeros(3, np.float32)

    def SetMinMax(self, mn, mx) -> None:
        mn, mx = np.asarray(mn, np.float32), np.asarray(mx, np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            self.extents = ((mx - mn) * np.float32(0.5)).astype(np.float32)
            self.center = (mn + self.extents).astype(np.float32)

    @property
    def min(self) -> np.ndarray:
        with np.errstate(over="ignore", invalid="ignore"):
            return (self.center - self.extents).astype(np.float32)

    @property
    def max(self) -> np.ndarray:
        with np.errstate(over="ignore", invalid="ignore"):
            return (self.center + self.extents).astype(np.float32)


class GpuContext:
    """One GPU + one HIP stream (the analogue of Unity's graphics device + render thread)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._h = C.c_void_p()
        check(_lib.lib().gs_context_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h)), "gs_context_create")
        self.device = device
        self._children = weakref.WeakSet()      # targets / sorters / renderers: disposed before the context is
        _live_contexts.add(self)

    def _adopt(self, child) -> None:
        self._children.add(child)

    def Synchronize(self) -> None:
        check(_lib.lib().gs_context_synchronize(self._h), "gs_context_synchronize")

    def SetSharedGpu(self, shared) -> None:
        """Other kernels that wait on their own workgroups (another process using the library, another context sorting or binning at the same time) may share
        the GPU: gs_context_set_shared_gpu -- the full sort's XCD-dealt gather pass and a persistent grid's static first round give way to the dependency-ordered
        forms.  True / False pin it, None = automatic (shared while this process holds more than one context on the device)."""
        check(_lib.lib().gs_context_set_shared_gpu(self._h, -1 if shared is None else int(bool(shared))), "gs_context_set_shared_gpu")

    def SetOverlap(self, enabled: bool) -> None:
        """Run SortPoints concurrently with CalcViewData on the context's second queue (default off: no gain on MI355X)."""
        check(_lib.lib().gs_context_set_overlap(self._h, int(bool(enabled))), "gs_context_set_overlap")

    def CreateScreenMask(self, width: int, height: int) -> "ScreenMask":
        """A zeroed screen mask of this context: what FillPolygon / Stroke draw into and EditUpdateSelectionMask / EditSelectSurfaceMask select through."""
        return ScreenMask(self, width, height)

    def DeviceInfo(self) -> Tuple[str, int, int]:
        name = C.create_string_buffer(256)
        cus = C.c_int32()
        mem = C.c_uint64()
        check(_lib.lib().gs_context_device_info(self._h, name, 256, C.byref(cus), C.byref(mem)), "gs_context_device_info")
        return name.value.decode(), cus.value, mem.value

    def Dispose(self) -> None:
        if self._h:
            for ch in sorted(self._children, key=lambda c: isinstance(c, GpuAsset)):     # a child must never outlive its context (it holds a raw pointer
                ch.Dispose()                                                             # to it), nor a device asset the renderers over it
            _lib.lib().gs_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass


class RenderTarget:
    """The _GaussianSplatRT temporary: RGBA16F, premultiplied, cleared to 0 (GaussianSplatRenderer.cs:194-196)."""

    def __init__(self, ctx: GpuContext, width: int, height: int):
        self.ctx, self.width, self.height = ctx, width, height
        self._h = C.c_void_p()
        check(_lib.lib().gs_target_create(ctx._h, width, height, C.byref(self._h)), "gs_target_create")
        ctx._adopt(self)

    def Clear(self) -> None:
        check(_lib.lib().gs_target_clear(self._h), "gs_target_clear")

    def SetSceneDepth(self, depth: Optional[np.ndarray]) -> None:
        """The camera's depth attachment (GaussianSplatRenderer.cs:195): H x W float32 VIEW depths of the opaque scene, or None."""
        if depth is None:
            check(_lib.lib().gs_target_set_scene_depth(self._h, None, 0), "gs_target_set_scene_depth")
            return
        d = np.ascontiguousarray(depth, np.float32)
        assert d.shape == (self.height, self.width)
        check(_lib.lib().gs_target_set_scene_depth(self._h, d.ctypes.data, 0), "gs_target_set_scene_depth")

    def Download(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), np.uint16)
        check(_lib.lib().gs_target_download(self._h, out.ctypes.data, out.nbytes), "gs_target_download")
        return out

    def SetPickOutput(self, enabled: bool, threshold: float = 0.5) -> None:
        """True: splat draws also leave one record per pixel -- the splat whose blend took the pixel's accumulated alpha across `threshold`
        (0 < threshold <= 1), its view depth and the drawing renderer's tag (gs_target_set_pick_output).  False: frees the records."""
        check(_lib.lib().gs_target_set_pick_output(self._h, int(bool(enabled)), float(threshold)), "gs_target_set_pick_output")

    def DownloadPick(self) -> np.ndarray:
        """H x W structured array (depth f4, splat u4, tag u4, zero u4), row 0 = top; a pixel never crossed is (+inf, 0xFFFFFFFF, 0, 0).  Blocks."""
        out = np.empty((self.height, self.width), np.dtype(PICK_DTYPE))
        check(_lib.lib().gs_target_download_pick(self._h, out.ctypes.data, out.nbytes), "gs_target_download_pick")
        return out

    def PickAt(self, x: int, y: int) -> Tuple[float, int, int]:
        """(depth, splat, tag) of pixel (x, y), y down; splat = 0xFFFFFFFF and depth = +inf where no splat crossed the threshold.  Blocks."""
        if x < 0 or y < 0:
            raise GsError(GS_ERR_INVALID_ARGUMENT, "gs_target_pick_at", "pixel outside the target")
        rec = gs_pick_record()
        check(_lib.lib().gs_target_pick_at(self._h, int(x), int(y), C.byref(rec)), "gs_target_pick_at")
        return rec.depth, rec.splat, rec.tag

    def Resolve(self, background=(0.0, 0.0, 0.0, 0.0), want8: bool = True):
        """GaussianComposite.shader onto a constant background: (linear RGBA float32, sRGB RGBA8)."""
        bg = np.asarray(background, np.float32)
        o32 = np.empty((self.height, self.width, 4), np.float32)
        o8 = np.empty((self.height, self.width, 4), np.uint8) if want8 else None
        check(_lib.lib().gs_target_resolve(self._h, _fptr(bg), o32.ctypes.data, o8.ctypes.data if want8 else None), "gs_target_resolve")
        return o32, o8

    def ResolveAsync(self, background=(0.0, 0.0, 0.0, 0.0)) -> None:
        bg = np.asarray(background, np.float32)
        check(_lib.lib().gs_target_resolve(self._h, _fptr(bg), None, None), "gs_target_resolve")

    def SetProfiling(self, enabled: bool) -> None:
        check(_lib.lib().gs_target_set_profiling(self._h, int(bool(enabled))), "gs_target_set_profiling")

    def ResolveTime(self) -> Tuple[float, int]:
        """(mean GPU ms, count) of the resolves since the last call (hipEvents on the context's stream); blocks."""
        ms, cnt = C.c_float(), C.c_int32()
        check(_lib.lib().gs_target_resolve_time(self._h, C.byref(ms), C.byref(cnt)), "gs_target_resolve_time")
        return ms.value, cnt.value

    def Dispose(self) -> None:
        if self._h:
            _lib.lib().gs_target_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass


class ScreenMask:
    """One bit per pixel of a width x height screen, filled on the GPU: what the lasso, the polygon and the brush draw and the renderer selects through
    (gs_mask).  Row 0 = top, y down, x right, as the pick records; points are pixel coordinates in that frame."""

    def __init__(self, ctx: GpuContext, width: int, height: int):
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.rowWords = (self.width + 31) // 32
        self._h = C.c_void_p()
        check(_lib.lib().gs_mask_create(ctx._h, self.width, self.height, C.byref(self._h)), "gs_mask_create")
        ctx._adopt(self)

    @staticmethod
    def _points(points) -> np.ndarray:
        p = np.ascontiguousarray(points, np.float32)
        if p.ndim != 2 or p.shape[1] != 2:
            raise GsError(GS_ERR_INVALID_ARGUMENT, "ScreenMask", "points must be an n x 2 array of pixel coordinates")
        return p

    def Clear(self) -> None:
        check(_lib.lib().gs_mask_clear(self._h), "gs_mask_clear")

    def FillPolygon(self, points, subtract: bool = False) -> None:
        """Fill the closed outline through `points` (3 .. 65536 vertices) by the even-odd rule: the covered pixels are set, or with subtract cleared."""
        p = self._points(points)
        check(_lib.lib().gs_mask_fill_polygon(self._h, _fptr(p), len(p), int(bool(subtract))), "gs_mask_fill_polygon")

    def Stroke(self, points, radius: float, subtract: bool = False) -> None:
        """Draw the brush: the round-capped polyline through `points` (1 .. 65536; one point is a disc) with that radius, 0 < radius <= 65536."""
        p = self._points(points)
        check(_lib.lib().gs_mask_stroke(self._h, _fptr(p), len(p), float(radius), int(bool(subtract))), "gs_mask_stroke")

    def UploadWords(self, words: np.ndarray) -> None:
        w = np.ascontiguousarray(words, np.uint32).reshape(-1)
        check(_lib.lib().gs_mask_upload(self._h, w.ctypes.data, len(w)), "gs_mask_upload")

    def DownloadWords(self) -> np.ndarray:
        """height x ceil(width / 32) words, bit x & 31 of word x >> 5 = pixel x.  Blocks."""
        out = np.empty((self.height, self.rowWords), np.uint32)
        check(_lib.lib().gs_mask_download(self._h, out.ctypes.data, out.size), "gs_mask_download")
        return out

    def Upload(self, mask: np.ndarray) -> None:
        """mask: height x width booleans"""
        m = np.asarray(mask, bool)
        if m.shape != (self.height, self.width):
            raise GsError(GS_ERR_INVALID_ARGUMENT, "ScreenMask.Upload", "the array must be height x width")
        padded = np.zeros((self.height, self.rowWords * 32), np.uint8)
        padded[:, :self.width] = m
        self.UploadWords(np.packbits(padded, axis=1, bitorder="little").view(np.uint32))

    def Download(self) -> np.ndarray:
        """height x width booleans.  Blocks."""
        bits = np.unpackbits(self.DownloadWords().view(np.uint8), axis=1, bitorder="little")
        return bits[:, :self.width].astype(bool)

    def Dispose(self) -> None:
        if self._h:
            _lib.lib().gs_mask_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass


class GpuSorting:
    """GpuSorting.cs: stable ascending (uint key, uint payload) device sort.  `SupportResources.Load(count)`
    is the constructor; `Dispatch` sorts device buffers in place, `DispatchHost` round-trips numpy arrays."""

    def __init__(self, ctx: GpuContext, count: int):
        self.ctx, self.count = ctx, count
        self._h = C.c_void_p()
        check(_lib.lib().gs_sorter_create(ctx._h, count, C.byref(self._h)), "gs_sorter_create")
        ctx._adopt(self)

    @property
    def Valid(self) -> bool:
        return bool(self._h)

    def Dispatch(self, keys_dev: int, values_dev: int, count: int, key_bits: int = 32) -> None:
        check(_lib.lib().gs_sorter_dispatch(self._h, C.c_void_p(keys_dev), C.c_void_p(values_dev), count, key_bits), "gs_sorter_dispatch")

    def DispatchHost(self, keys: np.ndarray, values: np.ndarray, key_bits: int = 32):
        k = np.ascontiguousarray(keys, np.uint32).copy()
        v = np.ascontiguousarray(values, np.uint32).copy()
        check(_lib.lib().gs_sorter_sort_host(self._h, k.ctypes.data, v.ctypes.data, len(k), key_bits), "gs_sorter_sort_host")
        return k, v

    def Dispose(self) -> None:
        if self._h:
            _lib.lib().gs_sorter_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass


class GpuAsset:
    """A device-resident asset made on the GPU (GaussianSplatRenderer.EditBakeAsset, creator.CreateGpuAssetFromSplats): the native handle, its splat count, its four formats
    (pos, scale, color, sh) and the position bounds.  Immutable; owned by this object until Dispose()."""

    def __init__(self, ctx: "GpuContext", handle, splatCount: int, formats, boundsMin, boundsMax):
        self.ctx = ctx
        self.handle = handle
        self.splatCount = int(splatCount)
        self.formats = tuple(formats)
        self.boundsMin, self.boundsMax = tuple(boundsMin), tuple(boundsMax)
        ctx._adopt(self)

    def Download(self, name: str = "baked") -> GaussianSplatAsset:
        """The asset in host memory, dataHash computed: the five blobs at the importer's sizes (gs_import_blob_sizes).  Blocks."""
        assert self.handle
        fp, fs, fc, fsh = self.formats
        fmt = gs_import_formats(int(fp), int(fs), int(fc), int(fsh), 0, 0)
        sizes = (C.c_uint64 * 5)()
        check(_lib.lib().gs_import_blob_sizes(self.splatCount, C.byref(fmt), sizes), "gs_import_blob_sizes")
        blobs = [np.zeros(int(sz), np.uint8) if sz else None for sz in sizes]
        ptrs = (C.c_void_p * 5)(*[b.ctypes.data if b is not None else None for b in blobs])
        check(_lib.lib().gs_asset_download_blobs(self.handle, ptrs, sizes), "gs_asset_download_blobs")
        a = GaussianSplatAsset(splatCount=self.splatCount, posFormat=VectorFormat(fp), scaleFormat=VectorFormat(fs), shFormat=SHFormat(fsh),
                               colorFormat=ColorFormat(fc), posData=blobs[0], otherData=blobs[1], colorData=blobs[2], shData=blobs[3],
                               chunkData=blobs[4], boundsMin=self.boundsMin, boundsMax=self.boundsMax, name=name)
        a.dataHash = a.ComputeDataHash()
        a.Validate()
        return a

    def Dispose(self) -> None:
        """Every renderer created over the asset (CreateResourcesForGpuAsset) must have been disposed first."""
        if self.handle:
            _lib.lib().gs_asset_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass


class GaussianSplatRenderer:
    """GaussianSplatRenderer component (GaussianSplatRenderer.cs:214-680): the render path, and of the editing half (:705-1075) selection,
    deletion, moving / rotating / scaling the selection, export and the merge (EditSetSplatCount / EditCopySplatsInto) -- Edit* below.  Selected
    splats are drawn highlighted, as the reference's editor shows them, after SetSelectionHighlight(True); off by default."""

    def __init__(self, ctx: GpuContext, asset: Optional[GaussianSplatAsset] = None, transform: Optional[Transform] = None):
        self.ctx = ctx
        self.transform = transform or Transform()
        # serialized fields, :225-244
        self.m_Asset: Optional[GaussianSplatAsset] = asset
        self.m_RenderOrder = 0
        self.m_SplatScale = 1.0
        self.m_OpacityScale = 1.0
        self.m_SHOrder = 3
        self.m_SHOnly = False
        self.m_SortNthFrame = 1
        self.m_RenderMode = RenderMode.Splats                                # :241
        self.m_PointDisplaySize = 3.0                                        # :242
        self.m_Cutouts: Optional[List[Optional[GaussianCutout]]] = None      # :244
        self.m_FrameCounter = 0
        self.blendMode = 0            # 0 exact (fp16 ROP rounding), 1 fast (fp32 accumulate)
        # applied to the native renderer when its resources are created (SetSortMode changes it later).  GSPLAT_SORT_MODE=visible makes the visible-only
        # mode the default of this host layer -- how the whole GPU test suite is run through it (profiles/r05_pytest_gpu_visible.log)
        self.sortMode = SortMode.Visible if os.environ.get("GSPLAT_SORT_MODE", "") == "visible" else SortMode.Full
        self.framesInFlight = max(1, int(os.environ.get("GSPLAT_FRAMES_IN_FLIGHT", "1") or 1))     # SetFramesInFlight
        self.selectionHighlight = False           # SetSelectionHighlight
        self.pickTag = 0                          # SetPickTag
        self.rigidTransforms = False              # EditSetRigidTransforms
        self._asset_h = C.c_void_p()
        self._r_h = C.c_void_p()
        self._keep: list = []
        self.m_SplatCount = 0
        self.m_Resized = False                    # EditSetSplatCount has replaced the four blobs by private ones of the VeryHigh layout
        self.m_PrevAsset = None
        self.m_PrevHash = None
        self.m_Registered = False
        # edit state (:273-277, 705-740)
        self.m_GpuEditSelected = False            # the native renderer's edit buffers exist (EnsureEditingBuffers)
        self.m_GpuEditPosMouseDown = False        # EditStorePosMouseDown / EditStoreOtherMouseDown have run (:794-809)
        self.m_GpuEditOtherMouseDown = False
        self.m_GpuEditSHMouseDown = False         # EditStoreSHMouseDown has run (the third copy, read by a rigid rotate)
        self.editSelectedSplats = 0
        self.editDeletedSplats = 0
        self.editCutSplats = 0
        self.editModified = False
        self.editSelectedBounds = Bounds()
        ctx._adopt(self)

    def Dispose(self) -> None:
        self.DisposeResourcesForAsset()

    # -- properties ---------------------------------------------------------------------------------------
    @property
    def asset(self):
        return self.m_Asset

    @property
    def splatCount(self) -> int:
        return self.m_SplatCount

    @property
    def HasValidAsset(self) -> bool:          # :361-368
        a = self.m_Asset
        return (a is not None and a.splatCount > 0 and a.formatVersion == kCurrentVersion and a.posData is not None
                and a.otherData is not None and a.shData is not None and a.colorData is not None)

    @property
    def HasValidRenderSetup(self) -> bool:    # :369
        return bool(self._r_h)

    # -- lifetime -------------------------------------------------------------------------------------------
    def CreateResourcesForAsset(self) -> None:      # :373-424
        if not self.HasValidAsset:
            return
        a = self.m_Asset
        self._keep = []
        desc = make_asset_desc(a, self._keep)
        check(_lib.lib().gs_asset_create(self.ctx._h, C.byref(desc), C.byref(self._asset_h)), "gs_asset_create")
        self._keep = []                              # data was copied to the GPU
        check(_lib.lib().gs_renderer_create(self.ctx._h, self._asset_h, C.byref(self._r_h)), "gs_renderer_create")
        self.m_SplatCount = a.splatCount
        if self.sortMode != SortMode.Full:
            check(_lib.lib().gs_renderer_set_sort_mode(self._r_h, int(self.sortMode)), "gs_renderer_set_sort_mode")
        if self.framesInFlight > 1:
            check(_lib.lib().gs_renderer_set_frames_in_flight(self._r_h, int(self.framesInFlight)), "gs_renderer_set_frames_in_flight")
        if self.selectionHighlight:
            check(_lib.lib().gs_renderer_set_selection_highlight(self._r_h, 1), "gs_renderer_set_selection_highlight")
        if self.pickTag:
            check(_lib.lib().gs_renderer_set_pick_tag(self._r_h, self.pickTag), "gs_renderer_set_pick_tag")
        if self.rigidTransforms:
            check(_lib.lib().gs_renderer_edit_set_rigid_transforms(self._r_h, 1), "gs_renderer_edit_set_rigid_transforms")

    def ShareResourcesOf(self, other: "GaussianSplatRenderer") -> None:
        """A second renderer over the SAME device blobs as `other` (no copy; `other` must outlive this one), on this renderer's own context =
        its own stream: frames / views in flight side by side.  In SortMode.Visible tell every such renderer every SortPoints matrix and let
        each draw the frames dealt to it."""
        assert other._asset_h and not self._r_h
        self.m_Asset = other.m_Asset
        self._asset_h, self._asset_borrowed = other._asset_h, True
        check(_lib.lib().gs_renderer_create(self.ctx._h, self._asset_h, C.byref(self._r_h)), "gs_renderer_create")
        self.m_SplatCount = self._native_splat_count()          # the asset's: a resize of `other` is private to it
        self.m_PrevAsset, self.m_PrevHash = other.m_PrevAsset, other.m_PrevHash
        if self.sortMode != SortMode.Full:
            check(_lib.lib().gs_renderer_set_sort_mode(self._r_h, int(self.sortMode)), "gs_renderer_set_sort_mode")

    def CreateResourcesForGpuAsset(self, gpu_asset: "GpuAsset") -> None:
        """A renderer over a device-resident asset (EditBakeAsset): borrowed like ShareResourcesOf's, no upload; `gpu_asset` must outlive it.
        m_Asset stays None -- the data is on the GPU only; gpu_asset.Download() makes a host copy."""
        assert gpu_asset.handle and not self._r_h
        self._asset_h, self._asset_borrowed = gpu_asset.handle, True
        check(_lib.lib().gs_renderer_create(self.ctx._h, self._asset_h, C.byref(self._r_h)), "gs_renderer_create")
        self.m_SplatCount = self._native_splat_count()
        if self.sortMode != SortMode.Full:
            check(_lib.lib().gs_renderer_set_sort_mode(self._r_h, int(self.sortMode)), "gs_renderer_set_sort_mode")
        if self.framesInFlight > 1:
            check(_lib.lib().gs_renderer_set_frames_in_flight(self._r_h, int(self.framesInFlight)), "gs_renderer_set_frames_in_flight")
        if self.selectionHighlight:
            check(_lib.lib().gs_renderer_set_selection_highlight(self._r_h, 1), "gs_renderer_set_selection_highlight")
        if self.pickTag:
            check(_lib.lib().gs_renderer_set_pick_tag(self._r_h, self.pickTag), "gs_renderer_set_pick_tag")
        if self.rigidTransforms:
            check(_lib.lib().gs_renderer_edit_set_rigid_transforms(self._r_h, 1), "gs_renderer_edit_set_rigid_transforms")

    def DisposeResourcesForAsset(self) -> None:     # :527-565
        l = _lib.lib()
        if self._r_h:
            if self.m_GpuEditSelected or self.m_GpuEditPosMouseDown or self.m_GpuEditOtherMouseDown or self.m_GpuEditSHMouseDown:
                l.gs_renderer_edit_release(self._r_h)   # DisposeBuffer(ref m_GpuEditSelected) ..., :547-553
            self.m_GpuEditSelected = self.m_GpuEditPosMouseDown = self.m_GpuEditOtherMouseDown = self.m_GpuEditSHMouseDown = False
            self.editModified = False
            l.gs_renderer_destroy(self._r_h)
            self._r_h = C.c_void_p()
        if self._asset_h:
            if not getattr(self, "_asset_borrowed", False):
                l.gs_asset_destroy(self._asset_h)
            self._asset_h = C.c_void_p()
            self._asset_borrowed = False
        self.m_SplatCount = 0
        self.m_Resized = False

    def OnEnable(self) -> None:                     # :475-485
        self.m_FrameCounter = 0
        self.EnsureSorterAndRegister()
        self.CreateResourcesForAsset()
        self.m_PrevAsset = self.m_Asset
        self.m_PrevHash = self.m_Asset.dataHash if self.m_Asset else None

    def OnDisable(self) -> None:                    # :567-577
        self.DisposeResourcesForAsset()
        GaussianSplatRenderSystem.instance.UnregisterSplat(self)
        self.m_Registered = False

    def EnsureSorterAndRegister(self) -> None:      # :461-473
        if not self.m_Registered:
            GaussianSplatRenderSystem.instance.RegisterSplat(self)
            self.m_Registered = True

    def Update(self) -> None:                       # :641-658 asset hot-reload keyed on dataHash
        cur = self.m_Asset.dataHash if self.m_Asset else None
        if self.m_PrevAsset is not self.m_Asset or self.m_PrevHash != cur:
            self.m_PrevAsset, self.m_PrevHash = self.m_Asset, cur
            self.DisposeResourcesForAsset()
            self.CreateResourcesForAsset()

    def ActivateCamera(self, index: int, mainCam: Camera) -> None:     # :660-680
        """Pose `mainCam` as camera `index` of the asset's cameras.json: parented to this renderer's transform with
        localPosition = cam.pos and localRotation = LookRotation(cam.axisZ, cam.axisY), then unparented keeping its world pose,
        scale one.  World position = localToWorld * pos.  World rotation is Unity's Transform.rotation of a child: parent.rotation *
        ScaleMulQuat(parent.localScale, localRotation) -- the local rotation conjugated by the SIGNS of the parent's scale, which
        is what makes the importer's negated y / z camera axes come out looking at the scene under the sample scene's mirrored
        (scale z = -1) splat object (GSTestScene.unity:363-365)."""
        from .camera import look_rotation, quat_to_mat3
        if mainCam is None or self.m_Asset is None or not self.m_Asset.cameras:
            return
        ci = self.m_Asset.cameras[index]
        o2w = self.transform.localToWorldMatrix.astype(np.float64)
        pos = o2w @ np.array([ci.pos[0], ci.pos[1], ci.pos[2], 1.0])
        mainCam.position = tuple(float(v) for v in pos[:3])
        sgn = np.diag(np.sign(np.asarray(self.transform.scale, np.float64)))
        mainCam.rotation = quat_to_mat3(self.transform.rotation) @ (sgn @ look_rotation(ci.axisZ, ci.axisY) @ sgn)

    # -- per frame ------------------------------------------------------------------------------------------
    def FrameParams(self, cam: Camera) -> gs_frame_params:
        return frame_params(cam, self.transform, self.m_SplatScale, self.m_OpacityScale, self.m_SHOrder, self.m_SHOnly)

    def ResetOrder(self) -> None:                   # CSSetIndices, :434-438
        check(_lib.lib().gs_renderer_reset_order(self._r_h), "gs_renderer_reset_order")

    def SortPoints(self, cam: Camera, matrix: Optional[np.ndarray] = None) -> None:     # :612-639
        if matrix is None:
            matrix = self.transform.localToWorldMatrix
        m = np.ascontiguousarray(sort_matrix(cam, matrix), np.float32).reshape(16)
        check(_lib.lib().gs_renderer_sort(self._r_h, _fptr(m)), "gs_renderer_sort")

    def UpdateCutoutsBuffer(self) -> None:          # :742-764 (+ _SplatCutoutsCount, :508)
        arr, n = shader_data_array(self.m_Cutouts, self.transform.localToWorldMatrix)
        check(_lib.lib().gs_renderer_set_cutouts(self._r_h, arr, n), "gs_renderer_set_cutouts")

    def SetDeletedBits(self, bits: Optional[np.ndarray]) -> None:
        """The m_GpuEditDeleted buffer (:269,779): one bit per splat, ceil(N/32) uint32 words; None = no edit buffers
        (_SplatBitsValid = 0).  EditDeleteSelected fills it on the GPU; this call overwrites it from the host."""
        if bits is None:
            check(_lib.lib().gs_renderer_set_deleted_bits(self._r_h, None, 0), "gs_renderer_set_deleted_bits")
            return
        w = np.ascontiguousarray(bits, np.uint32)
        check(_lib.lib().gs_renderer_set_deleted_bits(self._r_h, w.ctypes.data, len(w)), "gs_renderer_set_deleted_bits")

    # -- editing: selection and deletion (:705-740, 767-840, 896-934) --------------------------------------------
    def UpdateEditCountsAndBounds(self) -> None:    # :705-740
        if not self.m_GpuEditSelected:
            self.editSelectedSplats = self.editDeletedSplats = self.editCutSplats = 0
            self.editModified = False
            self.editSelectedBounds = Bounds()
            return
        self.UpdateCutoutsBuffer()                  # SetAssetDataOnCS, :507
        info = gs_edit_info()
        check(_lib.lib().gs_renderer_edit_info(self._r_h, C.byref(info)), "gs_renderer_edit_info")
        self.editSelectedSplats, self.editDeletedSplats, self.editCutSplats = info.selected, info.deleted, info.cut
        bounds = Bounds()
        bounds.SetMinMax(np.array(info.bounds_min[:], np.float32), np.array(info.bounds_max[:], np.float32))
        e = bounds.extents
        with np.errstate(over="ignore", invalid="ignore"):
            sqr = np.float32(np.float32(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        if float(sqr) < 0.01:
            bounds.extents = np.full(3, 0.1, np.float32)
        self.editSelectedBounds = bounds

    def EnsureEditingBuffers(self) -> bool:         # :767-786 (the native renderer makes the buffers at the edit call that follows)
        if not self.HasValidAsset or not self.HasValidRenderSetup:
            return False
        self.m_GpuEditSelected = True
        return True

    def EditStoreSelectionMouseDown(self) -> None:  # :788-792
        if not self.EnsureEditingBuffers():
            return
        check(_lib.lib().gs_renderer_edit_store_selection(self._r_h), "gs_renderer_edit_store_selection")

    def EditUpdateSelection(self, rectMin, rectMax, cam: Camera, subtract: bool) -> None:     # :811-840
        """rectMin / rectMax: the corners of the drag in pixels, x right and y up from the bottom edge, as the reference's tool hands them in
        (rectMin = its top-left corner: the smaller x, the larger y)."""
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()
        p = self.FrameParams(cam)
        rect = np.array([rectMin[0], rectMax[1], rectMax[0], rectMin[1]], np.float32)       # :835
        check(_lib.lib().gs_renderer_edit_update_selection(self._r_h, C.byref(p), _fptr(rect), int(bool(subtract))), "gs_renderer_edit_update_selection")
        self.UpdateEditCountsAndBounds()

    def EditSelectSurface(self, target: "RenderTarget", rect, subtract: bool = False) -> None:
        """Select what one SEES: rect = (x0, y0, x1, y1), inclusive pixels, y down, clipped to the target (a click: x0 == x1, y0 == y1).  Every pixel whose
        pick record carries this renderer's tag names a splat; those that are neither deleted nor cut are added to the selection, or with subtract
        removed from it (gs_renderer_edit_select_surface).  The target needs SetPickOutput(True) and a splat frame drawn into it."""
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()
        x0, y0, x1, y1 = (int(v) for v in rect)
        check(_lib.lib().gs_renderer_edit_select_surface(self._r_h, target._h, x0, y0, x1, y1, int(bool(subtract))), "gs_renderer_edit_select_surface")
        self.UpdateEditCountsAndBounds()

    def EditUpdateSelectionMask(self, params, mask: "ScreenMask", subtract: bool = False) -> None:
        """The lasso counterpart of EditUpdateSelection: selected = the mouse-down copy plus (subtract: minus) every splat whose centre lands on a set
        pixel of `mask` (gs_renderer_edit_update_selection_mask).  params: a camera, or the gs_frame_params of one; its screen must be the mask's size.
        EditStoreSelectionMouseDown at mouse-down, this on every mouse move."""
        if not self.HasValidAsset or not self.HasValidRenderSetup:
            return
        self.UpdateCutoutsBuffer()
        p = params if isinstance(params, gs_frame_params) else self.FrameParams(params)
        check(_lib.lib().gs_renderer_edit_update_selection_mask(self._r_h, C.byref(p), mask._h, int(bool(subtract))), "gs_renderer_edit_update_selection_mask")
        self.m_GpuEditSelected = True               # (a refused call made no edit buffers)
        self.UpdateEditCountsAndBounds()

    def EditSelectSurfaceMask(self, target: "RenderTarget", mask: "ScreenMask", subtract: bool = False) -> None:
        """EditSelectSurface over every pixel whose bit in `mask` is set, in place of a rectangle (gs_renderer_edit_select_surface_mask); the mask
        must have the target's size."""
        if not self.HasValidAsset or not self.HasValidRenderSetup:
            return
        self.UpdateCutoutsBuffer()
        check(_lib.lib().gs_renderer_edit_select_surface_mask(self._r_h, target._h, mask._h, int(bool(subtract))), "gs_renderer_edit_select_surface_mask")
        self.m_GpuEditSelected = True
        self.UpdateEditCountsAndBounds()

    def _gesture_mask(self, p: gs_frame_params) -> "ScreenMask":
        w, h = int(p.screen_w), int(p.screen_h)
        m = getattr(self, "_screen_mask", None)
        if m is None or not m._h or (m.width, m.height) != (w, h):
            if m is not None:
                m.Dispose()
            m = self._screen_mask = ScreenMask(self.ctx, w, h)
        return m

    def EditSelectPolygon(self, params, points, subtract: bool = False) -> None:
        """The lasso / polygon tool in one call: a cached mask of the screen's size is cleared, filled with the outline and selected through."""
        p = params if isinstance(params, gs_frame_params) else self.FrameParams(params)
        m = self._gesture_mask(p)
        m.Clear()
        m.FillPolygon(points)
        self.EditUpdateSelectionMask(p, m, subtract)

    def EditSelectBrush(self, params, points, radius: float, subtract: bool = False) -> None:
        """The brush tool in one call: the cached mask is cleared, the stroke drawn and selected through."""
        p = params if isinstance(params, gs_frame_params) else self.FrameParams(params)
        m = self._gesture_mask(p)
        m.Clear()
        m.Stroke(points, radius)
        self.EditUpdateSelectionMask(p, m, subtract)

    def EditNeighbourCounts(self, radius: float, cap: int = 65535) -> np.ndarray:
        """For every alive splat -- not deleted, not cut -- min(cap, the other alive splats within `radius` of it), boundary included; 0xFFFFFFFF for a
        splat that is not alive.  `radius` is in object space, the space of the positions.  What an editor draws a histogram of before it picks the
        threshold of EditSelectSparse (gs_renderer_edit_neighbour_counts).  Changes nothing; blocks."""
        self.UpdateCutoutsBuffer()
        out = np.zeros(self.m_SplatCount, np.uint32)
        check(_lib.lib().gs_renderer_edit_neighbour_counts(self._r_h, float(radius), int(cap), out.ctypes.data, len(out)), "gs_renderer_edit_neighbour_counts")
        return out

    def EditSelectSparse(self, radius: float, minNeighbours: int, subtract: bool = False) -> None:
        """Select the floaters: every alive splat with fewer than minNeighbours other alive splats within `radius` (object space) is added to the
        selection, or with subtract removed from it (gs_renderer_edit_select_sparse).  Blocks."""
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()
        check(_lib.lib().gs_renderer_edit_select_sparse(self._r_h, float(radius), int(minNeighbours), int(bool(subtract))), "gs_renderer_edit_select_sparse")
        self.UpdateEditCountsAndBounds()

    def EditComponents(self, radius: float):
        """The connected components of the graph that joins two alive splats within `radius` (object space) of each other: (labels, sizes), per alive
        splat the smallest splat index of its component and the number of splats in it; 0xFFFFFFFF and 0 for a splat that is not alive
        (gs_renderer_edit_components).  Changes nothing; blocks."""
        self.UpdateCutoutsBuffer()
        labels, sizes = np.zeros(self.m_SplatCount, np.uint32), np.zeros(self.m_SplatCount, np.uint32)
        check(_lib.lib().gs_renderer_edit_components(self._r_h, float(radius), labels.ctypes.data, sizes.ctypes.data, len(labels)), "gs_renderer_edit_components")
        return labels, sizes

    def EditSelectIslands(self, radius: float, minSize: int, subtract: bool = False) -> None:
        """Select the clumps: every alive splat whose component (EditComponents) has fewer than minSize splats is added to the selection, or with
        subtract removed from it (gs_renderer_edit_select_islands).  Blocks."""
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()
        check(_lib.lib().gs_renderer_edit_select_islands(self._r_h, float(radius), int(minSize), int(bool(subtract))), "gs_renderer_edit_select_islands")
        self.UpdateEditCountsAndBounds()

    def EditGrowSelection(self, radius: float) -> None:
        """Click, then grow: every alive splat connected to a selected alive splat (through splats within `radius` of each other) joins the selection
        (gs_renderer_edit_grow_selection).  Blocks."""
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()
        check(_lib.lib().gs_renderer_edit_grow_selection(self._r_h, float(radius)), "gs_renderer_edit_grow_selection")
        self.UpdateEditCountsAndBounds()

    # -- editing: selection by attribute (no counterpart in the reference) ------------------------
    @staticmethod
    def _attr_point(point):
        """(keep-alive array or None, the pointer the C call takes): `point` is read for SplatAttribute.Dist2 only"""
        if point is None:
            return None, None
        a = np.ascontiguousarray(point, np.float32).reshape(3)
        return a, a.ctypes.data

    def EditAttributeValues(self, attr, point=None) -> np.ndarray:
        """value(i, attr) of every alive splat -- not deleted, not cut -- as float32; the word 0xFFFFFFFF (a NaN) for a splat that is not alive: view
        the result as uint32 to tell it from a value (gs_renderer_edit_attribute_values).  Changes nothing; blocks."""
        self.UpdateCutoutsBuffer()
        out = np.zeros(self.m_SplatCount, np.float32)
        keep, p = self._attr_point(point)
        check(_lib.lib().gs_renderer_edit_attribute_values(self._r_h, int(attr), p, out.ctypes.data, len(out)), "gs_renderer_edit_attribute_values")
        return out

    def EditSelectRange(self, attr, lo: float, hi: float, subtract: bool = False, point=None) -> None:
        """Every alive splat with lo <= value <= hi is added to the selection, or with subtract removed from it; +-inf bounds are allowed, lo > hi
        selects nothing (gs_renderer_edit_select_range)."""
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()
        keep, p = self._attr_point(point)
        check(_lib.lib().gs_renderer_edit_select_range(self._r_h, int(attr), p, float(lo), float(hi), int(bool(subtract))), "gs_renderer_edit_select_range")
        self.UpdateEditCountsAndBounds()

    def EditAttributeStats(self, attr, selectedOnly: bool = False, point=None) -> gs_attribute_stats:
        """members (the alive splats, or with selectedOnly the selected alive ones), nans (those whose value is NaN), vmin / vmax over the rest
        (+inf / -inf if there is none) (gs_renderer_edit_attribute_stats).  Blocks."""
        self.UpdateCutoutsBuffer()
        out = gs_attribute_stats()
        keep, p = self._attr_point(point)
        check(_lib.lib().gs_renderer_edit_attribute_stats(self._r_h, int(attr), p, GS_SCOPE_SELECTED if selectedOnly else GS_SCOPE_ALIVE, C.byref(out)),
              "gs_renderer_edit_attribute_stats")
        return out

    def EditAttributeHistogram(self, attr, lo: float, hi: float, bins: int, selectedOnly: bool = False, point=None):
        """(hist[bins], below, above, nans): the members' values counted in `bins` equal bins over [lo, hi] (hi itself in the last), those below lo,
        above hi and NaN apart (gs_renderer_edit_attribute_histogram).  Blocks."""
        self.UpdateCutoutsBuffer()
        out = np.zeros(int(bins) + 3, np.uint32)
        keep, p = self._attr_point(point)
        check(_lib.lib().gs_renderer_edit_attribute_histogram(self._r_h, int(attr), p, GS_SCOPE_SELECTED if selectedOnly else GS_SCOPE_ALIVE, float(lo), float(hi), int(bins),
                                                              out.ctypes.data, len(out)), "gs_renderer_edit_attribute_histogram")
        bins = int(bins)
        return out[:bins].copy(), int(out[bins]), int(out[bins + 1]), int(out[bins + 2])

    def EditAttributeRanks(self, attr, ranks, selectedOnly: bool = False, point=None):
        """(values, population): the members whose value is not NaN, sorted ascending (-0 before +0); values[k] is the one at position ranks[k], the
        word 0xFFFFFFFF where ranks[k] >= population.  At most 4096 ranks; none returns the population alone (gs_renderer_edit_attribute_ranks).  Blocks."""
        self.UpdateCutoutsBuffer()
        rk = np.ascontiguousarray(ranks, np.uint32).reshape(-1)
        out = np.zeros(len(rk), np.float32)
        pop = C.c_uint32(0)
        keep, p = self._attr_point(point)
        check(_lib.lib().gs_renderer_edit_attribute_ranks(self._r_h, int(attr), p, GS_SCOPE_SELECTED if selectedOnly else GS_SCOPE_ALIVE, rk.ctypes.data if len(rk) else None,
                                                          len(rk), out.ctypes.data if len(rk) else None, C.byref(pop)), "gs_renderer_edit_attribute_ranks")
        return out, int(pop.value)

    def EditAttributeQuantiles(self, attr, fractions, selectedOnly: bool = False, point=None):
        """A convenience composed of two EditAttributeRanks calls: the population from one with no ranks, then the values at rank
        min(population - 1, floor(f * population)) (float64) for every f of `fractions`.  (values, population); an empty population gives no values."""
        _, pop = self.EditAttributeRanks(attr, [], selectedOnly, point)
        f = np.asarray(fractions, np.float64).reshape(-1)
        if pop == 0:
            return np.zeros(0, np.float32), 0
        ranks = np.minimum(pop - 1, np.floor(f * np.float64(pop))).astype(np.uint32)
        return self.EditAttributeRanks(attr, ranks, selectedOnly, point)[0], pop

    def EditSelectTop(self, attr, fraction: float, largest: bool = True, subtract: bool = False, point=None) -> None:
        """A convenience composed of EditAttributeQuantiles and EditSelectRange: the `fraction` of the alive splats with the largest (or smallest)
        values -- the quantile's value, then the range from it to +inf (from -inf to it).  Ties at the threshold are all taken."""
        q = 1.0 - float(fraction) if largest else float(fraction)
        values, pop = self.EditAttributeQuantiles(attr, [min(max(q, 0.0), 1.0)], False, point)
        if pop == 0:
            return
        t = float(values[0])
        self.EditSelectRange(attr, t if largest else -np.inf, np.inf if largest else t, subtract, point)

    def EditDeleteSelected(self) -> None:           # :896-904
        if not self.EnsureEditingBuffers():
            return
        check(_lib.lib().gs_renderer_edit_delete_selected(self._r_h), "gs_renderer_edit_delete_selected")     # UnionGraphicsBuffers + EditDeselectAll
        self.UpdateEditCountsAndBounds()
        if self.editDeletedSplats != 0:
            self.editModified = True

    def EditSelectAll(self) -> None:                # :906-915
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()
        check(_lib.lib().gs_renderer_edit_select_all(self._r_h), "gs_renderer_edit_select_all")
        self.UpdateEditCountsAndBounds()

    def EditDeselectAll(self) -> None:              # :917-922
        if not self.EnsureEditingBuffers():
            return
        check(_lib.lib().gs_renderer_edit_deselect_all(self._r_h), "gs_renderer_edit_deselect_all")
        self.UpdateEditCountsAndBounds()

    def EditInvertSelection(self) -> None:          # :924-934
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()
        check(_lib.lib().gs_renderer_edit_invert_selection(self._r_h), "gs_renderer_edit_invert_selection")
        self.UpdateEditCountsAndBounds()

    def DownloadEditBits(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(selected, selected at mouse-down, deleted): ceil(N/32) uint32 words each; a buffer that does not exist reads as zeros.  Blocks."""
        n = (self.m_SplatCount + 31) // 32
        out = [np.zeros(n, np.uint32) for _ in range(3)]
        check(_lib.lib().gs_renderer_edit_download_bits(self._r_h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, n), "gs_renderer_edit_download_bits")
        return out[0], out[1], out[2]

    def UploadSelectedBits(self, bits: np.ndarray) -> None:
        """The selection from the host: ceil(N/32) uint32 words."""
        if not self.EnsureEditingBuffers():
            return
        w = np.ascontiguousarray(bits, np.uint32)
        check(_lib.lib().gs_renderer_edit_upload_selected_bits(self._r_h, w.ctypes.data, len(w)), "gs_renderer_edit_upload_selected_bits")
        self.UpdateEditCountsAndBounds()

    # -- editing: moving the selection (:794-809, 842-894) -----------------------------------------------------------
    def EditStorePosMouseDown(self) -> None:        # :794-801
        check(_lib.lib().gs_renderer_edit_store_pos_mouse_down(self._r_h), "gs_renderer_edit_store_pos_mouse_down")
        self.m_GpuEditPosMouseDown = True

    def EditStoreOtherMouseDown(self) -> None:      # :802-809
        check(_lib.lib().gs_renderer_edit_store_other_mouse_down(self._r_h), "gs_renderer_edit_store_other_mouse_down")
        self.m_GpuEditOtherMouseDown = True

    def EditStoreSHMouseDown(self) -> None:
        """The third mouse-down copy: the renderer's current SH blob (gs_renderer_edit_store_sh_mouse_down), read by a rotate while
        EditSetRigidTransforms is on.  192 bytes per splat where the asset passes the rotation gate, nothing elsewhere."""
        check(_lib.lib().gs_renderer_edit_store_sh_mouse_down(self._r_h), "gs_renderer_edit_store_sh_mouse_down")
        self.m_GpuEditSHMouseDown = True

    def EditSetRigidTransforms(self, enabled: bool) -> None:
        """True: EditRotateSelection also turns every selected splat's orientation and SH with the object and EditScaleSelection with a uniform
        scale (s, s, s) also multiplies the splats' own sizes by |s| -- what the reference's @TODOs leave out (gs_renderer_edit_set_rigid_transforms;
        DESIGN.md section 4.15).  False (default): the reference's kernels word for word."""
        self.rigidTransforms = bool(enabled)
        if self._r_h:
            check(_lib.lib().gs_renderer_edit_set_rigid_transforms(self._r_h, int(self.rigidTransforms)), "gs_renderer_edit_set_rigid_transforms")

    def EditTranslateSelection(self, localSpacePosDelta) -> None:      # :842-854
        if not self.EnsureEditingBuffers():
            return
        d = np.ascontiguousarray(localSpacePosDelta, np.float32).reshape(3)
        check(_lib.lib().gs_renderer_edit_translate_selection(self._r_h, _fptr(d)), "gs_renderer_edit_translate_selection")
        self.UpdateEditCountsAndBounds()
        self.editModified = True

    def EditRotateSelection(self, localSpaceCenter, localToWorld, worldToLocal, rotation) -> None:      # :856-874
        """localToWorld / worldToLocal: 4x4 matrices as camera.Transform hands them out; rotation: a quaternion x y z w"""
        if not self.EnsureEditingBuffers():
            return
        if not self.m_GpuEditPosMouseDown or not self.m_GpuEditOtherMouseDown:
            return                                  # should have captured initial state
        if self.rigidTransforms and not self.m_GpuEditSHMouseDown:
            return                                  # ... all three of them
        c = np.ascontiguousarray(localSpaceCenter, np.float32).reshape(3)
        l2w = np.ascontiguousarray(localToWorld, np.float32).reshape(16)
        w2l = np.ascontiguousarray(worldToLocal, np.float32).reshape(16)
        q = np.ascontiguousarray(rotation, np.float32).reshape(4)
        check(_lib.lib().gs_renderer_edit_rotate_selection(self._r_h, _fptr(c), _fptr(l2w), _fptr(w2l), _fptr(q)), "gs_renderer_edit_rotate_selection")
        self.UpdateEditCountsAndBounds()
        self.editModified = True

    def EditScaleSelection(self, localSpaceCenter, localToWorld, worldToLocal, scale) -> None:      # :877-894
        if not self.EnsureEditingBuffers():
            return
        if not self.m_GpuEditPosMouseDown:
            return                                  # should have captured initial state
        c = np.ascontiguousarray(localSpaceCenter, np.float32).reshape(3)
        l2w = np.ascontiguousarray(localToWorld, np.float32).reshape(16)
        w2l = np.ascontiguousarray(worldToLocal, np.float32).reshape(16)
        v = np.ascontiguousarray(scale, np.float32).reshape(3)
        if self.rigidTransforms and v[0] == v[1] == v[2] and not self.m_GpuEditOtherMouseDown:
            return                                  # the uniform handle scales the splats' own sizes from their mouse-down values
        check(_lib.lib().gs_renderer_edit_scale_selection(self._r_h, _fptr(c), _fptr(l2w), _fptr(w2l), _fptr(v)), "gs_renderer_edit_scale_selection")
        self.UpdateEditCountsAndBounds()
        self.editModified = True

    # -- editing: undo and redo (no counterpart in the reference, which has none) ------------------
    def EditHistoryEnable(self, maxBytes: int) -> None:
        """Switches the edit history on with a budget of maxBytes of device memory for its entries (0: off, every entry freed).  Off by default."""
        check(_lib.lib().gs_renderer_edit_history_enable(self._r_h, int(maxBytes)), "gs_renderer_edit_history_enable")

    def EditCheckpoint(self, what=EditHistoryFlags.Selection | EditHistoryFlags.Deleted | EditHistoryFlags.Transform) -> None:
        """Before a gesture, where the reference's tools call EditStore*MouseDown: captures the bit buffers named in `what` whole and the pos / other / SH
        records of the splats selected NOW, which is exactly what a later EditUndo restores.  Blocks (one 4-byte readback sizes the entry)."""
        check(_lib.lib().gs_renderer_edit_checkpoint(self._r_h, int(what)), "gs_renderer_edit_checkpoint")
        if int(what) & ~int(EditHistoryFlags.Deleted):
            self.m_GpuEditSelected = True           # (the native call made the edit buffers)

    def _history_step(self, fn, where) -> None:
        depth = self.EditHistoryInfo()
        check(fn(self._r_h), where)
        if depth.undo_depth + depth.redo_depth:
            self.m_GpuEditSelected = True           # an entry with the selection makes released edit buffers again
            self.UpdateEditCountsAndBounds()
            self.editModified = True

    def EditUndo(self) -> None:
        """The entry of the last checkpoint changes places with the renderer's state (asynchronous); nothing to undo: nothing happens."""
        self._history_step(_lib.lib().gs_renderer_edit_undo, "gs_renderer_edit_undo")

    def EditRedo(self) -> None:
        self._history_step(_lib.lib().gs_renderer_edit_redo, "gs_renderer_edit_redo")

    def EditHistoryClear(self) -> None:
        check(_lib.lib().gs_renderer_edit_history_clear(self._r_h), "gs_renderer_edit_history_clear")

    def EditHistoryInfo(self) -> gs_edit_history_info:
        info = gs_edit_history_info()
        check(_lib.lib().gs_renderer_edit_history_info(self._r_h, C.byref(info)), "gs_renderer_edit_history_info")
        return info

    def EditGesture(self, what=EditHistoryFlags.Selection | EditHistoryFlags.Deleted | EditHistoryFlags.Transform):
        """`with r.EditGesture(): ...` -- a checkpoint on entry, so that one EditUndo takes back everything the block did to the captured state."""
        return _EditGesture(self, what)

    def _blob_sizes(self) -> Tuple[int, int, int, int]:
        """bytes of the renderer's current pos / other / color / sh blobs: the asset's until the first resize, from then on -- also back at the
        asset's own count -- those of the VeryHigh layout at splatCount (whole records only, where the importer pads its blobs)"""
        a, n = self.m_Asset, self.m_SplatCount
        if not self.m_Resized:
            return len(a.posData), len(a.otherData), len(a.colorData), len(a.shData)
        w, h = CalcTextureSize(n)
        return 12 * n, 16 * n, w * h * 16, 192 * n

    def DownloadPosOther(self) -> Tuple[np.ndarray, np.ndarray]:
        """The renderer's current pos / other blobs as bytes (its private copies once it has been transformed, else the asset's).  Blocks."""
        sizes = self._blob_sizes()
        pos, other = np.zeros(sizes[0], np.uint8), np.zeros(sizes[1], np.uint8)
        check(_lib.lib().gs_renderer_edit_download_pos_other(self._r_h, pos.ctypes.data, pos.nbytes, other.ctypes.data, other.nbytes), "gs_renderer_edit_download_pos_other")
        return pos, other

    # -- editing: the merge (:960-1075; GaussianSplatRendererEditor.cs:213-235) ---------------------------------------
    def _native_splat_count(self) -> int:
        n = C.c_uint32(0)
        check(_lib.lib().gs_renderer_splat_count(self._r_h, C.byref(n)), "gs_renderer_splat_count")
        return int(n.value)

    def EditSetSplatCount(self, newSplatCount: int) -> None:      # :960-1031
        """Resizes the renderer: new zero-filled buffers of newSplatCount splats with the old splats copied into them (shrinking truncates); the
        order, the view buffer, the selection and the mouse-down copies start over.  Returns silently where the C# logs an error.  The C# passes
        its copy kernel worldToLocal x localToWorld of the one transform, the identity but for rounding; this passes the exact identity.  Blocks."""
        newSplatCount = int(newSplatCount)
        if newSplatCount <= 0 or newSplatCount > kMaxSplats:
            return                                  # Invalid new splat count
        if not self.HasValidAsset or not self.HasValidRenderSetup:
            return
        if self.m_Asset.chunkCount != 0:
            return                                  # Only splats with VeryHigh quality can be resized
        if newSplatCount == self.splatCount:
            return
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()                  # SetAssetDataOnCS, :507
        check(_lib.lib().gs_renderer_edit_set_splat_count(self._r_h, newSplatCount, None), "gs_renderer_edit_set_splat_count")
        self.m_GpuEditPosMouseDown = self.m_GpuEditOtherMouseDown = self.m_GpuEditSHMouseDown = False      # DisposeBuffer(ref m_GpuEditPosMouseDown) ..., :1026-1027
        self.m_SplatCount = self._native_splat_count()
        self.m_Resized = True
        self.editModified = True

    def CopyParams(self, dst: "GaussianSplatRenderer") -> gs_copy_params:
        """What EditCopySplats hands CSCopySplats (:1052-1054): copyMatrix = dst.worldToLocal x this.localToWorld in float32, its rotation and
        its lossy scale (camera.matrix_rotation_scale)."""
        m = mat_mul(dst.transform.worldToLocalMatrix, self.transform.localToWorldMatrix)
        q, sc = matrix_rotation_scale(m)
        p = gs_copy_params()
        p.matrix[0:16] = [float(v) for v in np.asarray(m, np.float32).reshape(-1)]
        p.rotation[0:4] = [float(np.float32(v)) for v in q]
        p.scale[0:3] = [float(np.float32(v)) for v in sc]
        return p

    def EditCopySplatsInto(self, dst: "GaussianSplatRenderer", copySrcStartIndex: int, copyDstStartIndex: int, copyCount: int) -> None:      # :1033-1075
        if not self.EnsureEditingBuffers():
            return
        self.UpdateCutoutsBuffer()                  # SetAssetDataOnCS, :507
        p = self.CopyParams(dst)
        check(_lib.lib().gs_renderer_edit_copy_splats_into(self._r_h, dst._r_h, C.byref(p), int(copySrcStartIndex), int(copyDstStartIndex), int(copyCount)),
              "gs_renderer_edit_copy_splats_into")
        dst.editModified = True

    def DownloadSplatData(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The renderer's current pos / other / color / sh blobs as bytes (private copies where they exist, else the asset's).  Blocks."""
        out = [np.zeros(b, np.uint8) for b in self._blob_sizes()]
        check(_lib.lib().gs_renderer_edit_download_splat_data(self._r_h, out[0].ctypes.data, out[0].nbytes, out[1].ctypes.data, out[1].nbytes,
                                                              out[2].ctypes.data, out[2].nbytes, out[3].ctypes.data, out[3].nbytes), "gs_renderer_edit_download_splat_data")
        return out[0], out[1], out[2], out[3]

    # -- editing: export (:936-958; GaussianSplatRendererEditor.cs:394-445) ------------------------------------------
    def ExportParams(self, bakeTransform: bool) -> gs_export_params:
        """What EditExportData hands CSExportData: transform.localRotation, localScale and localToWorldMatrix, and the bake flag."""
        p = gs_export_params()
        tr = self.transform
        p.matrix_object_to_world[0:16] = [float(v) for v in np.asarray(tr.localToWorldMatrix, np.float32).reshape(-1)]
        p.rotation[0:4] = [float(np.float32(v)) for v in tr.rotation]
        p.scale[0:3] = [float(np.float32(v)) for v in tr.scale]
        p.bake_transform = 1 if bakeTransform else 0
        return p

    def EditExportData(self, bakeTransform: bool = False) -> np.ndarray:      # :936-958
        """All N records of CSExportData, [N, 62] float32 (creator.PLY_ATTRS), nor = 1 for the cut splats.  Blocks."""
        self.UpdateCutoutsBuffer()                  # SetAssetDataOnCS, :507
        out = np.zeros((self.m_SplatCount, 62), np.float32)
        p = self.ExportParams(bakeTransform)
        check(_lib.lib().gs_renderer_edit_export_data(self._r_h, C.byref(p), out.ctypes.data, out.nbytes, 0), "gs_renderer_edit_export_data")
        return out

    def ExportAlive(self, bakeTransform: bool = False) -> np.ndarray:
        """The records of the splats that are neither deleted nor cut, in index order: [alive, 62] float32.  Blocks."""
        self.UpdateCutoutsBuffer()
        p = self.ExportParams(bakeTransform)
        alive = C.c_uint32(0)
        check(_lib.lib().gs_renderer_edit_export_alive(self._r_h, C.byref(p), None, 0, C.byref(alive)), "gs_renderer_edit_export_alive")
        out = np.zeros((alive.value, 62), np.float32)
        if alive.value:
            check(_lib.lib().gs_renderer_edit_export_alive(self._r_h, C.byref(p), out.ctypes.data, alive.value, C.byref(alive)), "gs_renderer_edit_export_alive")
        return out

    def ExportPlyFile(self, path: str, bakeTransform: bool = False) -> int:   # GaussianSplatRendererEditor.cs:394-445
        """Writes the alive splats as a PLY file the importer reads back; returns their number.  Blocks."""
        self.UpdateCutoutsBuffer()
        p = self.ExportParams(bakeTransform)
        alive = C.c_uint32(0)
        check(_lib.lib().gs_renderer_edit_export_ply(self._r_h, C.byref(p), os.fsencode(path), C.byref(alive)), "gs_renderer_edit_export_ply")
        return int(alive.value)

    # -- editing: export to SPZ (no counterpart in the reference, which only reads the format) ----------------------------------------
    @staticmethod
    def SpzParams(shLevel: int = 3, fractBits=None, level: int = -1, sliceBytes: int = 0) -> gs_spz_params:
        """fractBits None = automatic: the largest value up to 12 at which the largest exported |coordinate| still fits 24 bits"""
        s = gs_spz_params()
        s.sh_level, s.fract_bits = int(shLevel), GS_SPZ_FRACT_AUTO if fractBits is None else int(fractBits)
        s.compression_level, s.slice_bytes = int(level), int(sliceBytes)
        return s

    def ExportSpzBody(self, bakeTransform: bool = False, shLevel: int = 3, fractBits=None, sliceBytes: int = 0):
        """The gunzipped SPZ stream (16-byte header + six columns) of the splats that are neither deleted nor cut:
        (np.uint8 array, alive, fract_bits used).  Blocks."""
        self.UpdateCutoutsBuffer()
        p, s = self.ExportParams(bakeTransform), self.SpzParams(shLevel, fractBits, -1, sliceBytes)
        size, alive, fract = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        fn = _lib.lib().gs_renderer_edit_export_spz_body
        check(fn(self._r_h, C.byref(p), C.byref(s), None, 0, C.byref(size), C.byref(alive), C.byref(fract)), "gs_renderer_edit_export_spz_body")
        out = np.zeros(size.value, np.uint8)
        check(fn(self._r_h, C.byref(p), C.byref(s), out.ctypes.data, out.nbytes, C.byref(size), C.byref(alive), C.byref(fract)), "gs_renderer_edit_export_spz_body")
        return out, int(alive.value), int(fract.value)

    def ExportSpzFile(self, path: str, bakeTransform: bool = False, shLevel: int = 3, fractBits=None, level: int = -1, sliceBytes: int = 0) -> int:
        """Writes the alive splats as an SPZ file (gzip level -1..9) that ReadSPZ / CreateGpuAssetFromFile read back; returns their number.  Blocks."""
        self.UpdateCutoutsBuffer()
        p, s = self.ExportParams(bakeTransform), self.SpzParams(shLevel, fractBits, level, sliceBytes)
        alive = C.c_uint32(0)
        check(_lib.lib().gs_renderer_edit_export_spz(self._r_h, C.byref(p), C.byref(s), os.fsencode(path), C.byref(alive)), "gs_renderer_edit_export_spz")
        return int(alive.value)

    # -- editing: bake (no counterpart in the reference, whose way back is ExportPlyFile + the importer) -------------------------------
    def BakeFormats(self, quality="Medium", formatPos=None, formatScale=None, formatColor=None, formatSH=None, morton=True) -> gs_import_formats:
        from .creator import QUALITY
        fp, fs, fc, fsh = QUALITY[quality]
        fp = VectorFormat(fp if formatPos is None else formatPos)
        fs = VectorFormat(fs if formatScale is None else formatScale)
        fc = ColorFormat(fc if formatColor is None else formatColor)
        fsh = SHFormat(fsh if formatSH is None else formatSH)
        return gs_import_formats(int(fp), int(fs), int(fc), int(fsh), 0, int(bool(morton)))

    def EditBakeAsset(self, quality="Medium", *, formatPos=None, formatScale=None, formatColor=None, formatSH=None, morton=True) -> GpuAsset:
        """The alive splats (not deleted, not cut) of the renderer as it is now -- edits, private blobs and all -- as a new device-resident asset in
        the formats of `quality` (or the ones given), Morton-reordered and chunked like an imported one: the bytes the importer makes of
        ExportAlive's splats, without leaving the GPU.  The renderer itself is left as it is.  A Cluster* SH target ("Low"; the importer's palette
        of the alive splats' SH, computed on the GPU) needs more alive splats than table entries, as an import does.  Still refused: a BC7 colour
        target, hence the preset "VeryLow" as a whole -- EditBakeAsset("VeryLow", formatColor=ColorFormat.Norm8x4) works.  Blocks."""
        self.UpdateCutoutsBuffer()
        fmt = self.BakeFormats(quality, formatPos, formatScale, formatColor, formatSH, morton)
        h, alive = C.c_void_p(), C.c_uint32(0)
        bmin, bmax = (C.c_float * 3)(), (C.c_float * 3)()
        check(_lib.lib().gs_renderer_edit_bake_asset(self._r_h, C.byref(fmt), C.byref(h), C.byref(alive), bmin, bmax), "gs_renderer_edit_bake_asset")
        return GpuAsset(self.ctx, h, alive.value, (fmt.pos_format, fmt.scale_format, fmt.color_format, fmt.sh_format), tuple(bmin), tuple(bmax))

    def CalcViewData(self, cam: Camera) -> None:    # :579-610
        self.UpdateCutoutsBuffer()                  # SetAssetDataOnCS, :507
        p = self.FrameParams(cam)
        check(_lib.lib().gs_renderer_calc_view(self._r_h, C.byref(p)), "gs_renderer_calc_view")

    def Draw(self, cam: Camera, rt: RenderTarget) -> None:     # the DrawProcedural of :156-166
        check(_lib.lib().gs_renderer_set_blend_mode(self._r_h, int(self.blendMode)), "gs_renderer_set_blend_mode")
        check(_lib.lib().gs_renderer_set_render_mode(self._r_h, int(self.m_RenderMode), float(self.m_PointDisplaySize)), "gs_renderer_set_render_mode")
        p = self.FrameParams(cam)
        check(_lib.lib().gs_renderer_draw(self._r_h, C.byref(p), rt._h), "gs_renderer_draw")

    # -- the same three calls with constants the host has already built (a render loop that prepares its per-camera
    #    structs once, like Unity's own camera does, pays three ctypes calls per frame here) -----------------------------
    def SortMatrix(self, cam: Camera, matrix: Optional[np.ndarray] = None) -> np.ndarray:
        if matrix is None:
            matrix = self.transform.localToWorldMatrix
        return np.ascontiguousarray(sort_matrix(cam, matrix), np.float32).reshape(16)

    def SortPointsPrepared(self, m16: np.ndarray) -> None:
        check(_lib.lib().gs_renderer_sort(self._r_h, _fptr(m16)), "gs_renderer_sort")

    def CalcViewDataPrepared(self, p: gs_frame_params) -> None:
        check(_lib.lib().gs_renderer_calc_view(self._r_h, C.byref(p)), "gs_renderer_calc_view")

    def DrawPrepared(self, p: gs_frame_params, rt: RenderTarget) -> None:
        check(_lib.lib().gs_renderer_draw(self._r_h, C.byref(p), rt._h), "gs_renderer_draw")

    # -- parity / measurement hooks ---------------------------------------------------------------------------
    def SetViewBufferMode(self, every_frame: bool) -> None:
        """True: run the reference's full CSCalcViewData every frame (m_GpuView written); False (default): colours only for
        splats that reach the screen, m_GpuView materialised by DownloadView on demand."""
        check(_lib.lib().gs_renderer_set_view_buffer_mode(self._r_h, int(bool(every_frame))), "gs_renderer_set_view_buffer_mode")

    def SetSortMode(self, mode: SortMode) -> None:
        """SortMode.Visible: cull before sorting -- SortPoints only records its matrix and Draw sorts the splats CalcViewData found visible
        (same frame, same order among the drawn splats; include/gsplat_c.h gs_renderer_set_sort_mode for the conditions)."""
        self.sortMode = SortMode(mode)
        if self._r_h:
            check(_lib.lib().gs_renderer_set_sort_mode(self._r_h, int(self.sortMode)), "gs_renderer_set_sort_mode")

    def SetSelectionHighlight(self, enabled: bool) -> None:
        """True: splat frames draw the selected splats as the reference does (RenderGaussianSplats.shader:63-73,87-101: magenta tint, raised
        opacity, a solid outline ring) once the edit buffers exist; False (default): selection is not drawn (gs_renderer_set_selection_highlight)."""
        self.selectionHighlight = bool(enabled)
        if self._r_h:
            check(_lib.lib().gs_renderer_set_selection_highlight(self._r_h, int(self.selectionHighlight)), "gs_renderer_set_selection_highlight")

    def SetPickTag(self, tag: int) -> None:
        """What this renderer's draws write into the pick records they own (default 0): several renderers that share one target tell their
        records apart by it, and EditSelectSurface only considers the renderer's own (gs_renderer_set_pick_tag)."""
        self.pickTag = int(tag) & 0xFFFFFFFF
        if self._r_h:
            check(_lib.lib().gs_renderer_set_pick_tag(self._r_h, self.pickTag), "gs_renderer_set_pick_tag")

    def SetFramesInFlight(self, frames: int) -> None:
        """Frames (or the views of a batch of cameras) in flight INSIDE the library, behind this one renderer: `frames` lanes on streams of their own, dealt
        round-robin at every CalcViewData while SortMode.Visible draws splats -- one frame's latency-bound kernels under another's blend; the calls and the
        frames stay what they are with one frame at a time (gs_renderer_set_frames_in_flight).  1 = off (default)."""
        self.framesInFlight = int(frames)
        if self._r_h:
            check(_lib.lib().gs_renderer_set_frames_in_flight(self._r_h, int(frames)), "gs_renderer_set_frames_in_flight")

    def FramesInFlight(self):
        """(lanes set, True while the next CalcViewData goes to a lane)"""
        f, a = C.c_int32(), C.c_int32()
        check(_lib.lib().gs_renderer_frames_in_flight(self._r_h, C.byref(f), C.byref(a)), "gs_renderer_frames_in_flight")
        return f.value, bool(a.value)

    def SortModeActive(self) -> bool:
        """True while the visible-only path is what the next Draw uses (ABI 8: whenever the mode is set -- whatever the order buffer holds
        is the base its sorts start from)."""
        m, a = C.c_int32(), C.c_int32()
        check(_lib.lib().gs_renderer_sort_mode(self._r_h, C.byref(m), C.byref(a)), "gs_renderer_sort_mode")
        return bool(a.value)

    def SetSortHistoryLimit(self, rows: int) -> None:
        """SortMode.Visible: sort matrices recorded before the library carries them out on all N (2..128, default 128).  Same drawn order either way."""
        check(_lib.lib().gs_renderer_set_sort_history_limit(self._r_h, int(rows)), "gs_renderer_set_sort_history_limit")

    def SortHistory(self):
        """(matrices recorded since the base order, limit, consolidations so far)"""
        rows, limit, cons = C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(_lib.lib().gs_renderer_sort_history(self._r_h, C.byref(rows), C.byref(limit), C.byref(cons)), "gs_renderer_sort_history")
        return rows.value, limit.value, cons.value

    def DownloadVisibleOrder(self) -> np.ndarray:
        """SortMode.Visible: the depth-ordered indices of the visible splats (the visible subsequence of the reference's _OrderBuffer)."""
        out = np.empty(self.m_SplatCount, np.uint32)
        cnt = C.c_uint32()
        check(_lib.lib().gs_renderer_download_visible_order(self._r_h, out.ctypes.data, len(out), C.byref(cnt)), "gs_renderer_download_visible_order")
        return out[:cnt.value].copy()

    def SetProfiling(self, frames: int) -> None:
        """frames = 0 off; > 0: ring of per-frame hipEvent sets, averaged by StageTimes()."""
        check(_lib.lib().gs_renderer_set_profiling(self._r_h, int(frames)), "gs_renderer_set_profiling")

    def SetTileShape(self, tile_w: int = 0, tile_h: int = 0) -> None:
        """The compositor's tile, pixels: 16x16, 32x16 or 32x32; 0, 0 = automatic (per target size).  A performance knob: the frame
        is bit-identical whatever the shape."""
        check(_lib.lib().gs_renderer_set_tile_shape(self._r_h, int(tile_w), int(tile_h)), "gs_renderer_set_tile_shape")

    def TileShape(self, width: int, height: int) -> Tuple[int, int]:
        """(tile_w, tile_h) a draw into a width x height target composites with."""
        w, h = C.c_uint32(), C.c_uint32()
        check(_lib.lib().gs_renderer_tile_shape(self._r_h, int(width), int(height), C.byref(w), C.byref(h)), "gs_renderer_tile_shape")
        return w.value, h.value

    def SetKernelTiming(self, enabled: bool) -> None:
        """With profiling on: Onesweep launches carry their own start/stop timestamps (StageTimes().onesweep_*_kernel_ms); perturbs the stage brackets."""
        check(_lib.lib().gs_renderer_set_kernel_timing(self._r_h, int(bool(enabled))), "gs_renderer_set_kernel_timing")

    def PollPairs(self) -> Tuple[int, int]:
        """Non-blocking: (pair count of the most recent draw that started compositing, pair capacity); count > capacity = that draw was
        truncated (its farthest pairs dropped)."""
        p, c = C.c_uint64(), C.c_uint64()
        check(_lib.lib().gs_renderer_poll_pairs(self._r_h, C.byref(p), C.byref(c)), "gs_renderer_poll_pairs")
        return p.value, c.value

    def ReservePairs(self, n: int) -> None:
        check(_lib.lib().gs_renderer_reserve_pairs(self._r_h, n), "gs_renderer_reserve_pairs")

    def DownloadOrder(self) -> np.ndarray:
        out = np.empty(self.m_SplatCount, np.uint32)
        check(_lib.lib().gs_renderer_download_order(self._r_h, out.ctypes.data, len(out)), "gs_renderer_download_order")
        return out

    def UploadOrder(self, order: np.ndarray) -> None:
        o = np.ascontiguousarray(order, np.uint32)
        check(_lib.lib().gs_renderer_upload_order(self._r_h, o.ctypes.data, len(o)), "gs_renderer_upload_order")

    def DownloadDistances(self) -> np.ndarray:
        out = np.empty(self.m_SplatCount, np.uint32)
        check(_lib.lib().gs_renderer_download_distances(self._r_h, out.ctypes.data, len(out)), "gs_renderer_download_distances")
        return out

    def DownloadView(self) -> np.ndarray:
        out = np.empty(self.m_SplatCount, VIEW_DTYPE)
        check(_lib.lib().gs_renderer_download_view(self._r_h, out.ctypes.data, out.nbytes), "gs_renderer_download_view")
        return out

    def DownloadRasterRecords(self):
        """(recs N x 8 u32, rects N x 2 u32, vis_mask ceil(N/64) u64) as the per-frame calc_view launch left them."""
        n = self.m_SplatCount
        recs = np.empty((n, 8), np.uint32)
        rects = np.empty((n, 2), np.uint32)
        vis = np.empty((n + 63) // 64, np.uint64)
        check(_lib.lib().gs_renderer_download_raster_records(self._r_h, recs.ctypes.data, rects.ctypes.data, vis.ctypes.data),
              "gs_renderer_download_raster_records")
        return recs, rects, vis

    def FrameStats(self) -> gs_frame_stats:
        """Blocks.  Raises GsError(GS_ERR_PAIR_OVERFLOW) if the frame overflowed the pair buffer (it is grown: draw again)."""
        s = gs_frame_stats()
        check(_lib.lib().gs_renderer_frame_stats(self._r_h, C.byref(s)), "gs_renderer_frame_stats")
        return s

    def FrameTimes(self, capacity: int = 4096) -> np.ndarray:
        """GPU duration (ms) of every frame in the profiling ring; call before StageTimes (which resets the ring)."""
        out = np.zeros(capacity, np.float32)
        cnt = C.c_int32()
        check(_lib.lib().gs_renderer_frame_times(self._r_h, _fptr(out), capacity, C.byref(cnt)), "gs_renderer_frame_times")
        return out[:cnt.value].copy()

    def StageTimes(self) -> gs_stage_times:
        t = gs_stage_times()
        check(_lib.lib().gs_renderer_stage_times(self._r_h, C.byref(t)), "gs_renderer_stage_times")
        return t

    def __del__(self):
        try:
            self.DisposeResourcesForAsset()
        except Exception:
            pass


class _EditGesture:
    def __init__(self, renderer: GaussianSplatRenderer, what):
        self.renderer, self.what = renderer, what

    def __enter__(self) -> GaussianSplatRenderer:
        self.renderer.EditCheckpoint(self.what)
        return self.renderer

    def __exit__(self, *exc) -> bool:
        return False


class ViewsInFlight:
    """Several cameras (or consecutive frames) of ONE splat object side by side on one GPU (no counterpart in the reference, which records one camera
    after the other into one command buffer): `lanes` renderers on contexts (= HIP streams) of their own over one copy of the asset, all in
    SortMode.Visible, the views dealt round-robin.  SortPoints is bookkeeping in that mode, so every lane is told every view's matrix in the order the
    reference would sort them and each draws its views from the reference's order buffer: every target holds the bits a single renderer drawing
    the views one after the other would produce (tests/test_gpu_vissort.py), while one view's latency-bound sort / binning kernels run under
    another's VALU-bound blend (-20 % per view with two lanes)."""

    def __init__(self, renderer: "GaussianSplatRenderer", lanes: int = 2):
        assert lanes >= 1 and renderer.HasValidRenderSetup
        renderer.SetSortMode(SortMode.Visible)
        self.lanes = [renderer]
        for _ in range(lanes - 1):
            c = GpuContext(renderer.ctx.device)
            r = GaussianSplatRenderer(c, renderer.m_Asset)
            r.transform, r.sortMode = renderer.transform, SortMode.Visible
            r.ShareResourcesOf(renderer)
            self.lanes.append(r)
        self._targets = {}
        self._next = 0

    def _sync_fields(self):
        src = self.lanes[0]
        for r in self.lanes[1:]:
            for f in ("m_SplatScale", "m_OpacityScale", "m_SHOrder", "m_SHOnly", "m_RenderMode", "m_PointDisplaySize", "m_Cutouts", "blendMode", "transform"):
                setattr(r, f, getattr(src, f))

    def Target(self, lane: int, slot: int, W: int, H: int) -> RenderTarget:
        key = (lane, slot, W, H)
        if key not in self._targets:
            self._targets[key] = RenderTarget(self.lanes[lane].ctx, W, H)
        return self._targets[key]

    def Render(self, cams: Sequence[Camera], sort: bool = True) -> List[RenderTarget]:
        """SortPoints + CalcViewData + Draw for every camera, in order; returns one target per camera (owned by this object, reused by the next call
        with the same sizes: download or resolve them before calling again).  Nothing is synchronised here."""
        self._sync_fields()
        out = []
        for k, cam in enumerate(cams):
            if sort:
                for r in self.lanes:                         # every lane learns every matrix, in the reference's order
                    r.SortPoints(cam)
            li = self._next % len(self.lanes)
            self._next += 1
            r, rt = self.lanes[li], self.Target(li, k, cam.pixelWidth, cam.pixelHeight)
            r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
            out.append(rt)
        return out

    def Synchronize(self) -> None:
        for r in self.lanes:
            r.ctx.Synchronize()

    def Dispose(self) -> None:
        for t in self._targets.values():
            t.Dispose()
        self._targets = {}
        for r in self.lanes[1:]:
            r.DisposeResourcesForAsset()
        self.lanes = self.lanes[:1]


class GaussianSplatRenderSystem:
    """GaussianSplatRenderSystem (GaussianSplatRenderer.cs:17-212): per-camera gather, order, sort, draw, composite."""
    instance: "GaussianSplatRenderSystem" = None  # type: ignore

    def __init__(self):
        self.m_Splats: List[GaussianSplatRenderer] = []
        self.m_ActiveSplats: List[GaussianSplatRenderer] = []
        # A frame whose (tile, splat) pairs overflow the pair buffer drops its farthest pairs; the library notices (and grows
        # the buffer) within the pipeline depth, but THAT frame is truncated.  With strictPairs OnPreCullCamera reads the frame
        # statistics (BLOCKING: it serialises host and GPU) and renders the frame again after an overflow, so what it returns is
        # always complete.  Off by default: a render loop keeps the GPU queue full and a scene's first frames grow the buffer.
        self.strictPairs = False
        # Without strictPairs a truncated frame is still SIGNALLED: after the draws OnPreCullCamera polls (without blocking) what the
        # most recent draws that reached the GPU reported; True = some renderer's latest report exceeds its pair capacity, i.e. a frame
        # of the last few was drawn without its farthest pairs (the library grows the buffer at the next draw).
        self.lastFrameTruncated = False

    def RegisterSplat(self, r: GaussianSplatRenderer) -> None:      # :25-36
        if r not in self.m_Splats:
            self.m_Splats.append(r)

    def UnregisterSplat(self, r: GaussianSplatRenderer) -> None:    # :38-70
        if r in self.m_Splats:
            self.m_Splats.remove(r)

    def GatherSplatsForCamera(self, cam: Camera) -> bool:           # :73-105
        self.m_ActiveSplats = [gs for gs in self.m_Splats if gs.HasValidAsset and gs.HasValidRenderSetup]
        if not self.m_ActiveSplats:
            return False
        w2c = cam.worldToCameraMatrix.astype(np.float64)

        def cam_z(gs):                                              # camTr.InverseTransformPoint(pos).z (Unity: +z forward)
            p = np.append(np.asarray(gs.transform.position, np.float64), 1.0)
            return -float((w2c @ p)[2])
        # orderB.CompareTo(orderA), then posA.z.CompareTo(posB.z): stable sort on (-order, z)
        self.m_ActiveSplats.sort(key=lambda gs: (-gs.m_RenderOrder, cam_z(gs)))
        return True

    def SortAndRenderSplats(self, cam: Camera, rt: RenderTarget) -> None:     # :108-169
        for gs in self.m_ActiveSplats:
            if gs.m_FrameCounter % gs.m_SortNthFrame == 0:
                gs.SortPoints(cam, gs.transform.localToWorldMatrix)
            gs.m_FrameCounter += 1
            gs.CalcViewData(cam)
            gs.Draw(cam, rt)

    def OnPreCullCamera(self, cam: Camera, rt: RenderTarget, background=None):     # :187-211
        """Clear the splat RT, sort/calc/draw every active renderer, then (optionally) composite onto `background`."""
        if not self.GatherSplatsForCamera(cam):
            return None
        rt.Clear()
        self.SortAndRenderSplats(cam, rt)
        self.lastFrameTruncated = False
        for gs in self.m_ActiveSplats:
            if gs.m_RenderMode == RenderMode.Splats:
                pairs, cap = gs.PollPairs()
                self.lastFrameTruncated |= pairs > cap
        if self.strictPairs:
            overflowed = False
            for gs in self.m_ActiveSplats:
                if gs.m_RenderMode != RenderMode.Splats:
                    continue
                try:
                    gs.FrameStats()
                except GsError as e:
                    if e.code != GS_ERR_PAIR_OVERFLOW:
                        raise
                    overflowed = True                         # the buffer has been grown by the call
            if overflowed:                                     # same frame again: the order is already sorted, only the draws repeat
                rt.Clear()
                for gs in self.m_ActiveSplats:
                    gs.CalcViewData(cam)
                    gs.Draw(cam, rt)
            self.lastFrameTruncated = False                    # what is returned is complete
        if background is not None:
            return rt.Resolve(background)
        return None


GaussianSplatRenderSystem.instance = GaussianSplatRenderSystem()


def MergeSplatObjects(target: GaussianSplatRenderer, others: Sequence[GaussianSplatRenderer]) -> None:
    """GaussianSplatRendererEditor.MergeSplatObjects (GaussianSplatRendererEditor.cs:213-235): `target` grows by the splats of every valid renderer
    of `others`, which are copied behind its own in their order, each through dst.worldToLocal x src.localToWorld.  (The C# then deactivates the
    merged objects; here the caller disposes or keeps them.)"""
    valid = [gs for gs in others if gs is not target and gs.HasValidAsset and gs.HasValidRenderSetup]
    totalSplats = target.splatCount + sum(gs.splatCount for gs in valid)
    if totalSplats > kMaxSplats:
        return
    copyDstOffset = target.splatCount
    target.EditSetSplatCount(totalSplats)
    for gs in valid:
        gs.EditCopySplatsInto(target, 0, copyDstOffset, gs.splatCount)
        copyDstOffset += gs.splatCount
    assert copyDstOffset == totalSplats, f"Merge count mismatch, {copyDstOffset} vs {totalSplats}"
