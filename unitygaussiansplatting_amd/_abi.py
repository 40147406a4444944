"""ctypes mirror of include/gsplat_c.h (structs + enums only; loading the library is in _lib.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

GS_OK = 0
GS_ERR_INVALID_ARGUMENT = -1
GS_ERR_HIP = -2
GS_ERR_UNSUPPORTED_FORMAT = -3
GS_ERR_OUT_OF_MEMORY = -4
GS_ERR_INVALID_ASSET = -5
GS_ERR_PAIR_OVERFLOW = -6
GS_ERR_SORT_TIMEOUT = -7
GS_ERR_NO_DEVICE = -8
GS_ERR_COMM = -9
GS_SORT_FULL = 0
GS_SORT_VISIBLE = 1


class gs_asset_desc(C.Structure):
    _fields_ = [
        ("splat_count", C.c_uint32), ("pos_format", C.c_uint32), ("scale_format", C.c_uint32),
        ("color_format", C.c_uint32), ("sh_format", C.c_uint32), ("memory_kind", C.c_uint32),
        ("pos_data", C.c_void_p), ("pos_size", C.c_uint64),
        ("other_data", C.c_void_p), ("other_size", C.c_uint64),
        ("color_data", C.c_void_p), ("color_size", C.c_uint64),
        ("sh_data", C.c_void_p), ("sh_size", C.c_uint64),
        ("chunk_data", C.c_void_p), ("chunk_size", C.c_uint64),
    ]


class gs_frame_params(C.Structure):
    _fields_ = [
        ("matrix_mv", C.c_float * 16), ("matrix_object_to_world", C.c_float * 16),
        ("matrix_world_to_object", C.c_float * 16), ("matrix_vp", C.c_float * 16),
        ("proj_m00", C.c_float), ("proj_m11", C.c_float),
        ("screen_w", C.c_float), ("screen_h", C.c_float),
        ("cam_pos_world", C.c_float * 3),
        ("splat_scale", C.c_float), ("opacity_scale", C.c_float),
        ("sh_order", C.c_uint32), ("sh_only", C.c_uint32),
        ("near_clip", C.c_float), ("far_clip", C.c_float),
    ]


class gs_cutout(C.Structure):
    _fields_ = [("matrix", C.c_float * 16), ("type_and_flags", C.c_uint32)]


class gs_edit_info(C.Structure):         # m_GpuEditCountsBounds decoded (gs_renderer_edit_info)
    _fields_ = [("selected", C.c_uint32), ("deleted", C.c_uint32), ("cut", C.c_uint32),
                ("bounds_min", C.c_float * 3), ("bounds_max", C.c_float * 3)]


class gs_pick_record(C.Structure):       # one pixel of a target's pick output (gs_target_set_pick_output): 16 bytes
    _fields_ = [("depth", C.c_float), ("splat", C.c_uint32), ("tag", C.c_uint32), ("zero", C.c_uint32)]


GS_PICK_NO_SPLAT = 0xFFFFFFFF


class gs_attribute_stats(C.Structure):   # gs_renderer_edit_attribute_stats: the scope's size, its NaN values, the non-NaN values of smallest / largest key
    _fields_ = [("members", C.c_uint32), ("nans", C.c_uint32), ("vmin", C.c_float), ("vmax", C.c_float)]


GS_SCOPE_ALIVE = 0
GS_SCOPE_SELECTED = 1
GS_ATTR_NOT_ALIVE = 0xFFFFFFFF           # the word gs_renderer_edit_attribute_values / _ranks write where there is no value
# gs_target_download_pick as a structured numpy array
PICK_DTYPE = [("depth", "<f4"), ("splat", "<u4"), ("tag", "<u4"), ("zero", "<u4")]

GS_EXPORT_RECORD_BYTES = 248


class gs_export_params(C.Structure):     # what CSExportData reads of its dispatch (gs_renderer_edit_export_*)
    _fields_ = [("matrix_object_to_world", C.c_float * 16), ("rotation", C.c_float * 4), ("scale", C.c_float * 3),
                ("bake_transform", C.c_uint32)]


GS_SPZ_FRACT_AUTO = 0xffffffff


class gs_spz_params(C.Structure):        # gs_renderer_edit_export_spz / _spz_body
    _fields_ = [("sh_level", C.c_uint32), ("fract_bits", C.c_uint32), ("compression_level", C.c_int32), ("slice_bytes", C.c_uint32)]


class gs_copy_params(C.Structure):       # what CSCopySplats reads of its dispatch (gs_renderer_edit_set_splat_count / _copy_splats_into)
    _fields_ = [("matrix", C.c_float * 16), ("rotation", C.c_float * 4), ("scale", C.c_float * 3)]


GS_HIST_SELECTION = 1
GS_HIST_DELETED = 2
GS_HIST_POS = 4
GS_HIST_OTHER = 8
GS_HIST_SH = 16
GS_HIST_TRANSFORM = 0x80000000


class gs_edit_history_info(C.Structure):     # gs_renderer_edit_history_info
    _fields_ = [("enabled", C.c_uint32), ("undo_depth", C.c_uint32), ("redo_depth", C.c_uint32), ("top_what", C.c_uint32),
                ("bytes", C.c_uint64), ("max_bytes", C.c_uint64), ("top_bytes", C.c_uint64), ("top_splats", C.c_uint32),
                ("evicted", C.c_uint32), ("uncovered_transforms", C.c_uint32)]


class gs_import_input(C.Structure):
    _fields_ = [("splat_count", C.c_uint32), ("pos", C.c_void_p), ("dc0", C.c_void_p), ("sh", C.c_void_p),
                ("opacity", C.c_void_p), ("scale", C.c_void_p), ("rot", C.c_void_p)]


class gs_import_formats(C.Structure):
    _fields_ = [("pos_format", C.c_uint32), ("scale_format", C.c_uint32), ("color_format", C.c_uint32), ("sh_format", C.c_uint32),
                ("linearize", C.c_uint32), ("morton", C.c_uint32)]


GS_SPLAT_FILE_PLY = 1
GS_SPLAT_FILE_SPZ = 2
# gs_splat_file_info.offsets by name: the 59 float properties the importer reads, then the normals
PLY_OFFSET_NAMES = (["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
                    + [f"f_rest_{k}" for k in range(45)] + ["nx", "ny", "nz"])


class gs_splat_file_info(C.Structure):   # what gs_splat_file_open found in the file
    _fields_ = [("kind", C.c_uint32), ("splat_count", C.c_uint32), ("stride", C.c_uint32), ("sh_level", C.c_uint32), ("fract_bits", C.c_uint32),
                ("reserved", C.c_uint32), ("body_bytes", C.c_uint64), ("offsets", C.c_int32 * 62)]


class gs_frame_stats(C.Structure):
    _fields_ = [("tile_pairs", C.c_uint64), ("pair_capacity", C.c_uint64), ("visible_splats", C.c_uint32),
                ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32), ("sort_error", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
                ("sort_mode", C.c_uint32), ("tie_long_runs", C.c_uint32), ("tie_longest_run", C.c_uint32)]


class gs_stage_times(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("calc_distances_ms", "sort_ms", "calc_view_ms", "bin_ms", "pair_sort_ms",
                                         "blend_ms", "resolve_ms", "total_ms")] + [("frames", C.c_uint32)] + \
               [("onesweep_depth_ms", C.c_float), ("onesweep_pairs_ms", C.c_float), ("onesweep_pair_launches", C.c_uint32),
                ("onesweep_depth_kernel_ms", C.c_float), ("onesweep_pairs_kernel_ms", C.c_float), ("onesweep_depth_launches", C.c_uint32)]


VIEW_DTYPE = np.dtype([("pos", "<f4", (4,)), ("axis1", "<f4", (2,)), ("axis2", "<f4", (2,)), ("color", "<u4", (2,))])
assert VIEW_DTYPE.itemsize == 40     # kGpuViewDataSize, GaussianSplatRenderer.cs:371


def make_asset_desc(asset, keepalive: list) -> gs_asset_desc:
    """Host-memory gs_asset_desc for a unitygaussiansplatting_amd.asset.GaussianSplatAsset.
    `keepalive` receives the contiguous arrays whose pointers the struct borrows."""
    d = gs_asset_desc()
    d.splat_count = asset.splatCount
    d.pos_format, d.scale_format = int(asset.posFormat), int(asset.scaleFormat)
    d.color_format, d.sh_format = int(asset.colorFormat), int(asset.shFormat)
    d.memory_kind = 0
    for nm, blob in (("pos", asset.posData), ("other", asset.otherData), ("color", asset.colorData),
                     ("sh", asset.shData), ("chunk", asset.chunkData)):
        if blob is None or len(blob) == 0:
            setattr(d, nm + "_data", None)
            setattr(d, nm + "_size", 0)
            continue
        arr = np.ascontiguousarray(blob, dtype=np.uint8)
        keepalive.append(arr)
        setattr(d, nm + "_data", arr.ctypes.data)
        setattr(d, nm + "_size", arr.nbytes)
    return d
