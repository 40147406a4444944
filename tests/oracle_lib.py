"""ctypes binding of oracle/libgs_oracle.so -- the CPU restatement used ONLY as the checker in tests,
smoke() and bench.py's cpu_baseline leg (never by the product path)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from common import _p
from unitygaussiansplatting_amd._abi import VIEW_DTYPE, gs_asset_desc, gs_frame_params, make_asset_desc

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "oracle", "libgs_oracle.so")


def build(force: bool = False) -> str:
    src = os.path.join(_ROOT, "oracle", "gs_oracle.cpp")
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", os.path.join(_ROOT, "oracle"), "-B" if force else "-s"], stdout=subprocess.DEVNULL)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.gso_f16tof32.restype = C.c_float
        _lib.gso_f16tof32.argtypes = [C.c_uint16]
        _lib.gso_f32tof16.restype = C.c_uint16
        _lib.gso_f32tof16.argtypes = [C.c_float]
        _lib.gso_f64tof16.restype = C.c_uint16
        _lib.gso_f64tof16.argtypes = [C.c_double]
        _lib.gso_blend_f16.restype = C.c_float
        _lib.gso_blend_f16.argtypes = [C.c_float, C.c_float, C.c_float]
        _lib.gso_num_threads.restype = C.c_int32
    return _lib


# The compositor tile the (tile, splat) pair count refers to is a performance parameter of the build under test (16x16, 32x16 or
# 32x32 pixels; frames do not depend on it): Oracle.tile_pairs counts 16x16 tiles unless Oracle.tile says otherwise; GPU tests compare
# the library's count with Oracle.pairs(P, frame_stats), the count for the shape the draw reported.
tile_shape_hook = None


class Oracle:
    """Holds an asset description and runs the reference-semantics stages on the CPU."""

    def __init__(self, asset):
        self.asset = asset
        self._keep = []
        self.desc = make_asset_desc(asset, self._keep)
        self.n = asset.splatCount
        self.order = np.arange(self.n, dtype=np.uint32)      # CSSetIndices
        self.keys = np.zeros(self.n, np.uint32)
        self.view = np.zeros(self.n, VIEW_DTYPE)
        self.tile = None                                     # (tile_w, tile_h) for tile_pairs; None = tile_shape_hook or 16x16

    def _set_tile(self, W: int, H: int):
        t = self.tile or (tile_shape_hook(W, H) if tile_shape_hook else (16, 16))
        lib().gso_set_tile_shape(C.c_int32(int(t[0])), C.c_int32(int(t[1])))
        return t

    def reset_order(self):
        lib().gso_set_indices(_p(self.order), C.c_uint32(self.n))

    def calc_distances(self, matrix_sort: np.ndarray):
        m = np.ascontiguousarray(matrix_sort, np.float32).reshape(16)
        lib().gso_calc_distances(C.byref(self.desc), _p(self.order), _p(m), _p(self.keys))
        return self.keys

    def sort(self, matrix_sort: np.ndarray):
        """SortPoints: distances through the current order, then the stable pair sort."""
        self.calc_distances(matrix_sort)
        lib().gso_sort_pairs(_p(self.keys), _p(self.order), C.c_uint32(self.n), C.c_uint32(32))
        return self.order

    def calc_view(self, params: gs_frame_params, cutouts=None, cutout_count: int = 0, deleted_bits: np.ndarray | None = None):
        """cutouts: a ctypes array of gs_cutout (cutout.shader_data_array); deleted_bits: ceil(n/32) uint32 words or None."""
        db = np.ascontiguousarray(deleted_bits, np.uint32) if deleted_bits is not None else None
        lib().gso_calc_view_ex(C.byref(self.desc), C.byref(params), cutouts if cutout_count else None, C.c_uint32(cutout_count),
                               _p(db) if db is not None else None, _p(self.view))
        return self.view

    def draw(self, params: gs_frame_params, mode: int = 0, rt: np.ndarray | None = None, window=None, scene_depth: np.ndarray | None = None):
        """window = (x0, y0, x1, y1) inclusive: only those pixels are composited (the rest of rt is left alone);
        scene_depth = H x W float32 view depths of the opaque scene (a fragment is kept iff the splat's clip.w <= depth)."""
        W, H = int(params.screen_w), int(params.screen_h)
        if rt is None:
            rt = np.zeros((H, W, 4), np.uint16)
        pairs = C.c_uint64(0)
        vis = C.c_uint32(0)
        win = (C.c_int32 * 4)(*[int(v) for v in window]) if window is not None else None
        sd = np.ascontiguousarray(scene_depth, np.float32) if scene_depth is not None else None
        self._set_tile(W, H)
        lib().gso_draw_ex(_p(self.view), _p(self.order), C.c_uint32(self.n), C.byref(params), C.c_int32(mode), _p(rt),
                          C.byref(pairs), C.byref(vis), win, _p(sd) if sd is not None else None)
        self.tile_pairs, self.visible = pairs.value, vis.value
        return rt

    def pairs(self, params: gs_frame_params, tile) -> int:
        """(tile, splat) pairs of the frame for a given compositor tile: `tile` = (tile_w, tile_h) or a gs_frame_stats (its tile_w / tile_h:
        the shape the draw under test used -- a performance parameter the library picks per target and scene).  Also sets self.visible."""
        t = (int(tile.tile_w), int(tile.tile_h)) if hasattr(tile, "tile_w") else (int(tile[0]), int(tile[1]))
        keep, self.tile = self.tile, t
        try:
            self.draw(params, 0, window=(0, 0, -1, -1))          # counts only
        finally:
            self.tile = keep
        return self.tile_pairs

    def draw_debug_points(self, params: gs_frame_params, display_index: bool, size: float, rt: np.ndarray | None = None, scene_depth=None):
        W, H = int(params.screen_w), int(params.screen_h)
        if rt is None:
            rt = np.zeros((H, W, 4), np.uint16)
        sd = np.ascontiguousarray(scene_depth, np.float32) if scene_depth is not None else None
        lib().gso_draw_debug_points(C.byref(self.desc), C.byref(params), C.c_int32(int(display_index)), C.c_float(size), _p(rt), _p(sd) if sd is not None else None)
        return rt

    def draw_debug_boxes(self, params: gs_frame_params, chunks: bool, mode: int = 0, rt: np.ndarray | None = None, scene_depth=None):
        """RenderMode.DebugBoxes (through self.order) / DebugChunkBounds; every pixel tests every box: small scenes only."""
        W, H = int(params.screen_w), int(params.screen_h)
        if rt is None:
            rt = np.zeros((H, W, 4), np.uint16)
        sd = np.ascontiguousarray(scene_depth, np.float32) if scene_depth is not None else None
        lib().gso_draw_debug_boxes(C.byref(self.desc), _p(self.order), C.byref(params), C.c_int32(int(chunks)), C.c_int32(mode), _p(rt),
                                   _p(sd) if sd is not None else None)
        return rt

    def raster_records(self, params: gs_frame_params):
        """prepare() of every splat: (recs N x 8 u32, rects N x 2 u32, vis ceil(N/64) u64), gs_renderer_download_raster_records' layout."""
        recs = np.zeros((self.n, 8), np.uint32)
        rects = np.zeros((self.n, 2), np.uint32)
        vis = np.zeros((self.n + 63) // 64, np.uint64)
        lib().gso_raster_records(_p(self.view), C.c_uint32(self.n), C.byref(params), _p(recs), _p(rects), _p(vis))
        return recs, rects, vis

    def decode_all(self) -> np.ndarray:
        out = np.zeros((self.n, 59), np.float32)
        lib().gso_decode_all(C.byref(self.desc), _p(out))
        return out


def sort_pairs(keys: np.ndarray, vals: np.ndarray, key_bits: int = 32):
    k = np.ascontiguousarray(keys, np.uint32).copy()
    v = np.ascontiguousarray(vals, np.uint32).copy()
    lib().gso_sort_pairs(_p(k), _p(v), C.c_uint32(len(k)), C.c_uint32(key_bits))
    return k, v


def stable_sort_reference(keys: np.ndarray, key_bits: int = 32) -> np.ndarray:
    k = np.ascontiguousarray(keys, np.uint32)
    perm = np.zeros(len(k), np.uint32)
    lib().gso_stable_sort_reference(_p(k), _p(perm), C.c_uint32(len(k)), C.c_uint32(key_bits))
    return perm


def resolve(rt: np.ndarray, bg=(0.0, 0.0, 0.0, 0.0)):
    H, W, _ = rt.shape
    out32 = np.zeros((H, W, 4), np.float32)
    out8 = np.zeros((H, W, 4), np.uint8)
    b = np.asarray(bg, np.float32)
    lib().gso_resolve(_p(np.ascontiguousarray(rt)), C.c_uint32(W), C.c_uint32(H), _p(b), _p(out32), _p(out8))
    return out32, out8


def f16_to_f32(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, np.uint16).view(np.float16).astype(np.float32)
