"""The model of a frame with the selection highlight (RenderGaussianSplats.shader:63-73,87-101): tests/highlight_host_harness.cpp bound with ctypes.

Geometry of a selected splat is the oracle's, unchanged: gso_raster_records on a copy of the view whose selected, in-front splats have the alpha half
0x3C00 (1.0) -- exactly the opacity-1 centre, axes and rectangle.  The harness walks the depth order over those records with the selected fragment added and
blends like gso_blend_f16 (mode 0) or in fp32 (mode 1).  Test infrastructure only."""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_lib as O
from common import _p
from harness import build_harness

SELECTED_ALPHA_HALF = 0xBC00           # -1.0: the mark calc_view leaves in a selected splat's raster record


def build(tmpdir) -> C.CDLL:
    L = C.CDLL(build_harness(tmpdir, "highlight_host_harness.cpp"))
    L.hl_half_of.restype = C.c_uint16
    L.hl_half_of.argtypes = [C.c_double]
    L.hl_native_e.restype = C.c_float
    L.hl_fragment_from.argtypes = [C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int32]
    return L


def bits_of(mask: np.ndarray) -> np.ndarray:
    """bool per splat -> ceil(N/32) uint32 words"""
    n = len(mask)
    b = np.zeros(((n + 31) // 32) * 32, np.uint8)
    b[:n] = mask
    return np.packbits(b.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()


def mask_of(bits: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(bits, np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


class Frame:
    """What a highlighted frame must be: the raster records calc_view leaves (recs with the -1 mark, rects, vis) and the picture."""

    def __init__(self, L, view: np.ndarray, P, sel_bits, order: np.ndarray):
        self.L, self.P, self.n = L, P, len(view)
        self.order = np.ascontiguousarray(order, np.uint32)
        sel = mask_of(sel_bits, self.n) if sel_bits is not None else np.zeros(self.n, bool)
        self.selected = sel & (view["pos"][:, 3] > 0)                   # vert(): only a splat that is not behind the camera is marked
        v1 = view.copy()
        v1["color"][self.selected, 1] = (v1["color"][self.selected, 1] & np.uint32(0xFFFF0000)) | np.uint32(0x3C00)
        self.recs = np.zeros((self.n, 8), np.uint32)
        self.rects = np.zeros((self.n, 2), np.uint32)
        self.vis = np.zeros((self.n + 63) // 64, np.uint64)
        O.lib().gso_raster_records(_p(v1), C.c_uint32(self.n), C.byref(P), _p(self.recs), _p(self.rects), _p(self.vis))
        self.visible = np.unpackbits(self.vis.view(np.uint8), bitorder="little")[:self.n].astype(bool)
        # the records the library must hold: the oracle's opacity-1 records with the alpha half -1
        self.want_recs = self.recs.copy()
        m = self.selected & self.visible
        self.want_recs[m, 7] = (self.want_recs[m, 7] & np.uint32(0xFFFF0000)) | np.uint32(SELECTED_ALPHA_HALF)
        self.depth = np.ascontiguousarray(view["pos"][:, 3], np.float32)

    def pairs(self, tile) -> int:
        """(tile, splat) pairs for a tile shape (tile_w, tile_h) or a gs_frame_stats"""
        tw, th = (int(tile.tile_w), int(tile.tile_h)) if hasattr(tile, "tile_w") else (int(tile[0]), int(tile[1]))
        wl, hl = tw.bit_length() - 1, th.bit_length() - 1
        r = self.rects[self.visible].astype(np.int64)
        x0, y0, x1, y1 = r[:, 0] & 0xFFFF, r[:, 0] >> 16, (r[:, 1] & 0xFFFF) - 1, (r[:, 1] >> 16) - 1
        return int((((x1 >> wl) - (x0 >> wl) + 1) * ((y1 >> hl) - (y0 >> hl) + 1)).sum())

    def draw(self, mode: int = 0, scene_depth=None, rt=None, classify: bool = False, tol: float = 1e-5):
        W, H = int(self.P.screen_w), int(self.P.screen_h)
        if rt is None:
            rt = np.zeros((H, W, 4), np.uint16)
        sd = np.ascontiguousarray(scene_depth, np.float32) if scene_depth is not None else None
        self.excused = np.zeros((H, W), np.uint8) if classify else None
        counts = np.zeros(6, np.uint64)
        sel8 = np.ascontiguousarray(self.selected, np.uint8)
        self.L.hl_draw(_p(self.recs), _p(self.rects), _p(self.vis), _p(self.depth), _p(sel8), _p(self.order), C.c_uint32(self.n), C.c_uint32(W), C.c_uint32(H),
                       C.c_int32(mode), _p(rt), _p(sd), _p(self.excused), C.c_double(tol), _p(counts) if classify else None)
        self.counts = dict(zip(("selected", "ring", "low", "unselected", "excused", "band_flips"), (int(c) for c in counts)))
        return rt


def host_records(L, view: np.ndarray, P, sel_bits):
    """calc_view's raster records as the HOST BUILD of the kernels' header computes them (gsm::PrepareSplatHighlight / RecordColor1)"""
    n = len(view)
    recs, rects, vis = np.zeros((n, 8), np.uint32), np.zeros((n, 2), np.uint32), np.zeros((n + 63) // 64, np.uint64)
    sb = np.ascontiguousarray(sel_bits, np.uint32) if sel_bits is not None else None
    L.hl_raster_records(_p(np.ascontiguousarray(view)), C.c_uint32(n), C.byref(P), _p(sb), _p(recs), _p(rects), _p(vis))
    return recs, rects, vis


def fragment(L, q, rgb, windowed: bool):
    out = np.zeros(4, np.float32)
    d = L.hl_fragment(_p(np.asarray(q, np.float32)), _p(np.asarray(rgb, np.float32)), _p(out), C.c_int32(int(windowed)))
    return int(d), out


def native_e(L, q):
    y = C.c_float()
    e = L.hl_native_e(_p(np.asarray(q, np.float32)), C.byref(y))
    return np.float32(e), np.float32(y.value)


def fragment_from(L, e_native, y, rgb, windowed: bool):
    """the selected fragment from a given native e (e.g. the canon's moved by an ulp, as a GPU's exp2 unit may return it)"""
    out = np.zeros(4, np.float32)
    d = L.hl_fragment_from(float(e_native), float(y), _p(np.asarray(rgb, np.float32)), _p(out), int(windowed))
    return int(d), out
