"""The yardstick of the edit kernels (helper, not a test): a numpy restatement of CSInitEditData, CSUpdateEditData, CSClearBuffer,
CSInvertSelection, CSSelectAll, CSOrBuffers and CSSelectionUpdate (SplatUtilities.compute:266-423), written from the reference's text,
over data from the CPU oracle:

  positions            Oracle.decode_all()[:, :3]                                   (LoadSplatPos)
  raw clip positions   Oracle.calc_view(P)['pos'] without cutouts                   (mul(UNITY_MATRIX_VP, mul(_MatrixObjectToWorld, pos)))
  cut flags            Oracle.calc_view with the cutouts and a frame whose matrix_vp is the identity: row 3 = 0 0 0 1, so w = 1 for a splat
                       that is kept (NaN for a NaN position that is kept) and w = 0 exactly for a splat IsSplatCut cuts

Pixel positions are the reference's expression evaluated in float32, operation by operation:
  px = ((x / w) * 0.5 + 0.5) * W,  py = (((-y) / w) * -0.5 + 0.5) * H
and the rectangle test is its four comparisons, so a NaN pixel position is a hit.

`EditModel` holds the three bit buffers the way the renderer does (None = the buffer does not exist and reads as zeros) and states what every
gs_renderer_edit_* call leaves in them.  Two quirks of the reference are the model's too: select-all / invert set the bits of the last word
beyond N and the counts include them; bounds of nothing are +1e38 / -1e38."""
from __future__ import annotations

import numpy as np

import oracle_lib as O
from unitygaussiansplatting_amd import camera
from unitygaussiansplatting_amd._abi import gs_frame_params
from unitygaussiansplatting_amd.cutout import GaussianCutout, Type, shader_data_array

f32 = np.float32


# ---- FloatToSortableUint (SplatUtilities.compute:52-57) / SortableUintToFloat (GaussianSplatRenderer.cs:699-703) ---------------------
def float_to_sortable_uint(f) -> np.ndarray:
    fu = np.ascontiguousarray(f, np.float32).view(np.uint32)
    mask = (np.uint32(0) - (fu >> np.uint32(31))) | np.uint32(0x80000000)
    return fu ^ mask


def sortable_uint_to_float(v) -> np.ndarray:
    v = np.ascontiguousarray(v, np.uint32)
    mask = ((v >> np.uint32(31)) - np.uint32(1)) | np.uint32(0x80000000)
    return (v ^ mask).view(np.float32)


INIT_MIN = int(float_to_sortable_uint(np.array([1.0e38], f32))[0])
INIT_MAX = int(float_to_sortable_uint(np.array([-1.0e38], f32))[0])


def pack_bits(flags: np.ndarray, n_words: int) -> np.ndarray:
    """bool per splat -> ceil(N/32) words, bit i & 31 of word i >> 5"""
    m = np.zeros(n_words * 32, np.uint8)
    m[:len(flags)] = np.asarray(flags, bool)
    return np.packbits(m, bitorder="little").view(np.uint32).copy()


def unpack_bits(words: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


def popcount(words: np.ndarray) -> int:
    return int(np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8)).sum())


def identity_vp_params() -> gs_frame_params:
    """A frame whose matrix_vp (and every other matrix) is the identity: clip.w = 1 for every splat calc_view keeps."""
    p = gs_frame_params()
    eye = [float(v) for v in np.eye(4, dtype=f32).reshape(-1)]
    for m in (p.matrix_mv, p.matrix_object_to_world, p.matrix_world_to_object, p.matrix_vp):
        m[0:16] = eye
    p.proj_m00 = p.proj_m11 = 1.0
    p.screen_w, p.screen_h = 64.0, 64.0
    p.splat_scale = p.opacity_scale = 1.0
    p.sh_order, p.sh_only = 0, 0
    p.near_clip, p.far_clip = 0.3, 1000.0
    return p


def pixel_positions(clip: np.ndarray, W: float, H: float):
    """float32, one rounding per operation, in the reference's order (SplatUtilities.compute:404-411)"""
    x, y, w = clip[:, 0].astype(f32), clip[:, 1].astype(f32), clip[:, 3].astype(f32)
    with np.errstate(all="ignore"):
        px = ((x / w) * f32(0.5) + f32(0.5)) * f32(W)
        py = (((-y) / w) * f32(-0.5) + f32(0.5)) * f32(H)
    return px.astype(f32), py.astype(f32)


def hit_flags(clip: np.ndarray, cut: np.ndarray, W: float, H: float, rect) -> np.ndarray:
    """CSSelectionUpdate's early-outs (:400-416), literally"""
    r = np.asarray(rect, f32)
    w = clip[:, 3].astype(f32)
    px, py = pixel_positions(clip, W, H)
    with np.errstate(invalid="ignore"):
        behind = w <= f32(0.0)                                   # a NaN w is not "behind"
        outside = (px < r[0]) | (px > r[2]) | (py < r[1]) | (py > r[3])      # a NaN pixel position is outside no edge
    return ~np.asarray(cut, bool) & ~behind & ~outside


def splat_bounds(pos: np.ndarray):
    """per splat and component: FloatToSortableUint(min(1e38, p)), FloatToSortableUint(max(-1e38, p)) -- min / max drop a NaN"""
    p = np.ascontiguousarray(pos, f32)
    lo = np.fmin(f32(1.0e38), p).astype(f32)
    hi = np.fmax(f32(-1.0e38), p).astype(f32)
    return float_to_sortable_uint(lo).reshape(p.shape), float_to_sortable_uint(hi).reshape(p.shape)


class EditModel:
    def __init__(self, asset):
        self.asset = asset
        self.orc = O.Oracle(asset)
        self.n = asset.splatCount
        self.nw = (self.n + 31) // 32
        self.pos = self.orc.decode_all()[:, :3].astype(f32).copy()
        self.lo, self.hi = splat_bounds(self.pos)
        self.cut = np.zeros(self.n, bool)
        self.cutouts, self.cutout_count = None, 0
        self.sel = self.md = self.deleted = None                  # None: the buffer does not exist
        self._clip_key, self._clip = None, None

    # -- inputs ---------------------------------------------------------------------------------------------------------------------------
    def set_cutouts(self, cutouts, renderer_matrix) -> None:
        """cutouts: a list of GaussianCutout / None, as GaussianSplatRenderer.m_Cutouts"""
        self.cutouts, self.cutout_count = shader_data_array(cutouts, renderer_matrix)
        if self.cutout_count == 0:
            self.cut = np.zeros(self.n, bool)
            return
        v = self.orc.calc_view(identity_vp_params(), self.cutouts, self.cutout_count)
        self.cut = (v["pos"][:, 3] == 0.0).copy()

    def clip_positions(self, P: gs_frame_params) -> np.ndarray:
        key = bytes(P)
        if self._clip_key != key:
            self._clip_key, self._clip = key, self.orc.calc_view(P)["pos"].copy()
        return self._clip

    def hits(self, P: gs_frame_params, rect) -> np.ndarray:
        return hit_flags(self.clip_positions(P), self.cut, P.screen_w, P.screen_h, rect)

    def _cut_words(self) -> np.ndarray:
        return pack_bits(self.cut, self.nw)

    def _ensure(self) -> None:                                    # EnsureEditingBuffers
        if self.sel is None:
            self.sel, self.md = np.zeros(self.nw, np.uint32), np.zeros(self.nw, np.uint32)

    # -- the calls --------------------------------------------------------------------------------------------------------------------------
    def select_all(self) -> None:                                 # CSSelectAll: v = ~0, minus the cut splats below N
        self._ensure()
        self.sel = ~np.zeros(self.nw, np.uint32) & ~self._cut_words()

    def invert_selection(self) -> None:                           # CSInvertSelection
        self._ensure()
        self.sel = ~self.sel & ~self._cut_words()

    def deselect_all(self) -> None:                               # CSClearBuffer
        self._ensure()
        self.sel = np.zeros(self.nw, np.uint32)

    def store_selection(self) -> None:                            # Graphics.CopyBuffer(selected -> mouse-down)
        self._ensure()
        self.md = self.sel.copy()

    def update_selection(self, P: gs_frame_params, rect, subtract: bool) -> None:      # CopyBuffer(mouse-down -> selected) + CSSelectionUpdate
        self._ensure()
        hw = pack_bits(self.hits(P, rect), self.nw)
        self.sel = (self.md & ~hw) if subtract else (self.md | hw)

    def delete_selected(self) -> None:                            # CSOrBuffers + CSClearBuffer
        self._ensure()
        self.deleted = (self.deleted if self.deleted is not None else np.zeros(self.nw, np.uint32)) | self.sel
        self.sel = np.zeros(self.nw, np.uint32)

    def upload_selected(self, words) -> None:
        self._ensure()
        self.sel = np.ascontiguousarray(words, np.uint32).copy()

    def set_deleted_bits(self, words) -> None:                    # gs_renderer_set_deleted_bits: overwrite, None frees
        self.deleted = None if words is None else np.ascontiguousarray(words, np.uint32).copy()

    def release(self) -> None:
        self.sel = self.md = None

    # -- what can be read back ---------------------------------------------------------------------------------------------------------
    def bits(self):
        z = np.zeros(self.nw, np.uint32)
        return tuple(z if b is None else b for b in (self.sel, self.md, self.deleted))

    def info(self):
        """(selected, deleted, cut, min x y z, max x y z): counts, then the bounds as float32 BIT PATTERNS (uint32); all zeros without edit buffers"""
        if self.sel is None:
            return np.zeros(9, np.uint32)
        val_del = self.deleted if self.deleted is not None else np.zeros(self.nw, np.uint32)
        cutw = self._cut_words()
        val_sel = self.sel & ~val_del & ~cutw
        val_cut = cutw & ~val_del
        m = unpack_bits(val_sel, self.n)                          # the position loop stops at N
        lo = self.lo[m].min(axis=0, initial=INIT_MIN) if m.any() else np.full(3, INIT_MIN, np.uint32)
        hi = self.hi[m].max(axis=0, initial=INIT_MAX) if m.any() else np.full(3, INIT_MAX, np.uint32)
        out = np.zeros(9, np.uint32)
        out[0:3] = popcount(val_sel), popcount(val_del), popcount(val_cut)
        out[3:6] = sortable_uint_to_float(lo.astype(np.uint32)).view(np.uint32)
        out[6:9] = sortable_uint_to_float(hi.astype(np.uint32)).view(np.uint32)
        return out


# ---- shared cases --------------------------------------------------------------------------------------------------------------------------
PREMISE_RECT = (80.25, 50.5, 200.75, 150.0)


def inside_camera() -> camera.Camera:
    """a camera INSIDE the scene: about half the splats are behind it"""
    return camera.Camera(position=(0.3, 0.2, 0.1), target=(1.0, 0.0, 0.5), fieldOfView=60.0, pixelWidth=320, pixelHeight=200)


def cutout_lists():
    T = camera.Transform
    ell = GaussianCutout(Type.Ellipsoid, False, T(position=(0.4, -0.2, 0.3), scale=(2.2, 1.6, 2.0)))
    box_inv = GaussianCutout(Type.Box, True, T(position=(-0.8, 0.3, 0.2), rotation=(0.0, 0.259, 0.0, 0.966), scale=(1.2, 1.5, 1.0)))
    ell2 = GaussianCutout(Type.Ellipsoid, False, T(position=(-0.5, 0.5, -0.4), scale=(1.5, 2.0, 1.5)))
    # (IsSplatCut walks the list in order and the first volume a splat is inside decides; an inverted box BEHIND an ellipsoid would decide nothing --
    # outside the ellipsoid the splat is cut either way -- so the box comes first: cut = inside the box, or outside the ellipsoid)
    return {"none": None, "ellipsoid": [ell], "ellipsoid+inverted box": [box_inv, ell], "null between": [ell, None, ell2]}


def point_asset(n: int, seed: int = 3, nan_at=None):
    """n seeded random positions in [-2, 2)^3 as an all-fp32, chunk-less asset (tests/crafted.asset); nan_at: that splat's x and z are NaN"""
    import crafted
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) * 4.0 - 2.0).astype(f32)
    if nan_at is not None:
        pos[nan_at] = (np.nan, 0.5, np.nan)
    return crafted.asset(pos, np.full((n, 3), 0.02, f32))


def info_words(info) -> np.ndarray:
    """a gs_edit_info as the model's nine words"""
    return np.frombuffer(bytes(info), np.uint32).copy()
