"""The yardstick of the rigid rotate / scale of the selection (helper, not a test): a numpy twin of gs::edit_rigid_rotate_of (csrc/gs_params.h) and of
the RIGID instantiations of the transform kernel (csrc/gs_edit.hip), on top of transform_model.TransformModel -- which supplies
the positions, the format gates and the rotation codec -- and export_model's SH rotation (the bands of CalcSHRot, RotateSH).

The per-call part follows the operation order gs_params.h writes down, step by step: the delta normalised in float64, R(delta) and
L = W2O3 . R . O2W3 in float64 (products and sums one at a time, two-then-one), L rounded to float32 once, the band matrices of L's row-normalised form,
and the quaternion of that form by the largest-diagonal method in float64 with strict comparisons, normalised and rounded to float32 once.
With dtype = float64 nothing is rounded to float32: the form tests/test_rigid_model.py holds to the physics.

`RigidModel` adds to TransformModel what the renderer adds: the current SH blob, its mouse-down copy, the setting.  With the setting off every call is
TransformModel's."""
from __future__ import annotations

import dataclasses

import numpy as np

import export_model as XM
import transform_model as TM
from unitygaussiansplatting_amd import asset as A

f32, f64 = np.float32, np.float64


class Refused(ValueError):
    """the arguments of a rigid call are refused (GS_ERR_INVALID_ARGUMENT)"""


# ---- the per-call part ------------------------------------------------------------------------------------------------------------------------
def _mat3(a, b):
    """entry (i, j) = (a[i][0] b[0][j] + a[i][1] b[1][j]) + a[i][2] b[2][j], in float64"""
    out = np.zeros((3, 3), f64)
    for i in range(3):
        for j in range(3):
            out[i, j] = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
    return out


def rotation_matrix(d):
    """R(d) of a unit quaternion x y z w, float64, every operation as gs_params.h writes it"""
    x, y, z, w = (f64(c) for c in d)
    two, one = f64(2.0), f64(1.0)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], f64)


def quat_of_matrix(M):
    """the quaternion (x y z w, float64, normalised) of a 3x3 matrix: largest-diagonal branch, strict comparisons"""
    M = np.asarray(M, f64)
    one, two, four = f64(1.0), f64(2.0), f64(4.0)
    with np.errstate(all="ignore"):
        t = (M[0, 0] + M[1, 1]) + M[2, 2]
        if t > 0.0:
            s = np.sqrt(t + one) * two
            w, x, y, z = s / four, (M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s
        elif M[0, 0] > M[1, 1] and M[0, 0] > M[2, 2]:
            s = np.sqrt(((one + M[0, 0]) - M[1, 1]) - M[2, 2]) * two
            w, x, y, z = (M[2, 1] - M[1, 2]) / s, s / four, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s
        elif M[1, 1] > M[2, 2]:
            s = np.sqrt(((one + M[1, 1]) - M[0, 0]) - M[2, 2]) * two
            w, x, y, z = (M[0, 2] - M[2, 0]) / s, (M[0, 1] + M[1, 0]) / s, s / four, (M[1, 2] + M[2, 1]) / s
        else:
            s = np.sqrt(((one + M[2, 2]) - M[0, 0]) - M[1, 1]) * two
            w, x, y, z = (M[1, 0] - M[0, 1]) / s, (M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, s / four
        n = np.sqrt(((x * x + y * y) + z * z) + w * w)
        return np.array([x / n, y / n, z / n, w / n], f64)


def quat_branch(M) -> int:
    """which of the four branches quat_of_matrix takes (0: trace, 1..3: the diagonal entry)"""
    M = np.asarray(M, f64)
    if (M[0, 0] + M[1, 1]) + M[2, 2] > 0.0:
        return 0
    if M[0, 0] > M[1, 1] and M[0, 0] > M[2, 2]:
        return 1
    return 2 if M[1, 1] > M[2, 2] else 3


@dataclasses.dataclass
class Rigid:
    L: np.ndarray              # [3, 3]: the linear part of the position map (dtype)
    q: np.ndarray              # [4] x y z w (dtype)
    bands: tuple               # (sh1 [3, 3], sh2 [5, 5], sh3 [7, 7]) (dtype)
    s: float = 1.0


def rigid_rotate_of(o2w, w2o, delta, dtype=f32) -> Rigid:
    """gs::edit_rigid_rotate_of.  o2w / w2o: 4x4 float32 matrices as the call receives them; delta: x y z w float32"""
    src = f32 if dtype is f32 else f64                              # (the float64 form takes its arguments unrounded)
    d = np.asarray(delta, src).astype(f64).reshape(4)
    with np.errstate(all="ignore"):
        n = np.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3])
        if not (n > 0.0) or not np.isfinite(n):
            raise Refused("rotate: the delta quaternion has a zero or non-finite norm")
        d = d / n
        Am = np.asarray(o2w, src).reshape(4, 4)[:3, :3].astype(f64)
        Bm = np.asarray(w2o, src).reshape(4, 4)[:3, :3].astype(f64)
        for r in range(3):
            len2 = (Am[r, 0] * Am[r, 0] + Am[r, 1] * Am[r, 1]) + Am[r, 2] * Am[r, 2]
            if not (len2 > 0.0) or not np.isfinite(len2):
                raise Refused("rotate: local_to_world has a zero or non-finite row")
        L = _mat3(Bm, _mat3(rotation_matrix(d), Am)).astype(dtype)
        L4 = np.zeros((4, 4), dtype)
        L4[:3, :3] = L
        L4[3, 3] = 1
        bands = XM.sh_bands(L4, dtype)
        M = XM.sh_rot_matrix(L4, dtype).astype(f64)
        q = quat_of_matrix(M).astype(dtype)
    return Rigid(L, q, bands)


def shade_basis(d) -> np.ndarray:
    """the 15 weights ShadeSH (GaussianSplatting.hlsl:130-179) gives sh1..sh15 for unit directions d ([M, 3] -> [M, 15]), float64, its constants in
    closed form and its signs: what the physics of the float64 form is checked with"""
    pi = np.pi
    c1 = np.sqrt(3.0 / (4.0 * pi))
    c2 = [0.5 * np.sqrt(15.0 / pi), -0.5 * np.sqrt(15.0 / pi), 0.25 * np.sqrt(5.0 / pi), -0.5 * np.sqrt(15.0 / pi), 0.25 * np.sqrt(15.0 / pi)]
    c3 = [-0.25 * np.sqrt(35.0 / (2.0 * pi)), 0.5 * np.sqrt(105.0 / pi), -0.25 * np.sqrt(21.0 / (2.0 * pi)), 0.25 * np.sqrt(7.0 / pi),
          -0.25 * np.sqrt(21.0 / (2.0 * pi)), 0.25 * np.sqrt(105.0 / pi), -0.25 * np.sqrt(35.0 / (2.0 * pi))]
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([-c1 * y, c1 * z, -c1 * x,
                     c2[0] * xy, c2[1] * yz, c2[2] * (2 * zz - xx - yy), c2[3] * xz, c2[4] * (xx - yy),
                     c3[0] * y * (3 * xx - yy), c3[1] * xy * z, c3[2] * y * (4 * zz - xx - yy), c3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                     c3[4] * x * (4 * zz - xx - yy), c3[5] * z * (xx - yy), c3[6] * x * (xx - 3 * yy)], axis=1)


def is_uniform(scale) -> bool:
    v = np.asarray(scale, f32).reshape(3)
    return bool(v[0] == v[1] and v[1] == v[2])


# ---- the per-splat part -------------------------------------------------------------------------------------------------------------------------
def rotate_words(words, q):
    """decode, QuatMul(q_L, rot), pack, encode"""
    return TM.encode_quat_norm10(TM.pack_smallest3(TM.quat_mul(np.asarray(q, f32), TM.decode_rotation(words))))


def rotate_sh_records(rec, bands):
    """[M, 48] float32 SH records: the 45 coefficients through the bands, the last three floats as they were"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 48)
    out = rec.copy()
    out[:, :45] = XM.rotate_sh(rec[:, :45].reshape(-1, 15, 3), bands, f32).reshape(-1, 45)
    return out


def scale_scales(scales, s):
    with np.errstate(all="ignore"):
        return (np.asarray(scales, f32) * np.abs(f32(s))).astype(f32)


# ---- the renderer's state -----------------------------------------------------------------------------------------------------------------------
class RigidModel(TM.TransformModel):
    def __init__(self, asset, rigid: bool = False):
        super().__init__(asset)
        self.rigid = bool(rigid)
        self.sh_asset = np.array(asset.shData, np.uint8, copy=True)    # the asset's own bytes: what the renderer's blob is until it is made private
        self.sh_blob = self.sh_asset.copy()
        self.sh_md = None
        self.sh_stored = False
        self.sh_private = False                                    # the renderer has made its SH blob private

    def sh_rows(self, blob=None) -> np.ndarray:
        assert self.rot_gate
        return (self.sh_blob if blob is None else blob)[:self.n * 192].view(f32).reshape(self.n, 48)

    def scale_rows(self, blob=None) -> np.ndarray:
        assert self.rot_gate
        return (self.other_blob if blob is None else blob)[:self.n * 16].view(f32).reshape(self.n, 4)[:, 1:4]

    def current_asset(self):
        return dataclasses.replace(super().current_asset(), shData=self.sh_blob.copy())

    def blobs3(self):
        return self.pos_blob, self.other_blob, self.sh_blob

    def set_rigid(self, on: bool) -> None:
        self.rigid = bool(on)

    def store_sh(self) -> None:                                    # gs_renderer_edit_store_sh_mouse_down
        self.sh_stored = True
        if self.rot_gate:
            self.sh_md = self.sh_blob.copy()

    def rotate(self, center, l2w, w2l, rot) -> bool:
        if not self.rigid:
            return super().rotate(center, l2w, w2l, rot)
        self._ensure()
        if not (self.pos_stored and self.other_stored and self.sh_stored):
            return False
        try:
            G = rigid_rotate_of(l2w, w2l, rot)
        except Refused:
            return False
        m = self.selected()
        if self.pos_gate:
            self.pos_rows()[m] = TM.rotate_pos(self.pos_rows(self.pos_md)[m], center, l2w, w2l, rot)
        if self.rot_gate:
            self.rot_words()[m] = rotate_words(self.rot_words(self.other_md)[m], G.q)
            self.sh_rows()[m] = rotate_sh_records(self.sh_rows(self.sh_md)[m], G.bands)
            self.sh_private = True
        if self.pos_gate or self.rot_gate:
            self._moved()
        return True

    def scale(self, center, l2w, w2l, scale) -> bool:
        if not self.rigid or not is_uniform(scale):
            return super().scale(center, l2w, w2l, scale)
        self._ensure()
        if not (self.pos_stored and self.other_stored):
            return False
        m = self.selected()
        if self.pos_gate:
            self.pos_rows()[m] = TM.scale_pos(self.pos_rows(self.pos_md)[m], center, l2w, w2l, scale)
        if self.rot_gate:
            self.scale_rows()[m] = scale_scales(self.scale_rows(self.other_md)[m], np.asarray(scale, f32)[0])
        if self.pos_gate or self.rot_gate:
            self._moved()
        return True

    def release(self) -> None:
        super().release()
        self.sh_md = None
        self.sh_stored = False


def very_high(asset) -> bool:
    return (asset.chunkData is None or len(asset.chunkData) == 0) and asset.scaleFormat == A.VectorFormat.Float32 and asset.shFormat == A.SHFormat.Float32
