"""The yardstick of the merge (helper, not a test): a numpy restatement of CSCopySplats (SplatUtilities.compute:675-758), of the bookkeeping of
EditSetSplatCount / EditCopySplatsInto (GaussianSplatRenderer.cs:960-1075) and of the editor's MergeSplatObjects
(GaussianSplatRendererEditor.cs:213-235), written from the reference's text on top of parts the suite already has: the full decode ([N, 59],
Oracle.decode_all) and the bake of tests/export_model.py, the rotation codec of tests/transform_model.py, the Morton texel index and the texture
size of the importer (creator.SplatIndexToTextureIndex, asset.CalcTextureSize).

`Blobs` is what a VeryHigh, chunk-less renderer holds: pos 12 N bytes, other 16 N, the colour texture 2048 x CalcTextureSize(N).h texels of four
fp32, sh 192 N, and the deleted words (None: no buffer).  Two things of the kernel's text are kept literally: it bounds-checks srcIdx =
srcStart + idx and reads the deleted bit of srcIdx but loads splat idx (:697); and it has no IsSplatCut test."""
from __future__ import annotations

import dataclasses

import numpy as np

import export_model as XM
import oracle_lib as O
import transform_model as TM
from unitygaussiansplatting_amd import asset as A
from unitygaussiansplatting_amd import creator

f32 = np.float32
IDENTITY = (np.eye(4, dtype=f32), np.array([0, 0, 0, 1], f32), np.ones(3, f32))


def copy_records(dec, transform=None):
    """the transformed, re-encoded records of decoded splats ([M, 59]): pos [M, 3] f32, other [M, 4] u32, texel [M, 4] f32, sh [M, 45] f32"""
    dec = np.ascontiguousarray(dec, f32)
    m = len(dec)
    matrix, q, s = IDENTITY if transform is None else transform
    s = np.asarray(s, f32)
    pos, rot, scale, opacity, col = dec[:, 0:3], dec[:, 3:7].copy(), dec[:, 7:10], dec[:, 10], dec[:, 11:14]
    sh = dec[:, 14:59].reshape(m, 15, 3)
    with np.errstate(all="ignore"):
        pos = XM.mul_point(matrix, pos)                            # mul(_CopyTransformMatrix, float4(src.pos, 1)).xyz
        if s[0] < 0:
            rot[:, [1, 2]] = -rot[:, [1, 2]]
        if s[1] < 0:
            rot[:, [0, 2]] = -rot[:, [0, 2]]
        if s[2] < 0:
            rot[:, [0, 1]] = -rot[:, [0, 1]]
        rot = XM.quat_mul(np.asarray(q, f32), rot)
        scale = (scale * np.abs(s)).astype(f32)
        sh = XM.rotate_sh(sh, XM.sh_bands(matrix, f32), f32)
        other = np.zeros((m, 4), np.uint32)
        other[:, 0] = TM.encode_quat_norm10(TM.pack_smallest3(rot))
        other[:, 1:4] = np.ascontiguousarray(scale, f32).view(np.uint32)
        texel = np.concatenate([col, opacity[:, None]], axis=1).astype(f32)
    return np.ascontiguousarray(pos, f32), other, texel, np.ascontiguousarray(sh.reshape(m, 45), f32)


@dataclasses.dataclass
class Blobs:
    n: int
    pos: np.ndarray            # uint8
    other: np.ndarray
    color: np.ndarray
    sh: np.ndarray
    deleted: np.ndarray | None = None

    @property
    def words(self) -> int:
        return (self.n + 31) // 32

    def copy(self) -> "Blobs":
        return Blobs(self.n, self.pos.copy(), self.other.copy(), self.color.copy(), self.sh.copy(), None if self.deleted is None else self.deleted.copy())

    def deleted_words(self) -> np.ndarray:
        return np.zeros(self.words, np.uint32) if self.deleted is None else self.deleted

    def asset(self, name="merged") -> A.GaussianSplatAsset:
        """a host asset made of the four blobs (VeryHigh: all fp32, chunk-less)"""
        a = A.GaussianSplatAsset(splatCount=self.n, posFormat=A.VectorFormat.Float32, scaleFormat=A.VectorFormat.Float32, shFormat=A.SHFormat.Float32,
                                 colorFormat=A.ColorFormat.Float32x4, posData=self.pos.copy(), otherData=self.other.copy(), colorData=self.color.copy(),
                                 shData=self.sh.copy(), chunkData=None, name=name)
        a.dataHash = a.ComputeDataHash()
        return a


def zero_blobs(n: int) -> Blobs:
    """what EditSetSplatCount allocates: every byte zero"""
    w, h = A.CalcTextureSize(n)
    return Blobs(n, np.zeros(12 * n, np.uint8), np.zeros(16 * n, np.uint8), np.zeros(w * h * 16, np.uint8), np.zeros(192 * n, np.uint8), np.zeros((n + 31) // 32, np.uint32))


def is_very_high(asset) -> bool:
    return (asset.chunkCount == 0 and asset.posFormat == A.VectorFormat.Float32 and asset.scaleFormat == A.VectorFormat.Float32
            and asset.shFormat == A.SHFormat.Float32 and asset.colorFormat == A.ColorFormat.Float32x4)


def blobs_of(asset) -> Blobs:
    assert is_very_high(asset)
    n = asset.splatCount
    w, h = A.CalcTextureSize(n)
    u8 = lambda b, size: np.ascontiguousarray(b, np.uint8)[:size].copy()      # (the importer pads pos / other / sh by a dword: whole records only)
    return Blobs(n, u8(asset.posData, 12 * n), u8(asset.otherData, 16 * n), u8(asset.colorData, w * h * 16), u8(asset.shData, 192 * n), None)


def decode(source) -> np.ndarray:
    """LoadSplatData of every splat of an asset or of Blobs: [N, 59]"""
    return O.Oracle(source.asset() if isinstance(source, Blobs) else source).decode_all()


def copy_splats(src_dec, src_deleted, dst: Blobs, transform, src_start: int, dst_start: int, count: int) -> None:
    """CSCopySplats dispatched over `count` threads, into dst in place.  src_dec: the decode of the source ([srcN, 59]); src_deleted: its words or None."""
    src_n = len(src_dec)
    idx = np.arange(count, dtype=np.int64)
    src_idx, dst_idx = src_start + idx, dst_start + idx
    keep = (src_idx < src_n) & (dst_idx < dst.n)
    idx, src_idx, dst_idx = idx[keep], src_idx[keep], dst_idx[keep]
    if len(idx) == 0:
        return
    pos, other, texel, sh = copy_records(src_dec[idx], transform)  # LoadSplatData(idx): the thread index, not srcIdx
    dst.pos.view(f32).reshape(dst.n, 3)[dst_idx] = pos
    dst.other.view(np.uint32).reshape(dst.n, 4)[dst_idx] = other
    dst.color.view(f32).reshape(-1, 4)[creator.SplatIndexToTextureIndex(dst_idx.astype(np.uint32))] = texel
    dst.sh.view(f32).reshape(dst.n, 48)[dst_idx, :45] = sh         # the 12 bytes behind the coefficients are not written
    if src_deleted is not None:
        if dst.deleted is None:
            dst.deleted = np.zeros(dst.words, np.uint32)           # a destination without a deleted buffer gets a zeroed one
        w = np.asarray(src_deleted, np.uint32)
        bit = ((w[src_idx >> 5] >> (src_idx & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
        np.bitwise_or.at(dst.deleted, dst_idx[bit] >> 5, np.uint32(1) << (dst_idx[bit] & 31).astype(np.uint32))      # InterlockedOr: never cleared


def set_splat_count(src_dec, src_deleted, new_n: int, transform=None) -> Blobs:
    """EditSetSplatCount: zero-filled buffers of new_n splats, the old splats copied into them (srcStart = dstStart = 0, count = old N)"""
    dst = zero_blobs(new_n)
    copy_splats(src_dec, src_deleted, dst, transform, 0, 0, len(src_dec))
    return dst


def decompose(m):
    """(rotation xyzw, scale) of a 4x4 matrix as camera.matrix_rotation_scale hands them out"""
    from unitygaussiansplatting_amd import camera
    return camera.matrix_rotation_scale(m)


def copy_transform(src_tr, dst_tr):
    """EditCopySplats (:1052-1054): copyMatrix = dst.worldToLocal x src.localToWorld in float32, its rotation and lossy scale"""
    from unitygaussiansplatting_amd import camera
    m = camera.mat_mul(dst_tr.worldToLocalMatrix, src_tr.localToWorldMatrix)
    q, s = decompose(m)
    return m, np.asarray(q, f32), np.asarray(s, f32)


def merge(target: Blobs, target_tr, others):
    """MergeSplatObjects: others = [(decode, deleted words or None, transform)]; returns the merged Blobs"""
    total = target.n + sum(len(d) for d, _, _ in others)
    out = set_splat_count(decode(target), target.deleted, total)
    offset = target.n
    for dec, deleted, tr in others:
        copy_splats(dec, deleted, out, copy_transform(tr, target_tr), 0, offset, len(dec))
        offset += len(dec)
    assert offset == total
    return out
