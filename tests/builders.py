"""Scenes, assets and constants that more than one suite uses (helper, not a test): the crafted assets, the cutout sets and their float64 decision
table, the seeded random case, the golden vectors, the asset comparison of the importer suites, and the transforms, cameras and bake targets of the
edit path.  Needs no GPU and no renderer state; what drives a renderer is in tests/gpu_rig.py."""
from __future__ import annotations

import dataclasses
import functools
import os

import numpy as np

import copy_model as CM
import edit_model as EM
import export_model as XM
from common import default_camera, small_asset
from unitygaussiansplatting_amd import _abi, asset as A, camera, creator, scenes
from unitygaussiansplatting_amd.cutout import GaussianCutout, Type
from unitygaussiansplatting_amd.renderer import SortMode

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
VF, CF, SF = A.VectorFormat, A.ColorFormat, A.SHFormat

# ---- the edit path: transforms, cameras, bake targets ---------------------------------------------------------------------------------------------
SRC_TR = camera.Transform(**XM.BAKE_TRANSFORM)                      # rotated, non-uniformly scaled, mirrored in x: the transform of the export's bake tests
DST_TR = camera.Transform(position=(-0.4, 0.1, 0.2), rotation=(0.5, -0.5, 0.5, 0.5), scale=(0.8, 1.25, 2.0))
CAMS = [default_camera(az=25.0), default_camera(az=110.0, elev=-20.0), default_camera(az=250.0, elev=35.0, radius=7.0)]
TOOL = camera.Transform(position=(0.2, -0.1, 0.3), rotation=(0.1, 0.2, 0.05, 0.9695), scale=(1.25, 0.75, -1.5))      # non-uniform and mirrored
CLUSTER4K = (VF.Norm11, VF.Norm6, CF.Norm8x4, SF.Cluster4k)           # VeryLow with a colour format the bake has
LOW = (VF.Norm11, VF.Norm6, CF.Norm8x4, SF.Cluster16k)


@functools.lru_cache(maxsize=None)
def decode_of(n: int, quality: str, seed: int = 5) -> np.ndarray:
    """one oracle decode per source asset, shared by the tests that use it and left unchanged"""
    dec = CM.decode(small_asset(n, seed, quality))
    dec.setflags(write=False)
    return dec


def params_of(transform) -> _abi.gs_copy_params:
    m, q, s = transform
    p = _abi.gs_copy_params()
    p.matrix[0:16] = [float(v) for v in np.asarray(m, f32).reshape(-1)]
    p.rotation[0:4] = [float(f32(v)) for v in q]
    p.scale[0:3] = [float(f32(v)) for v in s]
    return p


# ---- crafted assets -----------------------------------------------------------------------------------------------------------------------------
def fp32_point_asset(points):
    """All-fp32, chunk-less asset whose decode is the identity on positions."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    other = np.zeros((n, 4), np.uint32)
    other[:, 0] = (511 | (511 << 10) | (511 << 20) | (3 << 30))          # ~identity rotation, largest = w
    other[:, 1:4] = np.float32(0.05).view(np.uint32)
    col = np.zeros((A.CalcTextureSize(n)[0] * A.CalcTextureSize(n)[1], 4), np.float32)
    col[:, :] = (0.5, 0.5, 0.5, 1.0)
    return A.GaussianSplatAsset(splatCount=n, posFormat=A.VectorFormat.Float32, scaleFormat=A.VectorFormat.Float32,
                                shFormat=A.SHFormat.Float32, colorFormat=A.ColorFormat.Float32x4,
                                posData=pts.view(np.uint8).reshape(-1).copy(), otherData=other.view(np.uint8).reshape(-1).copy(),
                                colorData=col.view(np.uint8).reshape(-1).copy(), shData=np.zeros(n * 192, np.uint8))


def pos_only_asset(n, seed=5):
    """fp32 positions and scales, no chunks, but Norm11 SH: the position gate passes, the rotation gate does not"""
    a = EM.point_asset(n, seed)
    return dataclasses.replace(a, shFormat=A.SHFormat.Norm11, shData=np.zeros(n * 60, np.uint8))


def tie_heavy_asset(kind: str, n: int = 6000, seed: int = 3, quality: str = "VeryHigh"):
    """Positions arranged so that MANY splats share a sort key (VeryHigh: fp32, exact; Medium: the same geometry on Norm11 lattices per chunk)."""
    raw = scenes.make_splats(n, seed, 3.0)
    rng = np.random.default_rng(seed)
    pos = raw.pos.copy()
    if kind == "lattice":            # columns of equal (x, z): a yaw-only camera ties each column
        g = np.stack(np.meshgrid(np.arange(10), np.arange(30), np.arange(10), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        pos = ((g[rng.integers(0, len(g), n)] - np.array([4.5, 14.5, 4.5], np.float32)) * np.float32(0.25)).astype(np.float32)
    elif kind == "planes":           # two planes facing a camera on the z axis
        pos[:, 2] = np.where(rng.random(n) < 0.5, np.float32(-0.5), np.float32(0.75))
    elif kind == "duplicates":       # every position three times
        base = pos[: n // 3]
        pos = np.concatenate([base, base, base, pos[: n - 3 * (n // 3)]])[:n]
    elif kind == "colocated":        # 150 splats at each of 8 points (runs of > 64 equal keys that NO matrix separates), the rest random
        pts = pos[:8].copy()
        pos[: 8 * 150] = np.repeat(pts, 150, axis=0)[rng.permutation(8 * 150)]
    raw = creator.InputSplatData(pos.astype(np.float32), raw.dc0, raw.sh, raw.opacity, raw.scale, raw.rot)
    return creator.CreateAssetFromSplats(raw, quality, name=f"ties_{kind}_{quality}")


def cams_for(kind: str):
    z_axis = camera.Camera(position=(0.0, 0.0, 6.0), pixelWidth=320, pixelHeight=200)
    yaw = lambda deg: camera.Camera(position=scenes.orbit_eye(6.0, 0.0, deg), pixelWidth=320, pixelHeight=200)
    pitched = lambda deg: camera.Camera(position=scenes.orbit_eye(6.0, 25.0, deg), pixelWidth=320, pixelHeight=200)
    if kind == "lattice":
        return [pitched(10.0), yaw(20.0), yaw(20.0), pitched(40.0), yaw(20.0), yaw(33.0), pitched(10.0)]
    if kind == "planes":
        return [pitched(15.0), z_axis, z_axis, yaw(8.0), z_axis]
    return [default_camera(az=a) for a in (0.0, 5.0, 5.0, 10.0, 0.0, 15.0)]


# ---- cutouts ------------------------------------------------------------------------------------------------------------------------------------
CUTOUT_SETS = {
    "crop_box": [GaussianCutout(Type.Box, False, camera.Transform(position=(0.2, 0.0, -0.1), scale=(1.5, 1.0, 2.0)))],
    "hole_ellipsoid": [GaussianCutout(Type.Ellipsoid, True, camera.Transform(position=(0.5, 0.3, 0.0), rotation=(0.0, 0.3826834, 0.0, 0.9238795), scale=(1.2, 0.6, 0.9)))],
    "hole_then_crop": [GaussianCutout(Type.Ellipsoid, True, camera.Transform(scale=(0.8, 0.8, 0.8))),
                       None,
                       GaussianCutout(Type.Box, False, camera.Transform(scale=(2.0, 2.0, 2.0))),
                       GaussianCutout(Type.Box, False, camera.Transform(position=(3, 3, 3)), isActiveAndEnabled=False)],
    "crop_then_hole": [GaussianCutout(Type.Box, False, camera.Transform(scale=(2.0, 2.0, 2.0))),
                       GaussianCutout(Type.Ellipsoid, True, camera.Transform(scale=(0.8, 0.8, 0.8)))],
    "only_null": [None],
}


def _decoded_positions(orc):
    return orc.decode_all()[:, 0:3].astype(np.float64)


def _expected_cut(pos, cutouts, renderer_matrix):
    """IsSplatCut written independently in float64 numpy (decision table of SplatUtilities.compute:164-187)."""
    n = len(pos)
    decided = np.zeros(n, bool)
    result = np.zeros(n, bool)
    final = np.zeros(n, bool)
    for c in cutouts:
        if c is None or not c.isActiveAndEnabled:
            continue
        m = c.transform.worldToLocalMatrix.astype(np.float64) @ np.asarray(renderer_matrix, np.float64)
        q = pos @ m[:3, :3].T + m[:3, 3]
        inside = (q * q).sum(1) <= 1.0 if c.m_Type == Type.Ellipsoid else (np.abs(q) <= 1.0).all(1)
        take = inside & ~decided
        result[take] = c.m_Invert
        decided |= take
        if not c.m_Invert:
            final[~decided] = True
    return np.where(decided, result, final)


def _margin_ok(pos, cutouts, renderer_matrix, eps=1e-4):
    """Splats not within eps of any cutout surface (fp32 vs fp64 may legitimately disagree there)."""
    ok = np.ones(len(pos), bool)
    for c in cutouts:
        if c is None or not c.isActiveAndEnabled:
            continue
        m = c.transform.worldToLocalMatrix.astype(np.float64) @ np.asarray(renderer_matrix, np.float64)
        q = pos @ m[:3, :3].T + m[:3, 3]
        d = (q * q).sum(1) - 1.0 if c.m_Type == Type.Ellipsoid else np.abs(q).max(1) - 1.0
        ok &= np.abs(d) > eps
    return ok


# ---- the importer suites: two assets, byte for byte -----------------------------------------------------------------------------------------------
BLOBS = ("posData", "otherData", "colorData", "shData", "chunkData")


def _same(a, b):
    for nm in BLOBS:
        x, y = getattr(a, nm), getattr(b, nm)
        if x is None or y is None or len(x) == 0 or len(y) == 0:
            assert (x is None or len(x) == 0) and (y is None or len(y) == 0), nm
            continue
        x, y = np.asarray(x, np.uint8), np.asarray(y, np.uint8)
        assert len(x) == len(y), (nm, len(x), len(y))
        bad = np.flatnonzero(x != y)
        assert len(bad) == 0, f"{nm}: {len(bad)} bytes differ, first at {bad[:5]}"
    assert np.array_equal(np.asarray(a.boundsMin, np.float32), np.asarray(b.boundsMin, np.float32)), ("boundsMin", a.boundsMin, b.boundsMin)
    assert np.array_equal(np.asarray(a.boundsMax, np.float32), np.asarray(b.boundsMax, np.float32)), ("boundsMax", a.boundsMax, b.boundsMax)
    assert a.dataHash == b.dataHash, ("dataHash", a.dataHash, b.dataHash)


# ---- the golden vectors ---------------------------------------------------------------------------------------------------------------------------
def load_golden(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    f = z["fmt"]
    a = A.GaussianSplatAsset(splatCount=int(z["n"]), posFormat=A.VectorFormat(int(f[0])), scaleFormat=A.VectorFormat(int(f[1])),
                             colorFormat=A.ColorFormat(int(f[2])), shFormat=A.SHFormat(int(f[3])), posData=z["posData"],
                             otherData=z["otherData"], colorData=z["colorData"], shData=z["shData"],
                             chunkData=z["chunkData"] if len(z["chunkData"]) else None, name=name)
    return z, a


# ---- the seeded random case of the parity walks -----------------------------------------------------------------------------------------------------
_SIZES = [(320, 200), (333, 217), (17, 9), (8, 8), (640, 360), (1280, 720), (48, 1024), (1024, 48), (1, 1), (31, 33)]


def _case(seed):
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([257, 1_000, 5_003, 20_011, 60_000]))
    quality = str(rng.choice(["VeryHigh", "High", "Medium", "Low", "VeryLow"]))
    if quality in ("Low", "VeryLow"):
        # Cluster16k / Cluster4k SH: the importer refuses fewer splats than table entries (the reference's creator skips the clustering there and writes a
        # blob its own shader cannot index: GaussianSplatAssetCreator.cs:481-483, 1046-1065), and the k-means is slow on the host beyond ~20 k splats
        n = 20_011 if quality == "Low" else min(max(n, 5_003), 20_011)
    extent = float(rng.choice([0.5, 3.0, 10.0]))
    W, H = _SIZES[int(rng.integers(len(_SIZES)))]
    kind = str(rng.choice(["orbit", "inside", "grazing", "far"], p=[0.5, 0.25, 0.15, 0.1]))
    radius = {"orbit": rng.uniform(1.5, 3.0) * extent, "inside": rng.uniform(0.05, 0.6) * extent, "grazing": rng.uniform(0.9, 1.1) * extent,
              "far": rng.uniform(20.0, 60.0) * extent}[kind]
    cam = camera.Camera(position=scenes.orbit_eye(float(radius), float(rng.uniform(-60, 60)), float(rng.uniform(0, 360))), pixelWidth=W, pixelHeight=H,
                        fieldOfView=float(rng.choice([10.0, 39.0965, 60.0, 110.0])))
    tr = None
    if rng.random() < 0.4:
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        sc = rng.uniform(0.5, 2.0, 3) * (np.array([-1.0, 1.0, 1.0]) if rng.random() < 0.3 else 1.0)      # (mirrored: the sample scene's transform is)
        tr = camera.Transform(position=tuple(rng.uniform(-0.5, 0.5, 3) * extent), rotation=tuple(q), scale=tuple(sc))
    fields = dict(m_SplatScale=float(rng.choice([1.0, 0.3, 2.0])), m_OpacityScale=float(rng.choice([1.0, 0.5, 1.7])), m_SHOrder=int(rng.integers(0, 4)),
                  m_SHOnly=bool(rng.random() < 0.15))
    mode = SortMode.Visible if rng.random() < 0.5 else SortMode.Full
    tile = [(0, 0), (16, 16), (32, 16), (32, 32)][int(rng.integers(4))]
    asset_seed = int(rng.integers(1, 50))
    # (drawn last, so that the cases above are the ones of the first campaign) cutouts, deleted bits, the fast blend mode
    cut = str(rng.choice(list(CUTOUT_SETS))) if rng.random() < 0.3 else None
    bits_seed = int(rng.integers(1, 1000)) if rng.random() < 0.25 else None
    blend = 1 if rng.random() < 0.2 else 0
    return dict(n=n, quality=quality, extent=extent, cam=cam, tr=tr, fields=fields, mode=mode, tile=tile, kind=kind, asset_seed=asset_seed, cut=cut,
                bits_seed=bits_seed, blend=blend)
