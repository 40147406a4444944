"""-m gpu: the per-frame calc_view kernels with a creator preset's formats compiled in (gs_view.hip) against the kernel that reads the formats at
run time, and both against the oracle.

Every case runs twice in this process, on two contexts: the session's, whose per-frame launch of a preset asset takes the preset's kernel, and one created
under GSPLAT_VIEW_GENERIC=1, which always takes the run-time kernel.  The two must agree bit for bit on what that launch leaves behind -- the pixel rectangles,
the visibility words and the raster records -- and each is compared with the oracle the way test_gpu_view.py does (check_raster_records, then the 40-byte
view records).  (A raster record is only written for a visible splat -- the blend reads no other -- so records are compared where the visibility bit is set.)

Cases: the five presets and one combination that is no preset and so runs the run-time kernel on both contexts.  N = 257 and N = 3,000: a partial last
chunk, a partial last wave, two and twelve workgroups.  The camera sits inside the cloud, so that there are splats in front of it and behind it, splats the
early cull drops and whole chunks outside the frustum.  The Medium case carries deleted bits and a cutout.

Low and VeryLow keep their SH in a palette of 16 k / 4 k entries, and the creator (like the reference's) refuses to cluster fewer splats than that.  At these
sizes their assets are therefore put together here: everything but the SH from the creator, the palette drawn like the scene's SH coefficients, one u16 index
after every splat's scale -- the preset's layout, which is all the kernel and the oracle look at."""
import copy
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
from common import views_equal
from builders import CUTOUT_SETS
from gpu_rig import check_raster_records
from unitygaussiansplatting_amd import asset as A
from unitygaussiansplatting_amd import camera, creator, scenes
from unitygaussiansplatting_amd.cutout import shader_data_array
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext

pytestmark = pytest.mark.gpu

EXTENT = 3.0
NOT_A_PRESET = dict(formatPos=A.VectorFormat.Norm16, formatScale=A.VectorFormat.Norm11, formatColor=A.ColorFormat.Float16x4, formatSH=A.SHFormat.Norm6)
CASES = [("VeryHigh", {}), ("High", {}), ("Medium", {}), ("Low", {}), ("VeryLow", {}), ("Medium", NOT_A_PRESET)]
SIZES = [257, 3_000]


@functools.lru_cache(maxsize=None)
def preset_asset(n, quality, fmt_items=()):
    raw = scenes.make_splats(n, 11, EXTENT)
    fmt = dict(fmt_items)
    fsh = A.SHFormat(fmt.get("formatSH", creator.QUALITY[quality][3]))
    if fsh <= A.SHFormat.Norm6:
        return creator.CreateAssetFromSplats(raw, quality, name=f"vp{n}_{quality}", **fmt)
    a = copy.copy(creator.CreateAssetFromSplats(raw, quality, name=f"vp{n}_{quality}", **{**fmt, "formatSH": A.SHFormat.Norm6}))
    rng = np.random.default_rng(n)
    k = A.GetSHCount(fsh, n)
    table = np.zeros((k, 48), "<f2")
    table[:, :45] = (rng.standard_normal((k, 45), dtype=np.float32) * np.float32(0.08)).astype(np.float16)
    stride = A.GetOtherSizeNoSHIndex(a.scaleFormat)
    other = np.zeros((n, stride + 2), np.uint8)
    other[:, :stride] = a.otherData[:n * stride].reshape(n, stride)
    other[:, stride:] = rng.integers(0, k, n).astype("<u2").view(np.uint8).reshape(n, 2)
    a.otherData = np.concatenate([other.reshape(-1), np.zeros(8, np.uint8)])
    a.shData = table.view(np.uint8).reshape(-1).copy()
    a.shFormat = fsh
    a.dataHash = a.ComputeDataHash()
    a.Validate()
    return a


@pytest.fixture(scope="module")
def generic_ctx():
    old = os.environ.get("GSPLAT_VIEW_GENERIC")
    os.environ["GSPLAT_VIEW_GENERIC"] = "1"                 # read once, when the context is created
    try:
        ctx = GpuContext(0)
    finally:
        if old is None:
            del os.environ["GSPLAT_VIEW_GENERIC"]
        else:
            os.environ["GSPLAT_VIEW_GENERIC"] = old
    yield ctx
    ctx.Dispose()


def _frame(ctx, a, cam, cutouts, bits):
    """One frame's calc_view on `ctx`: (recs, rects, vis) of the per-frame launch, then the renderer (for the oracle checks)."""
    r = GaussianSplatRenderer(ctx, a)
    r.OnEnable()
    r.m_Cutouts = cutouts
    r.SetDeletedBits(bits)
    r.SortPoints(cam)
    r.CalcViewData(cam)
    return r.DownloadRasterRecords(), r


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("quality,fmt", CASES, ids=["VeryHigh", "High", "Medium", "Low", "VeryLow", "no_preset"])
def test_preset_kernel_equals_generic_kernel_and_oracle(gpu_ctx, generic_ctx, quality, fmt, n):
    a = preset_asset(n, quality, tuple(sorted(fmt.items())))
    edited = quality == "Medium" and not fmt
    cutouts = CUTOUT_SETS["hole_ellipsoid"] if edited else None
    bits = None
    if edited:
        g = np.random.default_rng(5)
        bits = (g.integers(0, 2 ** 32, (n + 31) // 32, dtype=np.uint64) & g.integers(0, 2 ** 32, (n + 31) // 32, dtype=np.uint64)).astype(np.uint32)
    cam = camera.Camera(position=scenes.orbit_eye(1.2, 10.0, 25.0), pixelWidth=320, pixelHeight=200, fieldOfView=39.0965)      # inside the +-3 cloud

    (recs_s, rects_s, vis_s), r_s = _frame(gpu_ctx, a, cam, cutouts, bits)
    (recs_g, rects_g, vis_g), r_g = _frame(generic_ctx, a, cam, cutouts, bits)
    assert np.array_equal(rects_s, rects_g), "pixel rectangles differ between the preset and the run-time kernel"
    assert np.array_equal(vis_s, vis_g), "visibility words differ between the preset and the run-time kernel"
    m = np.unpackbits(vis_s.view(np.uint8), bitorder="little")[:n].astype(bool)
    assert np.array_equal(recs_s[m], recs_g[m]), "raster records differ between the preset and the run-time kernel"

    orc = O.Oracle(a)
    P = r_s.FrameParams(cam)
    arr, ncut = shader_data_array(cutouts, r_s.transform.localToWorldMatrix)
    want = orc.calc_view(P, arr, ncut, bits).copy()
    for r in (r_s, r_g):
        visible = check_raster_records(r, orc, P)
        assert views_equal(r.DownloadView(), want)
        r.OnDisable()
    # the scene exercises every exit of the kernel: drawn, behind the camera, in front of it but never reaching the screen
    front = want["pos"][:, 3] > 0
    assert 0 < visible < int(front.sum()) < n
