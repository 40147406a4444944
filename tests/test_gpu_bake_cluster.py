"""-m gpu: the bake to the Cluster* SH targets (csrc/gs_bake.hip + the device-resident Lloyd loop of csrc/gs_cluster.hip through
gs_renderer_edit_bake_asset / GaussianSplatRenderer.EditBakeAsset) against the yardstick of tests/bake_model.py: the native host importer with
linearize = 0 fed with the oracle's decode of the alive splats in index order.  Compared after every bake: the five blobs -- `other` with its index
halfword and the SH table among them -- byte for byte, the alive count, the bounds bit for bit.  Every yardstick input is finite and free of -0
(bake_model.assert_no_negative_zero): the byte contract of the palette holds for finite SH only.

Two yardsticks are too slow for the host importer's assignment passes (200,300 x 4,096 and 17,000 x 16,384 take 16 s and 6 s on eight threads); they
are built with CreateAssetFromSplatsNative(context=gpu_ctx), whose bytes tests/test_gpu_import_cluster.py holds to the host's.  That route still sums
the means on the host: only the assignment kernel is shared with the code under test."""
import ctypes as C

import numpy as np
import pytest

import bake_model as BM
import cluster_model as KM
import copy_model as CM
import edit_model as EM
import export_model as XM
from builders import CLUSTER4K, LOW, decode_of
from common import PRESETS, default_camera, small_asset
from gpu_rig import BAD, CAM, check_bake, frame_of, keep_only, pinned_renderer as make_renderer, same_frame, yardstick
from unitygaussiansplatting_amd import _abi, _lib, asset as A, camera, creator
from unitygaussiansplatting_amd.cutout import GaussianCutout, Type
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

pytestmark = pytest.mark.gpu
f32 = np.float32
VF, CF, SF = A.VectorFormat, A.ColorFormat, A.SHFormat


def check_cluster_bake(r, dec_alive, formats, what, morton=True, ctx=None):
    """one bake against the Cluster yardstick (ctx: its assignment passes on the GPU)"""
    return check_bake(r, dec_alive, formats, what, morton, want=yardstick(dec_alive, formats, morton, ctx))


def table_index(asset: A.GaussianSplatAsset) -> np.ndarray:
    """the u16 SH table index of every splat, read off `other`"""
    rec = 4 + {VF.Float32: 12, VF.Norm16: 6, VF.Norm11: 4, VF.Norm6: 2}[VF(asset.scaleFormat)] + 2
    return np.ascontiguousarray(asset.otherData[:asset.splatCount * rec].reshape(-1, rec)[:, rec - 2:]).view(np.uint16).reshape(-1)


# ---- 1. the target of the small presets, both orders ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("morton", [True, False])
def test_very_high_to_cluster4k(gpu_ctx, morton):
    r = make_renderer(gpu_ctx, small_asset(4500, 5, "VeryHigh"))
    try:
        want = check_cluster_bake(r, decode_of(4500, "VeryHigh"), CLUSTER4K, ("Cluster4k", morton), morton)
        assert len(want.shData) == 4096 * 96 and len(np.unique(table_index(want))) > 3000
    finally:
        r.DisposeResourcesForAsset()


# ---- 2. the `other` records of 10, 12 and 18 bytes (8: above) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,record", [(VF.Norm11, 10), (VF.Norm16, 12), (VF.Float32, 18)])
def test_other_record_sizes(gpu_ctx, scale, record):
    formats = (VF.Norm11, scale, CF.Norm8x4, SF.Cluster4k)
    r = make_renderer(gpu_ctx, small_asset(4500, 5, "VeryHigh"))
    try:
        want = check_cluster_bake(r, decode_of(4500, "VeryHigh"), formats, formats)
        assert len(want.otherData) == (4500 * record + 7) // 8 * 8
    finally:
        r.DisposeResourcesForAsset()


def test_cluster8k(gpu_ctx):
    formats = (VF.Norm16, VF.Float32, CF.Float16x4, SF.Cluster8k)
    r = make_renderer(gpu_ctx, small_asset(9000, 5, "VeryHigh"))
    try:
        check_cluster_bake(r, decode_of(9000, "VeryHigh"), formats, "Cluster8k")
    finally:
        r.DisposeResourcesForAsset()


# ---- 3. every source preset ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", PRESETS)
def test_source_presets(gpu_ctx, quality):
    """the first 4,500 splats of a 20,000-splat asset of each preset (a Cluster palette as the SOURCE needs more splats than entries), the rest deleted"""
    r = make_renderer(gpu_ctx, small_asset(20000, 5, quality))
    keep_only(r, 20000, np.arange(4500))
    try:
        check_cluster_bake(r, decode_of(20000, quality)[:4500], CLUSTER4K, quality)
    finally:
        r.DisposeResourcesForAsset()


# ---- 4. the alive mask -----------------------------------------------------------------------------------------------------------------------------
def test_deleted_bits_and_cutouts(gpu_ctx):
    n = 9000
    asset = small_asset(n, 5, "VeryHigh")
    r = make_renderer(gpu_ctx, asset)
    m = XM.ExportModel(asset, decode_of(n, "VeryHigh"))
    words = EM.pack_bits(np.arange(n) % 5 == 2, (n + 31) // 32)
    cuts = [GaussianCutout(Type.Ellipsoid, True, camera.Transform(position=(0.5, 0.3, 0.0), scale=(1.2, 0.8, 0.9)))]
    try:
        r.SetDeletedBits(words); r.m_Cutouts = cuts
        m.edit.set_deleted_bits(words); m.edit.set_cutouts(cuts, r.transform.localToWorldMatrix)
        alive = m.alive()
        assert 4096 < alive.sum() < n * 4 // 5 and m.edit.cut.sum() > 50
        check_cluster_bake(r, m.dec[alive], CLUSTER4K, "bits + cutouts")
    finally:
        r.DisposeResourcesForAsset()


# ---- 5. the importer's rule: more alive splats than table entries ----------------------------------------------------------------------------------
def test_as_many_alive_as_entries_is_refused_one_more_is_accepted(gpu_ctx):
    lib = _lib.lib()
    n = 4500
    r = make_renderer(gpu_ctx, small_asset(n, 5, "VeryHigh"))
    fmt = _abi.gs_import_formats(*[int(f) for f in CLUSTER4K], 0, 1)

    def refused():
        out, alive = C.c_void_p(0x1234), C.c_uint32(7)
        rc = lib.gs_renderer_edit_bake_asset(r._r_h, C.byref(fmt), C.byref(out), C.byref(alive), None, None)
        return rc == BAD and not out and alive.value == 7
    try:
        for alive in (4096, 4095):
            keep_only(r, n, np.arange(alive))
            assert refused(), alive
            assert b"more splats than table entries" in lib.gs_last_error_string()
        keep_only(r, n, np.arange(4097))
        check_cluster_bake(r, decode_of(n, "VeryHigh")[:4097], CLUSTER4K, "4,097 alive")
    finally:
        r.DisposeResourcesForAsset()


# ---- 6. empty clusters and one long cluster ----------------------------------------------------------------------------------------------------------
def test_crafted_empty_and_long_clusters(gpu_ctx):
    """6,000 splats of which 2,500 share one SH row and 500 another: the stride-sampled seeds repeat, so about two thousand clusters never get a point
    and one holds 2,500 -- paths the random scenes never reach.  Built as a VeryHigh asset, where fp32 SH decodes exactly."""
    dec = KM.crafted_decode()
    asset = creator.CreateAssetFromSplats(BM.columns(dec), "VeryHigh", linearize=False, morton=False, name="crafted")
    dec2 = CM.decode(asset)
    assert np.array_equal(dec2[:, 14:59].view(np.uint32), np.ascontiguousarray(dec[:, 14:59]).view(np.uint32))
    r = make_renderer(gpu_ctx, asset)
    try:
        want = check_cluster_bake(r, dec2, CLUSTER4K, "crafted")
        cnt = np.bincount(table_index(want), minlength=4096)
        assert (cnt == 0).sum() >= 1500 and cnt.max() >= 2500
    finally:
        r.DisposeResourcesForAsset()


# ---- 7. the training subset ------------------------------------------------------------------------------------------------------------------------
def test_more_than_200k_alive_takes_the_subset(gpu_ctx):
    """200,300 alive: the Lloyd passes run on the 200,000 stride-sampled rows, the final assignment on all.  (Seed 6: seeds 5 and 7 hold one -0.)"""
    n = 200300
    r = make_renderer(gpu_ctx, small_asset(n, 6, "VeryHigh"))
    try:
        check_cluster_bake(r, decode_of(n, "VeryHigh", 6), CLUSTER4K, "200,300", ctx=gpu_ctx)
    finally:
        r.DisposeResourcesForAsset()


# ---- 8. the asset is usable --------------------------------------------------------------------------------------------------------------------------
def test_baked_low_asset_renders_like_the_uploaded_yardstick(gpu_ctx):
    n = 20000
    src = make_renderer(gpu_ctx, small_asset(n, 5, "High"))
    words = EM.pack_bits(np.arange(n) % 8 == 1, (n + 31) // 32)
    src.SetDeletedBits(words)
    g = src.EditBakeAsset("Low")
    want = yardstick(decode_of(n, "High")[~EM.unpack_bits(words, n)], LOW, ctx=gpu_ctx)
    baked = GaussianSplatRenderer(gpu_ctx)
    baked.CreateResourcesForGpuAsset(g)
    uploaded = make_renderer(gpu_ctx, want)
    try:
        assert baked.splatCount == uploaded.splatCount == g.splatCount == want.splatCount == 17500
        host = g.Download()
        BM.assert_same_asset(host, want, "Low")
        assert host.dataHash == want.dataHash and host.dataHash
        for cam in (CAM, default_camera(az=110.0, elev=-20.0)):
            a, b = frame_of(baked, gpu_ctx, cam), frame_of(uploaded, gpu_ctx, cam)
            assert same_frame(a, b) and a[2].any()
    finally:
        baked.DisposeResourcesForAsset(); uploaded.DisposeResourcesForAsset(); src.DisposeResourcesForAsset()
        g.Dispose()


def test_very_low_needs_another_colour_format(gpu_ctx):
    """BC7 stays refused, hence the preset VeryLow as a whole; with another colour format it is the target of test 1"""
    r = make_renderer(gpu_ctx, small_asset(4500, 5, "VeryHigh"))
    try:
        with pytest.raises(_lib.GsError, match="BC7 colour target") as refusal:
            r.EditBakeAsset("VeryLow")
        assert refusal.value.code == BAD
        g = r.EditBakeAsset("VeryLow", formatColor=CF.Norm8x4)
        assert g.splatCount == 4500
        g.Dispose()
    finally:
        r.DisposeResourcesForAsset()
