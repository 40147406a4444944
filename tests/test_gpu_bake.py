"""The bake on the GPU (csrc/gs_bake.hip through gs_renderer_edit_bake_asset / gs_asset_download_blobs and GaussianSplatRenderer.EditBakeAsset /
CreateResourcesForGpuAsset / GpuAsset) against the yardstick of tests/bake_model.py: the native host importer with linearize = 0 fed with the oracle's
decode of the alive splats in index order (its premises are asserted on the CPU by tests/test_bake_model.py).  Compared after every bake: the five
blobs over gs_import_blob_sizes bytes each, byte for byte; the alive count; the bounds, bit for bit.

Two of the issue's cases are stated as they can be built: a resize needs a VeryHigh target, so "MergeSplatObjects of a Medium and a High renderer"
merges the two INTO a small VeryHigh one; and a lane is an object the C ABI never hands out, so its refusal cannot be provoked from outside the
library.  The coplanar case orders the yardstick's input by the model's key with the degenerate component forced to 0 and imports it with morton = 0:
the form that does not lean on the host's conversion of a NaN (tests/test_bake_model.py::test_premise_degenerate_axis shows the two agree here)."""
import ctypes as C

import numpy as np
import pytest

import bake_model as BM
import copy_model as CM
import crafted
import edit_model as EM
import export_model as XM
import transform_model as TM
from builders import decode_of
from common import PRESETS, default_camera, small_asset
from gpu_rig import BAD, CAM, bake, check_bake, frame_of, keep_only, pinned_renderer as make_renderer, same_frame
from unitygaussiansplatting_amd import _abi, _lib, asset as A, camera
from unitygaussiansplatting_amd.cutout import GaussianCutout, Type
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, MergeSplatObjects, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
f32 = np.float32


# ---- 1. chunk tails ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alive", [1, 255, 256, 257, 513])
def test_chunk_tails(gpu_ctx, alive):
    """a lone splat, a chunk one short, a full chunk, a one-splat last chunk, and a third chunk (513: also past the first wave of it): every second
    splat of an 1,100-splat High source, into Medium and VeryHigh"""
    r = make_renderer(gpu_ctx, small_asset(1100, 5, "High"))
    src = np.arange(alive) * 2 + 1
    keep_only(r, 1100, src)
    try:
        for formats in (BM.MEDIUM, BM.VERY_HIGH):
            check_bake(r, decode_of(1100, "High")[src], formats, (alive, formats))
    finally:
        r.DisposeResourcesForAsset()


# ---- 2. the alive mask ------------------------------------------------------------------------------------------------------------------------
def test_alive_mask(gpu_ctx):
    n = 700
    asset = small_asset(n, 5, "Medium")
    r = make_renderer(gpu_ctx, asset)
    m = XM.ExportModel(asset, decode_of(n, "Medium"))
    flags = np.zeros(n, bool)
    flags[[0, 31, 32, 63, 64, 255, 256, n - 1]] = True             # both sides of every word boundary
    words = EM.pack_bits(flags, (n + 31) // 32)
    cuts = [GaussianCutout(Type.Box, False, camera.Transform(position=(0.2, 0.0, -0.1), scale=(2.5, 2.0, 2.5))),
            GaussianCutout(Type.Ellipsoid, True, camera.Transform(position=(0.5, 0.3, 0.0), scale=(1.2, 0.8, 0.9)))]
    try:
        for what, w, c in (("bits", words, None), ("bits + cutouts", words, cuts), ("cutouts", None, cuts)):
            r.SetDeletedBits(w); r.m_Cutouts = c
            m.edit.set_deleted_bits(w); m.edit.set_cutouts(c, r.transform.localToWorldMatrix)
            alive = m.alive()
            assert 0 < alive.sum() < n and (c is None or m.edit.cut.sum() > 50)
            check_bake(r, m.dec[alive], BM.MEDIUM, what)
    finally:
        r.DisposeResourcesForAsset()


# ---- 3. every target format -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(BM.FORMAT_TARGETS)))
def test_target_formats(gpu_ctx, k):
    r = make_renderer(gpu_ctx, small_asset(600, 5, "VeryHigh"))
    try:
        check_bake(r, decode_of(600, "VeryHigh"), BM.FORMAT_TARGETS[k], BM.FORMAT_TARGETS[k])
    finally:
        r.DisposeResourcesForAsset()


# ---- 4. every source preset -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", PRESETS)
def test_source_presets(gpu_ctx, quality):
    """the first 513 splats of a 20,000-splat asset of each preset (a Cluster palette needs more splats than entries), the rest deleted"""
    r = make_renderer(gpu_ctx, small_asset(20000, 5, quality))
    keep_only(r, 20000, np.arange(513))
    try:
        check_bake(r, decode_of(20000, quality)[:513], BM.MEDIUM, quality)
    finally:
        r.DisposeResourcesForAsset()


# ---- 5. the sort ------------------------------------------------------------------------------------------------------------------------------
def test_sort_spans_partitions(gpu_ctx):
    """20,000 alive splats: both Onesweep sorts run over several partitions"""
    r = make_renderer(gpu_ctx, small_asset(20000, 5, "Medium"))
    try:
        check_bake(r, decode_of(20000, "Medium"), BM.MEDIUM, "20000")
    finally:
        r.DisposeResourcesForAsset()


def duplicate_positions(n=1000, dup=200, seed=11) -> np.ndarray:
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) * 6.0 - 3.0).astype(f32)
    where = rng.permutation(n)[:dup]
    pos[where] = pos[where[:3]][np.arange(dup) % 3]
    return pos


def point_cloud(pos) -> A.GaussianSplatAsset:
    rng = np.random.default_rng(3)
    return crafted.asset(pos, (rng.random((len(pos), 3)) * 0.05 + 0.01).astype(f32))      # distinct scales: equal positions stay distinguishable


def test_equal_codes_keep_the_source_order(gpu_ctx):
    """200 of 1,000 splats share 3 exact positions: equal codes come out in source index order; and the same source with morton = 0"""
    asset = point_cloud(duplicate_positions())
    dec = CM.decode(asset)
    r = make_renderer(gpu_ctx, asset)
    try:
        want = check_bake(r, dec, BM.MEDIUM, "duplicates")
        plain = check_bake(r, dec, BM.MEDIUM, "duplicates, morton = 0", morton=False)
        assert not np.array_equal(want.posData, plain.posData)
        check_bake(r, dec, BM.VERY_HIGH, "duplicates, chunk-less")
    finally:
        r.DisposeResourcesForAsset()


def test_coplanar_source(gpu_ctx):
    """one axis constant: max == min, the Morton component is 0 x inf = NaN, which the bake defines as 0"""
    pos = (np.random.default_rng(13).random((700, 3)) * 4.0 - 2.0).astype(f32)
    pos[:, 1] = f32(0.75)
    asset = point_cloud(pos)
    dec = CM.decode(asset)
    assert np.array_equal(dec[:, 0:3], pos)
    order = np.argsort(BM.morton_codes(pos, pos.min(axis=0), pos.max(axis=0)), kind="stable")
    r = make_renderer(gpu_ctx, asset)
    try:
        check_bake(r, dec, BM.MEDIUM, "coplanar", want=BM.yardstick(dec[order], BM.MEDIUM, morton=False))
    finally:
        r.DisposeResourcesForAsset()


# ---- 6. after edits ---------------------------------------------------------------------------------------------------------------------------
def test_after_select_translate_delete(gpu_ctx):
    asset = small_asset(700, 5, "VeryHigh")
    r = make_renderer(gpu_ctx, asset)
    m = TM.TransformModel(asset)
    P = r.FrameParams(CAM)
    rect = EM.PREMISE_RECT
    try:
        r.EditStoreSelectionMouseDown(); m.store_selection()
        r.EditUpdateSelection((rect[0], rect[3]), (rect[2], rect[1]), CAM, False); m.update_selection(P, rect, False)
        sel = r.DownloadEditBits()[0]
        assert np.array_equal(sel, m.bits()[0]) and 10 < EM.popcount(sel) < 690
        delta = np.array([0.25, -0.5, 0.125], f32)
        r.EditTranslateSelection(delta); assert m.translate(delta)
        check_bake(r, CM.decode(m.current_asset()), BM.MEDIUM, "translated")         # the private positions are what is baked
        r.EditDeleteSelected(); m.delete_selected()
        alive = ~EM.unpack_bits(m.bits()[2], 700)
        assert np.array_equal(r.DownloadEditBits()[2], m.bits()[2]) and 10 < alive.sum() < 690
        check_bake(r, CM.decode(m.current_asset())[alive], BM.MEDIUM, "translated, then deleted")
    finally:
        r.DisposeResourcesForAsset()


def test_after_merge(gpu_ctx):
    """the resized VeryHigh path: a Medium and a High renderer merged into a small VeryHigh one, then baked to Medium"""
    tr_t = camera.Transform(position=(-0.4, 0.1, 0.2), rotation=(0.5, -0.5, 0.5, 0.5), scale=(0.8, 1.25, 2.0))
    tr_b = camera.Transform(**XM.BAKE_TRANSFORM)                   # mirrored
    target = make_renderer(gpu_ctx, small_asset(40, 5, "VeryHigh"), tr_t)
    a = make_renderer(gpu_ctx, small_asset(257, 6, "Medium"))
    b = make_renderer(gpu_ctx, small_asset(300, 7, "High"), tr_b)
    words = EM.pack_bits(np.arange(300) % 5 == 0, (300 + 31) // 32)
    b.SetDeletedBits(words)                                        # the merge carries the deleted bits over
    try:
        MergeSplatObjects(target, [a, b])
        want = CM.merge(CM.blobs_of(small_asset(40, 5, "VeryHigh")), tr_t, [(decode_of(257, "Medium", 6), None, camera.Transform()), (decode_of(300, "High", 7), words, tr_b)])
        assert target.splatCount == 597 == want.n
        alive = ~EM.unpack_bits(want.deleted_words(), 597)
        assert alive.sum() == 597 - 60
        check_bake(target, CM.decode(want)[alive], BM.MEDIUM, "merged")
    finally:
        a.DisposeResourcesForAsset(); b.DisposeResourcesForAsset(); target.DisposeResourcesForAsset()


# ---- 7. the source is left as it is -------------------------------------------------------------------------------------------------------------
def test_source_untouched(gpu_ctx):
    asset = small_asset(700, 5, "VeryHigh")
    r = make_renderer(gpu_ctx, asset)
    try:
        r.EditSelectAll()
        r.EditTranslateSelection(np.array([0.1, 0.2, -0.1], f32))   # private blobs
        r.EditDeselectAll()
        rect = EM.PREMISE_RECT
        r.EditStoreSelectionMouseDown()
        r.EditUpdateSelection((rect[0], rect[3]), (rect[2], rect[1]), CAM, False)
        r.EditDeleteSelected()
        r.EditSelectAll()

        def state():
            return list(r.DownloadSplatData()) + list(r.DownloadEditBits()) + list(frame_of(r, gpu_ctx))
        before = state()
        g = bake(r, BM.MEDIUM)
        assert 0 < g.splatCount < 700
        after = state()
        g.Dispose()
        assert len(before) == len(after) == 10
        for k, (x, y) in enumerate(zip(before, after)):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), k
    finally:
        r.DisposeResourcesForAsset()


# ---- 8. with frames in flight -------------------------------------------------------------------------------------------------------------------
def test_bake_between_frames_in_flight(gpu_ctx):
    asset, dec = small_asset(20000, 5, "Medium"), decode_of(20000, "Medium")
    words = EM.pack_bits(np.arange(20000) % 3 == 0, (20000 + 31) // 32)

    def frames(bake_between: bool):
        r = make_renderer(gpu_ctx, asset, mode=SortMode.Visible)
        r.SetFramesInFlight(2)
        assert r.FramesInFlight() == (2, True)
        r.SetDeletedBits(words)
        rts = [RenderTarget(gpu_ctx, 320, 200) for _ in range(4)]
        got = None
        for k, rt in enumerate(rts):
            cam = default_camera(az=25.0 + 9.0 * k)
            r.SortPoints(cam); r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
            if bake_between and k == 1:
                g = bake(r, BM.MEDIUM)
                got = g.Download()
                g.Dispose()
        imgs = [rt.Download() for rt in rts]
        order = r.DownloadOrder()
        for rt in rts:
            rt.Dispose()
        r.DisposeResourcesForAsset()
        return imgs, order, got

    plain, plain_order, _ = frames(False)
    imgs, order, got = frames(True)
    assert all(np.array_equal(x, y) for x, y in zip(plain, imgs)) and np.array_equal(order, plain_order)      # the frames are those of a renderer that never baked
    assert all(img.any() for img in imgs)
    BM.assert_same_asset(got, BM.yardstick(dec[~EM.unpack_bits(words, 20000)], BM.MEDIUM), "between frames in flight")


# ---- 9. the asset is usable ---------------------------------------------------------------------------------------------------------------------
def test_baked_asset_renders_like_the_uploaded_yardstick(gpu_ctx):
    n = 3000
    src = make_renderer(gpu_ctx, small_asset(n, 5, "High"))
    words = EM.pack_bits(np.arange(n) % 4 == 1, (n + 31) // 32)
    src.SetDeletedBits(words)
    g = bake(src, BM.MEDIUM)
    want = BM.yardstick(decode_of(n, "High")[~EM.unpack_bits(words, n)], BM.MEDIUM)
    baked = GaussianSplatRenderer(gpu_ctx)
    baked.CreateResourcesForGpuAsset(g)
    uploaded = make_renderer(gpu_ctx, want)
    try:
        assert baked.splatCount == uploaded.splatCount == g.splatCount == want.splatCount
        host = g.Download()
        assert host.dataHash == want.dataHash and host.dataHash
        assert g.boundsMin == tuple(want.boundsMin) and g.boundsMax == tuple(want.boundsMax)
        for cam in (CAM, default_camera(az=110.0, elev=-20.0)):
            a, b = frame_of(baked, gpu_ctx, cam), frame_of(uploaded, gpu_ctx, cam)
            assert same_frame(a, b) and a[2].any()
    finally:
        baked.DisposeResourcesForAsset(); uploaded.DisposeResourcesForAsset(); src.DisposeResourcesForAsset()
        g.Dispose()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx):
    lib = _lib.lib()
    r = make_renderer(gpu_ctx, small_asset(700, 5, "Medium"))
    before = frame_of(r, gpu_ctx)
    good = (2, 2, 2, 3, 0, 1)

    def refused(rh, fmt, with_out=True, with_alive=True):
        out, alive = C.c_void_p(0x1234), C.c_uint32(7)
        f = None if fmt is None else C.byref(_abi.gs_import_formats(*fmt))
        rc = lib.gs_renderer_edit_bake_asset(rh, f, C.byref(out) if with_out else None, C.byref(alive) if with_alive else None, None, None)
        return rc == BAD and not (with_out and out) and alive.value == 7

    try:
        assert refused(None, good) and refused(r._r_h, None) and refused(r._r_h, good, with_out=False) and refused(r._r_h, good, with_alive=False)
        for k in range(4):                                         # a format enum out of range
            fmt = list(good)
            fmt[k] = 9 if k == 3 else 4
            assert refused(r._r_h, tuple(fmt)), k
        assert refused(r._r_h, (2, 2, 2, 3, 1, 1))                 # linearize != 0
        assert refused(r._r_h, (2, 2, int(A.ColorFormat.BC7), 3, 0, 1))
        for sh in range(int(A.SHFormat.Cluster64k), int(A.SHFormat.Cluster4k) + 1):
            assert refused(r._r_h, (2, 2, 2, sh, 0, 1)), sh
        assert same_frame(frame_of(r, gpu_ctx), before)
        r.SetDeletedBits(EM.pack_bits(np.ones(700, bool), 22))     # no alive splat
        assert refused(r._r_h, good)
        r.SetDeletedBits(None)
        assert same_frame(frame_of(r, gpu_ctx), before)
        check_bake(r, decode_of(700, "Medium"), BM.MEDIUM, "after the refusals")
        ptrs, sizes = (C.c_void_p * 5)(), (C.c_uint64 * 5)()       # gs_asset_download_blobs: more bytes than a blob holds
        buf = np.zeros(16, np.uint8)
        ptrs[0], sizes[0] = buf.ctypes.data, 1 << 40
        assert lib.gs_asset_download_blobs(r._asset_h, ptrs, sizes) == BAD
    finally:
        r.DisposeResourcesForAsset()
