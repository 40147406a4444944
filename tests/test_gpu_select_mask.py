"""-m gpu: selecting through a screen mask (gs_renderer_edit_update_selection_mask, gs_renderer_edit_select_surface_mask and the EditSelectPolygon /
EditSelectBrush compositions; csrc/gs_edit.hip) against the numpy twins of tests/mask_model.py: every word of the selection, on
every preset, with cutouts and deleted bits; the gesture contract; the rectangle tool as a cross-check; the edges of the hit test; the refusals; undo."""
import ctypes as C

import numpy as np
import pytest

import edit_model as EM
import mask_model as MM
import pick_model as PM
from builders import load_golden
from common import PRESETS, default_camera, small_asset
from gpu_rig import BAD, edit_info, pinned_renderer
from unitygaussiansplatting_amd import _lib, camera
from unitygaussiansplatting_amd._lib import GsError
from unitygaussiansplatting_amd.renderer import EditHistoryFlags, GpuContext, RenderTarget

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 97, 61                                                      # no multiple of 32, more than one word per row


def cam_of(w=W, h=H):
    return default_camera(W=w, H=h)


def lasso_masks(w, h):
    """three masks of a w x h screen from the twin: a lasso, a pentagram with its hole, a brush stroke"""
    return (MM.polygon_coverage(w, h, MM.radial_lasso(w, h, 40, 3)), MM.polygon_coverage(w, h, MM.scaled(MM.PENTAGRAM, w, h)),
            MM.stroke_coverage(w, h, MM.random_stroke(w, h, 30, 6), 3.5))


class MaskRig:
    """a renderer and the EditModel of its edit state; every step ends with the comparison of the three bit buffers and of gs_renderer_edit_info"""

    def __init__(self, ctx, asset, w=W, h=H):
        self.ctx, self.r, self.m = ctx, pinned_renderer(ctx, asset), EM.EditModel(asset)
        self.mask = ctx.CreateScreenMask(w, h)
        self.n = asset.splatCount

    def close(self):
        self.mask.Dispose()
        self.r.DisposeResourcesForAsset()

    def check(self, what):
        for name, g, w in zip(("selected", "mouse-down", "deleted"), self.r.DownloadEditBits(), self.m.bits()):
            assert np.array_equal(g, w), (what, name, np.flatnonzero(g != w)[:8].tolist())
        assert np.array_equal(EM.info_words(edit_info(self.r)), self.m.info()), what

    def set_cutouts(self, cuts):
        self.r.m_Cutouts = cuts
        self.r.UpdateCutoutsBuffer()
        self.m.set_cutouts(cuts, self.r.transform.localToWorldMatrix)

    def upload_selected(self, words):
        self.r.UploadSelectedBits(words); self.m.upload_selected(words)

    def store(self):
        self.r.EditStoreSelectionMouseDown(); self.m.store_selection()

    def update(self, params, mask, subtract, what):
        """the mask (H x W bool from the twin) is uploaded, the call made on both sides; returns the number of hits"""
        P = params if not isinstance(params, camera.Camera) else self.r.FrameParams(params)
        self.mask.Upload(mask)
        self.r.EditUpdateSelectionMask(P, self.mask, subtract)
        MM.update_selection_mask(self.m, P, mask, subtract)
        self.check(what)
        return int(MM.mask_hit_flags(self.m.clip_positions(P), self.m.cut, mask).sum())


def random_words(n, seed):
    nw = (n + 31) // 32
    return np.random.default_rng(seed).integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32)


# ---- 1. every preset and size against the twin; the gesture contract ----------------------------------------------------------------------------------
def assets():
    # (the two clustered presets need more splats than their palette has entries: 20,000, as in the attribute suite)
    out = [(f"{n} {q}", n, q) for q in PRESETS[::-1] for n in ((20000,) if q in ("VeryLow", "Low") else (33, 257))]
    return out + [("golden medium_700", 0, "medium_700"), ("golden veryhigh_300", 0, "veryhigh_300")]


@pytest.mark.parametrize("name,n,quality", assets(), ids=[a[0] for a in assets()])
def test_update_selection_mask_equals_the_twin(gpu_ctx, name, n, quality):
    asset = small_asset(n, 5, quality) if n else load_golden(quality)[1]
    n = asset.splatCount
    rig = MaskRig(gpu_ctx, asset)
    cam = cam_of()
    lasso, star, brush = lasso_masks(W, H)
    rig.set_cutouts(EM.cutout_lists()["ellipsoid+inverted box"])
    assert 0 < rig.m.cut.sum() < n
    deleted = random_words(n, 12) & random_words(n, 13)
    rig.r.SetDeletedBits(deleted); rig.m.set_deleted_bits(deleted)
    rig.upload_selected(random_words(n, 14) & random_words(n, 15))      # a non-empty mouse-down copy, tail bits and cut splats included
    rig.store()
    assert rig.m.md.any()
    hits = rig.update(cam, lasso, False, "add")
    hits += rig.update(cam, star, False, "a second call replaces the first call's hits")
    assert np.array_equal(rig.m.sel, rig.m.md | EM.pack_bits(MM.mask_hit_flags(rig.m.clip_positions(rig.r.FrameParams(cam)), rig.m.cut, star), rig.m.nw))
    hits += rig.update(cam, brush, True, "subtract")
    hits += rig.update(cam, np.ones((H, W), bool), True, "subtract everything on screen")
    hits += rig.update(cam, np.zeros((H, W), bool), False, "an empty mask: the mouse-down copy")
    assert np.array_equal(rig.m.sel, rig.m.md) and hits > 0
    rig.set_cutouts(None)
    assert rig.update(cam, np.ones((H, W), bool), False, "without cutouts") > 0
    rig.close()


def test_update_selection_mask_on_a_larger_scene_and_screen(gpu_ctx):
    """20,011 splats (a partial last chunk, many workgroups) through a 333 x 217 lasso, from outside and from inside the scene"""
    w, h = 333, 217
    rig = MaskRig(gpu_ctx, small_asset(20011, 5, "Medium"), w, h)
    lasso, star, brush = lasso_masks(w, h)
    for which, cam in (("orbit", default_camera(W=w, H=h)), ("inside", camera.Camera(position=(0.3, 0.2, 0.1), target=(1.0, 0.0, 0.5), fieldOfView=60.0, pixelWidth=w, pixelHeight=h))):
        a = rig.update(cam, lasso, False, (which, "lasso"))
        rig.store()
        b = rig.update(cam, star, True, (which, "minus the pentagram"))
        c = rig.update(cam, brush, False, (which, "brush"))
        assert a > 500 and b > 100 and c > 0, (which, a, b, c)    # (the twin's hit counts: no step is vacuous; the thin brush meets 21 splats from inside)
    rig.close()


# ---- 2. the rectangle tool as a cross-check ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", ["Medium", "VeryHigh"])
def test_a_rectangle_mask_selects_what_the_rectangle_tool_selects(gpu_ctx, quality):
    asset = small_asset(5003, 5, quality)
    r = pinned_renderer(gpu_ctx, asset)
    cam = cam_of()
    P = r.FrameParams(cam)
    mask = gpu_ctx.CreateScreenMask(W, H)
    start = random_words(asset.splatCount, 3)
    for box in ((0, 0, W - 1, H - 1), (10, 7, 70, 44), (33, 20, 33, 20), (0, 30, 31, 60)):
        x0, y0, x1, y1 = box
        m = np.zeros((H, W), bool)
        m[y0:y1 + 1, x0:x1 + 1] = True
        rect = np.array(MM.rect_of_mask_box(x0, y0, x1, y1, H), f32)
        for subtract in (False, True):
            r.UploadSelectedBits(start)
            r.EditStoreSelectionMouseDown()
            _lib.check(_lib.lib().gs_renderer_edit_update_selection(r._r_h, C.byref(P), rect.ctypes.data_as(C.POINTER(C.c_float)), int(subtract)), "update_selection")
            want = r.DownloadEditBits()[0]
            r.UploadSelectedBits(start)
            mask.Upload(m)
            r.EditUpdateSelectionMask(P, mask, subtract)
            got = r.DownloadEditBits()[0]
            assert np.array_equal(got, want), (box, subtract, np.flatnonzero(got != want)[:8].tolist())
            if box[2] - box[0] > 5:
                assert not np.array_equal(got, start), (box, subtract)
    mask.Dispose()
    r.DisposeResourcesForAsset()


# ---- 3. the edges of the hit test ----------------------------------------------------------------------------------------------------------------------------
def edge_params(w, h):
    """a frame whose clip position is (x, y, z, z) of the object-space position: pixel positions can be crafted exactly"""
    P = EM.identity_vp_params()
    P.matrix_vp[12:16] = [0.0, 0.0, 1.0, 0.0]
    P.screen_w, P.screen_h = float(w), float(h)
    return P


def test_hit_test_edges(gpu_ctx):
    e = 2.0 ** -20
    pts = np.array([(0.0, 0.0, 1.0),                               # 0 the middle of the screen: hit
                    (-1.0, -1.0, 1.0),                             # 1 px = py = 0: the bottom-left pixel
                    (1.0 - e, 1.0 - e, 1.0),                       # 2 just inside the top-right corner
                    (-1.0 - e, 0.0, 1.0), (1.0, 0.0, 1.0),         # 3, 4 just outside the left edge; px == W
                    (0.0, -1.0 - e, 1.0), (0.0, 1.0, 1.0),         # 5, 6 just outside the bottom edge; py == H
                    (0.0, 0.0, -1.0), (0.3, 0.3, 0.0),             # 7, 8 behind the camera; w == 0
                    (np.nan, 0.0, 1.0), (0.0, np.nan, 1.0), (0.0, 0.0, np.nan),      # 9 .. 11 NaN pixel positions
                    (0.5, -0.5, 2.0)], f32)                        # 12 on screen
    import crafted
    asset = crafted.asset(pts, np.full((len(pts), 3), 0.02, f32))
    rig = MaskRig(gpu_ctx, asset)
    P = edge_params(W, H)
    px, py = EM.pixel_positions(rig.m.clip_positions(P), W, H)
    assert px[1] == 0 and py[1] == 0 and px[2] < W and int(px[2]) == W - 1 and int(py[2]) == H - 1
    assert px[3] < 0 and px[4] == W and py[5] < 0 and py[6] == H and np.isnan(px[9]) and np.isnan(py[10])
    full = np.ones((H, W), bool)
    assert rig.update(P, full, False, "full mask") == 4
    assert EM.unpack_bits(rig.r.DownloadEditBits()[0], len(pts)).nonzero()[0].tolist() == [0, 1, 2, 12]
    corner = np.zeros((H, W), bool)
    corner[H - 1, 0] = True                                        # the bottom-left pixel: py counts up from the bottom edge
    assert rig.update(P, corner, False, "bottom-left pixel") == 1
    assert EM.unpack_bits(rig.r.DownloadEditBits()[0], len(pts)).nonzero()[0].tolist() == [1]
    corner[:] = False
    corner[0, W - 1] = True                                        # the top-right pixel
    assert rig.update(P, corner, False, "top-right pixel") == 1
    assert EM.unpack_bits(rig.r.DownloadEditBits()[0], len(pts)).nonzero()[0].tolist() == [2]
    # the rectangle tool's quirk, for contrast: a NaN pixel position (a NaN w is not "behind") is inside every rectangle, also one nothing projects into
    rect = np.array([-900.0, -900.0, -800.0, -800.0], f32)
    _lib.check(_lib.lib().gs_renderer_edit_update_selection(rig.r._r_h, C.byref(P), rect.ctypes.data_as(C.POINTER(C.c_float)), 0), "update_selection")
    assert EM.unpack_bits(rig.r.DownloadEditBits()[0], len(pts)).nonzero()[0].tolist() == [9, 10, 11]
    rig.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_bits_and_make_no_edit_buffers(gpu_ctx):
    lib = _lib.lib()
    asset = EM.point_asset(257)
    r = pinned_renderer(gpu_ctx, asset)
    r.m_Cutouts = EM.cutout_lists()["ellipsoid"]
    r.UpdateCutoutsBuffer()
    cam = cam_of()
    P = r.FrameParams(cam)
    good, wide, tall = gpu_ctx.CreateScreenMask(W, H), gpu_ctx.CreateScreenMask(W + 1, H), gpu_ctx.CreateScreenMask(W, H - 1)
    other_ctx = GpuContext(0)
    foreign = other_ctx.CreateScreenMask(W, H)
    for m in (good, wide, tall, foreign):
        m.Upload(np.ones((m.height, m.width), bool))
    rt = RenderTarget(gpu_ctx, W, H)                               # no pick output
    picked = RenderTarget(gpu_ctx, W, H)
    picked.SetPickOutput(True)

    def refused_everywhere():
        for m in (wide, tall, foreign):
            assert lib.gs_renderer_edit_update_selection_mask(r._r_h, C.byref(P), m._h, 0) == BAD
            assert lib.gs_renderer_edit_select_surface_mask(r._r_h, picked._h, m._h, 0) == BAD
        assert lib.gs_renderer_edit_select_surface_mask(r._r_h, rt._h, good._h, 0) == BAD, "a target without pick output"
        assert lib.gs_renderer_edit_update_selection_mask(r._r_h, None, good._h, 0) == BAD and lib.gs_renderer_edit_update_selection_mask(r._r_h, C.byref(P), None, 0) == BAD
        assert lib.gs_renderer_edit_select_surface_mask(r._r_h, None, good._h, 0) == BAD and lib.gs_renderer_edit_select_surface_mask(r._r_h, picked._h, None, 0) == BAD
        with pytest.raises(GsError):
            r.EditUpdateSelectionMask(cam, wide)
        with pytest.raises(GsError):
            r.EditSelectSurfaceMask(picked, tall)

    refused_everywhere()
    # no edit buffers were made: gs_renderer_edit_info reports the cut splats only once they exist
    assert edit_info(r).cut == 0 and not r.m_GpuEditSelected
    r.EditUpdateSelectionMask(cam, good)
    sel, md, _ = r.DownloadEditBits()
    assert edit_info(r).cut > 0 and sel.any() and not md.any()
    refused_everywhere()
    got = r.DownloadEditBits()
    assert np.array_equal(got[0], sel) and np.array_equal(got[1], md)
    for t in (good, wide, tall, rt, picked):
        t.Dispose()
    r.DisposeResourcesForAsset()
    other_ctx.Dispose()


# ---- 5. EditSelectSurfaceMask ------------------------------------------------------------------------------------------------------------------------------------
def test_select_surface_mask_against_the_records(gpu_ctx):
    sc = PM.SCENES[0]
    n = sc.asset.splatCount
    r = pinned_renderer(gpu_ctx, sc.asset)
    r.m_OpacityScale = sc.opacity_scale
    r.SetPickTag(5)
    rt = RenderTarget(gpu_ctx, sc.W, sc.H)
    rt.SetPickOutput(True)
    r.SortPoints(sc.cam); r.CalcViewData(sc.cam); rt.Clear(); r.Draw(sc.cam, rt)
    rec = rt.DownloadPick()
    assert (rec["splat"] != 0xFFFFFFFF).sum() > 500
    model = EM.EditModel(sc.asset)
    model._ensure()
    mask = gpu_ctx.CreateScreenMask(sc.W, sc.H)
    lasso, star, brush = lasso_masks(sc.W, sc.H)

    def step(m, subtract, what, tag=5):
        mask.Upload(m)
        r.EditSelectSurfaceMask(rt, mask, subtract)
        model.sel = MM.select_surface_mask(rec, model.sel, m, tag, n, deleted=model.deleted, cut=model.cut, subtract=subtract)
        sel = r.DownloadEditBits()[0]
        assert np.array_equal(sel, model.sel), (what, np.flatnonzero(sel != model.sel)[:8].tolist())
        assert np.array_equal(EM.info_words(edit_info(r)), model.info()), what
        return EM.popcount(model.sel)

    a = step(lasso, False, "lasso")
    b = step(star, True, "minus the pentagram")
    c = step(brush, False, "plus the brush")
    assert a > 50 and b < a and c > b
    assert step(np.zeros((sc.H, sc.W), bool), False, "an empty mask") == c
    r.SetPickTag(6)
    assert step(np.ones((sc.H, sc.W), bool), False, "a tag nobody drew with", tag=6) == c
    r.SetPickTag(5)
    # cutouts, and splats deleted after the draw
    cuts = EM.cutout_lists()["ellipsoid"]
    r.m_Cutouts = cuts
    model.set_cutouts(cuts, r.transform.localToWorldMatrix)
    r.EditDeleteSelected(); model.delete_selected()
    d = step(np.ones((sc.H, sc.W), bool), False, "everything seen, after a delete, with a cutout")
    assert d > 0 and not (model.sel & model.deleted).any() and not EM.unpack_bits(model.sel, n)[model.cut].any()
    # a rectangle as a mask is EditSelectSurface of that rectangle
    for box in ((0, 0, sc.W - 1, sc.H - 1), (10, 8, 40, 30), (33, 20, 33, 20)):
        for subtract in (False, True):
            start = random_words(n, 21)
            m = np.zeros((sc.H, sc.W), bool)
            m[box[1]:box[3] + 1, box[0]:box[2] + 1] = True
            r.UploadSelectedBits(start)
            r.EditSelectSurface(rt, box, subtract)
            want = r.DownloadEditBits()[0]
            r.UploadSelectedBits(start)
            mask.Upload(m)
            r.EditSelectSurfaceMask(rt, mask, subtract)
            assert np.array_equal(r.DownloadEditBits()[0], want), (box, subtract)
            assert np.array_equal(want, PM.select_surface(rec, start, box, 5, n, deleted=model.deleted, cut=model.cut, subtract=subtract))
    mask.Dispose(); rt.Dispose()
    r.DisposeResourcesForAsset()


# ---- 6. the compositions, and undo ----------------------------------------------------------------------------------------------------------------------------
def test_compositions_equal_their_hand_composed_sequences(gpu_ctx):
    asset = small_asset(5003, 5, "Medium")
    r = pinned_renderer(gpu_ctx, asset)
    model = EM.EditModel(asset)
    cam = cam_of()
    P = r.FrameParams(cam)
    start = random_words(asset.splatCount, 5) & random_words(asset.splatCount, 6)
    outline, pts = MM.radial_lasso(W, H, 50, 9), MM.random_stroke(W, H, 25, 4)
    mask = gpu_ctx.CreateScreenMask(W, H)
    mask.Upload(np.ones((H, W), bool))                             # the compositions clear their own mask, not this one
    for subtract in (False, True):
        for tool in ("polygon", "brush"):
            r.UploadSelectedBits(start)
            r.EditStoreSelectionMouseDown()
            if tool == "polygon":
                r.EditSelectPolygon(cam, outline, subtract)
            else:
                r.EditSelectBrush(P, pts, 4.25, subtract)
            got = r.DownloadEditBits()[0]
            r.UploadSelectedBits(start)
            mask.Clear()
            mask.FillPolygon(outline) if tool == "polygon" else mask.Stroke(pts, 4.25)
            r.EditUpdateSelectionMask(P, mask, subtract)
            assert np.array_equal(got, r.DownloadEditBits()[0]), (tool, subtract)
            cov = MM.polygon_coverage(W, H, outline) if tool == "polygon" else MM.stroke_coverage(W, H, pts, 4.25)
            model.upload_selected(start); model.store_selection()
            MM.update_selection_mask(model, P, cov, subtract)
            assert np.array_equal(got, model.sel) and not np.array_equal(got, start), (tool, subtract)
    assert r._screen_mask is not mask and (r._screen_mask.width, r._screen_mask.height) == (W, H)
    mask.Dispose()
    r.DisposeResourcesForAsset()


def test_checkpoint_lasso_delete_undo_undo(gpu_ctx):
    asset = small_asset(5003, 5, "Medium")
    r = pinned_renderer(gpu_ctx, asset)
    cam = cam_of()
    r.EditHistoryEnable(1 << 20)
    start = random_words(asset.splatCount, 7) & random_words(asset.splatCount, 8)
    r.UploadSelectedBits(start)
    r.EditDeleteSelected()
    r.UploadSelectedBits(random_words(asset.splatCount, 9) & random_words(asset.splatCount, 10))
    before = r.DownloadEditBits()
    what = EditHistoryFlags.Selection | EditHistoryFlags.Deleted
    r.EditCheckpoint(what)
    r.EditStoreSelectionMouseDown()
    r.EditSelectPolygon(cam, MM.radial_lasso(W, H, 50, 9))
    lassoed = r.DownloadEditBits()
    assert not np.array_equal(lassoed[0], before[0]) and np.array_equal(lassoed[2], before[2])
    r.EditCheckpoint(what)
    r.EditDeleteSelected()
    after = r.DownloadEditBits()
    assert not after[0].any() and np.array_equal(after[2], before[2] | lassoed[0])
    r.EditUndo()
    got = r.DownloadEditBits()
    assert np.array_equal(got[0], lassoed[0]) and np.array_equal(got[2], lassoed[2]), "the first undo takes back the delete"
    r.EditUndo()
    got = r.DownloadEditBits()
    assert np.array_equal(got[0], before[0]) and np.array_equal(got[2], before[2]), "the second undo takes back the lasso"
    r.EditRedo()
    assert np.array_equal(r.DownloadEditBits()[0], lassoed[0])
    r.DisposeResourcesForAsset()
