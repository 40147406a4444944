"""-m gpu: the selection highlight (gs_renderer_set_selection_highlight; RenderGaussianSplats.shader:63-73,87-101) through calc_view and the blend, held to
the model of tests/highlight_model.py (whose own frame is held to the reference's vert + frag by tests/test_highlight_model.py).  Frames: plain RT_TOL, no
allowance -- the decisions are identical by construction.  Pixel rectangles, raster records and the visibility mask: bit for bit."""
import copy

import numpy as np
import pytest

import crafted as K
import highlight_model as HM
import oracle_lib as O
from common import RT_TOL, default_camera, rt_diff, small_asset
from unitygaussiansplatting_amd import camera
from unitygaussiansplatting_amd._lib import GsError
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderMode, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
SHAPES = ((16, 16), (32, 16), (32, 32))


@pytest.fixture(scope="module")
def hl(tmp_path_factory):
    return HM.build(tmp_path_factory.mktemp("hlg"))


def stats(r, cam, rt):
    try:
        return r.FrameStats()
    except GsError as ex:                                          # GS_ERR_PAIR_OVERFLOW: the pair buffer has been grown, the host draws the frame again
        assert ex.code == -6, ex
        rt.Clear(); r.Draw(cam, rt)
        return r.FrameStats()


def draw(r, cam, rt, sort=True):
    if sort:
        r.SortPoints(cam)
    r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
    st = stats(r, cam, rt)
    return rt.Download(), st


def err(img, ref):
    return float(rt_diff(img, ref).max()) if img.size else 0.0


def assert_records(r, f, what):
    recs, rects, vis = r.DownloadRasterRecords()
    assert np.array_equal(vis, f.vis), (what, "visibility mask")
    assert np.array_equal(rects, f.rects), (what, "pixel rectangles", np.flatnonzero((rects != f.rects).any(axis=1))[:8])
    v = f.visible
    assert np.array_equal(recs[v], f.want_recs[v]), (what, "records", np.flatnonzero(v)[(recs[v] != f.want_recs[v]).any(axis=1)][:8])


def new_renderer(ctx, asset, sort_mode=SortMode.Full, blend=0, highlight=True, tile=None):
    r = GaussianSplatRenderer(ctx, asset)
    r.sortMode = sort_mode
    r.blendMode = blend
    r.selectionHighlight = highlight                               # applied when the native renderer is made
    r.OnEnable()
    if tile:
        r.SetTileShape(*tile)
    return r


# ---- 1. the scene of the CPU tests, both sort modes, both blend modes, the three tile shapes -------------------------------------------------
@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("sort_mode", [SortMode.Full, SortMode.Visible])
def test_scene_every_third_splat_selected(gpu_ctx, hl, sort_mode, blend):
    a = small_asset(3000, 5, "Medium")
    cam = default_camera(W=160, H=100, az=25.0)
    sel = np.zeros(a.splatCount, bool)
    sel[::3] = True
    r = new_renderer(gpu_ctx, a, sort_mode, blend)
    rt = RenderTarget(gpu_ctx, 160, 100)
    r.UploadSelectedBits(HM.bits_of(sel))
    orc = O.Oracle(a)
    orc.sort(camera.sort_matrix(cam, r.transform.localToWorldMatrix))
    P = r.FrameParams(cam)
    view = orc.calc_view(P).copy()
    f = HM.Frame(hl, view, P, HM.bits_of(sel), orc.order)
    want = f.draw(blend)
    plain = orc.draw(P, blend)
    frames = []
    r.SortPoints(cam)
    for shape in SHAPES:
        r.SetTileShape(*shape)
        img, st = draw(r, cam, rt, sort=False)
        what = (sort_mode.name, blend, shape)
        assert (st.tile_w, st.tile_h) == shape and st.sort_error == 0, what
        assert_records(r, f, what)
        assert st.tile_pairs == f.pairs(st) and st.visible_splats == int(f.visible.sum()), (what, st.tile_pairs, f.pairs(st))
        e = err(img, want)
        print(f"{what}: P={st.tile_pairs} visible={st.visible_splats} err={e / RT_TOL:.3f} x RT_TOL")
        assert e <= RT_TOL, (what, e / RT_TOL)
        frames.append(img)
    assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[2])
    assert (rt_diff(frames[0], plain).max(axis=-1) > RT_TOL).mean() > 0.30                    # the highlight is on the frame
    got_view = r.DownloadView()                                    # m_GpuView is the reference's, selection or not; and materialising it keeps the records
    assert np.array_equal(got_view.view(np.uint32), view.view(np.uint32))
    assert_records(r, f, "after the view download")
    r.OnDisable(); rt.Dispose()


# ---- 2. crafted scenes --------------------------------------------------------------------------------------------------------------------
def crafted_cases():
    cases = {}
    b = K.Builder(64, 64)                                          # one splat of sigma ~ 10 px on the corner shared by the four middle tiles: its ring (|q| ~ 1.85,
    s = b.add(32.0, 32.0, 5.0, 10.0, 9.5, (0.2, 0.7, 0.4), 0.6)    # ~26 px out) runs through the twelve outer tiles and crosses tile corners on its way
    cases["ring"] = dict(W=64, H=64, asset=b.build(), selected=s)
    b = K.Builder(48, 40)
    s = b.add(20.5, 17.5, 5.0, 4.0, 3.0, (0.9, 0.1, 0.3), 0.0, angle=0.6)                   # opacity 0: PrepareSplat would cull it
    b.add(30.5, 22.5, 6.0, 3.0, 2.0, (0.1, 0.2, 0.9), 0.8)
    cases["opacity0"] = dict(W=48, H=40, asset=b.build(), selected=s)
    b = K.Builder(64, 64)                                          # an opaque 8x8 brick in front of the selected splat, another behind it: early termination / finished()
    b.add(28.0, 28.0, 4.0, K.SQUARE_SIGMA, K.SQUARE_SIGMA * 1.02, (0.3, 0.9, 0.2), K.SQUARE_OPACITY)
    s = b.add(32.5, 30.5, 5.0, 7.0, 5.0, (0.8, 0.6, 0.1), 0.5, angle=1.0)
    b.add(40.0, 36.0, 6.0, K.SQUARE_SIGMA, K.SQUARE_SIGMA * 1.02, (0.1, 0.3, 0.9), K.SQUARE_OPACITY)
    b.add(20.5, 40.5, 7.0, 6.0, 6.5, (0.5, 0.5, 0.5), 0.9)
    cases["between_opaque"] = dict(W=64, H=64, asset=b.build(), selected=s)
    b = K.Builder(48, 40)
    s = b.add(24.0, 20.0, 5.0, 6.0, 4.0, (0.7, 0.7, 0.1), 0.4, angle=0.3)
    b.add(12.5, 11.5, 3.0, 3.0, 2.5, (0.2, 0.9, 0.9), 0.7)
    depth = np.full((40, 48), 100.0, np.float32)
    depth[:, :24] = 4.0                                            # the left half of the selected splat lies behind the scene
    cases["scene_depth"] = dict(W=48, H=40, asset=b.build(), selected=s, depth=depth)
    b = K.Builder(48, 40)
    s1 = b.add(24.0, 20.0, -3.0, 5.0, 4.0, (0.9, 0.9, 0.9), 1.0)   # behind the camera
    s2 = b.add(20.0, 18.0, 5.0, 5.0, 4.0, (0.9, 0.2, 0.2), 1.0)    # selected AND deleted
    b.add(30.5, 25.5, 6.0, 2.0, 1.5, (0.2, 0.9, 0.2), 0.9)         # the one thing on the frame
    cases["behind_and_deleted"] = dict(W=48, H=40, asset=b.build(), selected=np.concatenate([s1, s2]), deleted=s2, nothing_selected_drawn=True)
    b = K.Builder(1, 1)
    s = b.add(0.5, 0.5, 5.0, 3.0, 2.0, (0.3, 0.6, 0.9), 0.2)
    cases["one_pixel"] = dict(W=1, H=1, asset=b.build(), selected=s)
    return cases


CASES = crafted_cases()


@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted(gpu_ctx, hl, name, blend):
    c = CASES[name]
    a, W, H = c["asset"], c["W"], c["H"]
    n = a.splatCount
    sel = np.zeros(n, bool); sel[c["selected"]] = True
    deleted = None
    if "deleted" in c:
        d = np.zeros(n, bool); d[c["deleted"]] = True
        deleted = HM.bits_of(d)
    cam = K.PixelCamera(W, H).cam
    orc = O.Oracle(a)
    tr = camera.Transform()
    orc.sort(camera.sort_matrix(cam, tr.localToWorldMatrix))
    P = camera.frame_params(cam, tr)
    view = orc.calc_view(P, deleted_bits=deleted).copy()
    f = HM.Frame(hl, view, P, HM.bits_of(sel), orc.order)
    want = f.draw(blend, scene_depth=c.get("depth"), classify=True)
    counts = f.counts
    plain = HM.Frame(hl, view, P, None, orc.order).draw(blend, scene_depth=c.get("depth"))
    # premises: what the case claims to hold
    if c.get("nothing_selected_drawn"):
        assert counts["selected"] == 0 and np.array_equal(want, plain) and want.any()
    else:
        assert counts["selected"] > 0 and not np.array_equal(want, plain)
    if name == "ring":
        ring = (want.view(np.float16) == np.array([1, 0, 1, 1], np.float16)).all(axis=-1)
        tiles = {(y // 16, x // 16) for y, x in np.argwhere(ring)}
        assert counts["ring"] >= 100 and len(tiles) >= 12 and {(0, 0), (0, 3), (3, 0), (3, 3)} <= tiles, (counts, sorted(tiles))
    if name == "opacity0":
        assert (view["color"][c["selected"], 1] & 0xFFFF == 0).all() and f.visible[c["selected"]].all() and counts["ring"] > 0
    if name == "between_opaque":
        A_ = want.view(np.float16)[..., 3]
        assert (A_ == 1.0).sum() >= 128 and counts["ring"] > 0
    if name == "scene_depth":
        nod = HM.Frame(hl, view, P, HM.bits_of(sel), orc.order).draw(blend)
        assert not np.array_equal(nod, want) and np.array_equal(nod[:, 30:], want[:, 30:])
    for sort_mode in (SortMode.Full, SortMode.Visible):
        for shape in SHAPES if name == "ring" else ((16, 16),):
            r = new_renderer(gpu_ctx, a, sort_mode, blend, tile=shape)
            rt = RenderTarget(gpu_ctx, W, H)
            if "depth" in c:
                rt.SetSceneDepth(c["depth"])
            if deleted is not None:
                r.SetDeletedBits(deleted)
            r.UploadSelectedBits(HM.bits_of(sel))
            img, st = draw(r, cam, rt)
            what = (name, blend, sort_mode.name, shape)
            assert_records(r, f, what)
            assert st.tile_pairs == f.pairs(st), what
            e = err(img, want)
            assert e <= RT_TOL, (what, e / RT_TOL)
            r.OnDisable(); rt.Dispose()


# ---- 3. select-all over faint splats: every splat drawn, through the growth of the pair buffers ------------------------------------------------
@pytest.mark.parametrize("sort_mode", [SortMode.Full, SortMode.Visible])
def test_select_all_over_faint_splats_grows_the_pair_buffers(gpu_ctx, hl, sort_mode):
    """2,000 splats of opacity 0.002 (< 1/255: none is drawn), each wider than the 768 x 704 target: selected, every one is drawn with the opacity-1 footprint,
    2,000 x 2,112 tiles of 16 x 16 = more pairs than the 2^22 a renderer starts with"""
    W, H, n = 768, 704, 2000
    rng = np.random.default_rng(8)
    b = K.Builder(W, H)
    b.add(rng.uniform(100, W - 100, n), rng.uniform(100, H - 100, n), rng.uniform(4.0, 8.0, n), rng.uniform(500, 700, n), rng.uniform(500, 700, n),
          rng.uniform(0, 1, (n, 3)), 0.002, angle=rng.uniform(0, 3, n))
    a = b.build()
    cam = K.PixelCamera(W, H).cam
    r = new_renderer(gpu_ctx, a, sort_mode, 0, tile=(16, 16))
    rt = RenderTarget(gpu_ctx, W, H)
    img, st = draw(r, cam, rt)
    assert st.tile_pairs == 0 and st.visible_splats == 0 and not img.any()                    # unselected: nothing
    cap0 = st.pair_capacity
    r.EditSelectAll()
    orc = O.Oracle(a)
    tr = camera.Transform()
    orc.sort(camera.sort_matrix(cam, tr.localToWorldMatrix))
    P = camera.frame_params(cam, tr)
    view = orc.calc_view(P).copy()
    f = HM.Frame(hl, view, P, HM.bits_of(np.ones(n, bool)), orc.order)
    want_pairs = f.pairs((16, 16))
    assert f.visible.all() and want_pairs > cap0 == 1 << 22                                   # premise: the frame does not fit
    r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
    with pytest.raises(GsError) as ex:                                                        # the truncation report, as for any frame that outgrows the buffers
        r.FrameStats()
    assert ex.value.code == -6
    rt.Clear(); r.Draw(cam, rt)
    st = r.FrameStats()
    assert st.tile_pairs == want_pairs and st.visible_splats == n and st.pair_capacity >= want_pairs and st.sort_error == 0
    assert_records(r, f, sort_mode.name)
    e = err(rt.Download(), f.draw(0))
    assert e <= RT_TOL, e / RT_TOL
    r.OnDisable(); rt.Dispose()


# ---- 4. the switch is off by default, and off means off -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sort_mode", [SortMode.Full, SortMode.Visible])
def test_default_off_and_empty_selection_change_nothing(gpu_ctx, sort_mode):
    a = small_asset(3000, 5, "Medium")
    cam = default_camera(W=160, H=100, az=25.0)
    r = new_renderer(gpu_ctx, a, sort_mode, 0, highlight=False)
    rt = RenderTarget(gpu_ctx, 160, 100)
    img0, st0 = draw(r, cam, rt)
    rec0 = r.DownloadRasterRecords()
    view0 = r.DownloadView()
    r.SetSelectionHighlight(True)                                  # on, but no edit buffers yet: nothing changes
    img, st = draw(r, cam, rt, sort=False)
    assert np.array_equal(img, img0) and st.tile_pairs == st0.tile_pairs
    r.SetSelectionHighlight(False)
    sel = np.zeros(a.splatCount, bool); sel[::3] = True
    r.UploadSelectedBits(HM.bits_of(sel))                          # a selection, highlight off: byte-identical frames, records and view
    img, st = draw(r, cam, rt, sort=False)
    rec = r.DownloadRasterRecords()
    assert np.array_equal(img, img0) and st.tile_pairs == st0.tile_pairs
    vis = np.unpackbits(rec0[2].view(np.uint8), bitorder="little")[:a.splatCount].astype(bool)
    assert np.array_equal(rec[2], rec0[2]) and np.array_equal(rec[1], rec0[1]) and np.array_equal(rec[0][vis], rec0[0][vis])
    assert np.array_equal(r.DownloadView().view(np.uint32), view0.view(np.uint32))
    r.SetSelectionHighlight(True)                                  # highlight on: the frame changes, the view buffer does not
    img1, st1 = draw(r, cam, rt, sort=False)
    assert not np.array_equal(img1, img0) and st1.tile_pairs > st0.tile_pairs
    assert np.array_equal(r.DownloadView().view(np.uint32), view0.view(np.uint32))
    r.EditDeselectAll()                                            # highlight on, empty selection: byte-identical to the plain frame
    img, st = draw(r, cam, rt, sort=False)
    assert np.array_equal(img, img0) and st.tile_pairs == st0.tile_pairs
    r.UploadSelectedBits(HM.bits_of(sel))
    r.m_RenderMode = RenderMode.DebugPoints              # the debug render modes do not read the selected bits
    r.SetSelectionHighlight(False); rt.Clear(); r.Draw(cam, rt); dbg0 = rt.Download()
    r.SetSelectionHighlight(True); r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
    assert np.array_equal(rt.Download(), dbg0) and dbg0.any()
    r.OnDisable(); rt.Dispose()


# ---- 5. a move, then a delete, of the selection ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort_mode", [SortMode.Full, SortMode.Visible])
def test_move_then_delete_with_highlight(gpu_ctx, hl, sort_mode):
    a = small_asset(2500, 7, "VeryHigh")                           # chunk-less fp32 positions: the translate's gate passes
    assert a.chunkCount == 0
    cam = default_camera(W=160, H=100, az=40.0)
    sel = np.zeros(a.splatCount, bool); sel[1::4] = True
    bits = HM.bits_of(sel)
    r = new_renderer(gpu_ctx, a, sort_mode, 0)
    rt = RenderTarget(gpu_ctx, 160, 100)
    r.UploadSelectedBits(bits)
    tr = r.transform
    P = r.FrameParams(cam)
    m = camera.sort_matrix(cam, tr.localToWorldMatrix)
    orc = O.Oracle(a)
    orc.sort(m)
    f = HM.Frame(hl, orc.calc_view(P).copy(), P, bits, orc.order)
    img, st = draw(r, cam, rt)
    assert_records(r, f, "before") ; assert err(img, f.draw(0)) <= RT_TOL
    r.EditTranslateSelection((0.35, -0.2, 0.15))                   # the selection moves, highlighted where it now is
    pos, _ = r.DownloadPosOther()
    a2 = copy.copy(a)
    a2.posData = pos
    orc2 = O.Oracle(a2)
    orc2.order = orc.order.copy()                                  # SortPoints sorts the order buffer it has, stably
    orc2.sort(m)
    f2 = HM.Frame(hl, orc2.calc_view(P).copy(), P, bits, orc2.order)
    img2, st = draw(r, cam, rt)
    assert_records(r, f2, "moved"); assert st.tile_pairs == f2.pairs(st)
    assert err(img2, f2.draw(0)) <= RT_TOL and not np.array_equal(img2, img)
    r.EditDeleteSelected()                                         # deleted |= selected, selected = 0: the moved splats go, nothing is highlighted
    orc2.sort(m)
    v3 = orc2.calc_view(P, deleted_bits=bits).copy()
    f3 = HM.Frame(hl, v3, P, np.zeros_like(bits), orc2.order)
    img3, st = draw(r, cam, rt)
    assert_records(r, f3, "deleted"); assert st.tile_pairs == f3.pairs(st)
    assert err(img3, f3.draw(0)) <= RT_TOL and np.array_equal(f3.draw(0), orc2.draw(P, 0))
    r.OnDisable(); rt.Dispose()


# ---- 6. two frames in flight: each frame shows the selection of the time it was dealt ---------------------------------------------------------
def test_frames_in_flight_follow_the_selection(gpu_ctx, hl):
    a = small_asset(3000, 5, "Medium")
    n = a.splatCount
    cams = [default_camera(W=160, H=100, az=25.0 + 30.0 * k) for k in range(6)]
    sels = []
    for k in range(6):
        s = np.zeros(n, bool)
        s[k % 3::3 + k] = True
        sels.append(HM.bits_of(s))
    lanes = new_renderer(gpu_ctx, a, SortMode.Visible, 0, tile=(16, 16))
    lanes.SetFramesInFlight(2)
    assert lanes.FramesInFlight() == (2, True)
    one = new_renderer(gpu_ctx, a, SortMode.Visible, 0, tile=(16, 16))
    targets = [RenderTarget(gpu_ctx, 160, 100) for _ in range(6)]
    for k in range(6):                                             # six frames dealt without waiting for any of them, the selection changed before each
        if k == 3:
            lanes.EditInvertSelection()                            # ... once by a kernel instead of an upload
            sels[3] = lanes.DownloadEditBits()[0]
        else:
            lanes.UploadSelectedBits(sels[k])
        lanes.SortPoints(cams[k]); lanes.CalcViewData(cams[k]); targets[k].Clear(); lanes.Draw(cams[k], targets[k])
    got = [t.Download() for t in targets]
    rt = RenderTarget(gpu_ctx, 160, 100)
    orc = O.Oracle(a)
    for k in range(6):
        one.UploadSelectedBits(sels[k])
        img, st = draw(one, cams[k], rt)
        assert np.array_equal(got[k], img), (k, int((got[k] != img).any(axis=-1).sum()))
        if k:
            assert not np.array_equal(got[k], got[k - 1])
        orc.sort(camera.sort_matrix(cams[k], one.transform.localToWorldMatrix))
        P = one.FrameParams(cams[k])
        f = HM.Frame(hl, orc.calc_view(P).copy(), P, sels[k], orc.order)
        assert err(img, f.draw(0)) <= RT_TOL, k
    lanes.SetSelectionHighlight(False)                             # the switch reaches the lanes
    lanes.SortPoints(cams[0]); lanes.CalcViewData(cams[0]); targets[0].Clear(); lanes.Draw(cams[0], targets[0])
    one.SetSelectionHighlight(False)
    img, _ = draw(one, cams[0], rt)
    assert np.array_equal(targets[0].Download(), img)
    for t in targets + [rt]:
        t.Dispose()
    lanes.OnDisable(); one.OnDisable()


# ---- 7. the setting survives EditSetSplatCount ---------------------------------------------------------------------------------------------------
def test_setting_survives_a_resize(gpu_ctx, hl):
    a = small_asset(300, 5, "VeryHigh")
    cam = default_camera(W=160, H=100, az=25.0)
    r = new_renderer(gpu_ctx, a, SortMode.Full, 0)
    rt = RenderTarget(gpu_ctx, 160, 100)
    r.EditSetSplatCount(130)
    img0, st0 = draw(r, cam, rt)                                   # the resize starts with an empty selection
    sel = np.zeros(130, bool); sel[::2] = True
    r.UploadSelectedBits(HM.bits_of(sel))
    img1, st1 = draw(r, cam, rt)
    assert not np.array_equal(img1, img0) and st1.tile_pairs > st0.tile_pairs
    recs, _, vis = r.DownloadRasterRecords()
    v = np.unpackbits(vis.view(np.uint8), bitorder="little")[:130].astype(bool)
    assert (((recs[:, 7] & 0xFFFF) == HM.SELECTED_ALPHA_HALF)[v] == sel[v]).all() and (sel & v).sum() > 10
    r.OnDisable(); rt.Dispose()
