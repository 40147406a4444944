"""-m gpu: the pick output (gs_target_set_pick_output) -- per-pixel surface depth and splat id from the blend -- held to the
unchanged CPU oracle through tests/pick_model.py: exact records on decidable pixels, self-consistent ones on the others, the ambiguous share within its cap;
crafted scenes whose every pixel is decidable; and gs_renderer_edit_select_surface against its numpy twin."""
import ctypes as C
import functools

import numpy as np
import pytest

import crafted as K
import edit_model as EM
import oracle_lib as O
import pick_model as PM
from common import _p
from gpu_rig import BAD, edit_info
from unitygaussiansplatting_amd import _abi, _lib, camera
from unitygaussiansplatting_amd._lib import GsError
from unitygaussiansplatting_amd.cutout import shader_data_array
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderMode, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
SHAPES = K.TILE_SHAPES
NONE = _abi.GS_PICK_NO_SPLAT


def new_renderer(ctx, asset, blend=0, sort_mode=SortMode.Full, frames=1, tag=0, opacity=1.0, tile=None, highlight=False):
    r = GaussianSplatRenderer(ctx, asset)
    r.sortMode, r.framesInFlight, r.blendMode, r.m_OpacityScale, r.pickTag, r.selectionHighlight = sort_mode, frames, blend, opacity, tag, highlight
    r.OnEnable()
    if tile:
        r.SetTileShape(*tile)
    return r


def pick_target(ctx, W, H, tau=0.5):
    rt = RenderTarget(ctx, W, H)
    rt.SetPickOutput(True, tau)
    return rt


def draw(r, cam, rt, sort=True, clear=True):
    if sort:
        r.SortPoints(cam)
    r.CalcViewData(cam)
    if clear:
        rt.Clear()
    r.Draw(cam, rt)                                                # (a few thousand pairs at most: far below the smallest pair buffer)
    return rt.DownloadPick()


def tile_of(r):
    st = r.FrameStats()
    assert st.sort_error == 0
    return st.tile_w, st.tile_h


def same_records(a, b) -> bool:
    return np.array_equal(PM.record_words(a), PM.record_words(b))


def assert_exact(got, want, what):
    bad = (PM.record_words(got) != PM.record_words(want)).any(axis=-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6].tolist(), want[bad][:6].tolist())


# ---- 1. parity on the fixed scenes, 2. pixels unchanged ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("scene", [s.name for s in PM.SCENES])
def test_parity_with_the_oracle_and_pixels_unchanged(gpu_ctx, scene, blend):
    sc = next(s for s in PM.SCENES if s.name == scene)
    orc, P, exp = PM.scene_expected(scene, blend)
    w = orc.view["pos"][:, 3]
    r = new_renderer(gpu_ctx, sc.asset, blend, opacity=sc.opacity_scale)
    plain = RenderTarget(gpu_ctx, sc.W, sc.H)
    r.SortPoints(sc.cam); r.CalcViewData(sc.cam); plain.Clear(); r.Draw(sc.cam, plain)
    pixels_off = plain.Download()
    assert np.array_equal(r.DownloadView()["pos"][:, 3].view(np.uint32), w.view(np.uint32))      # premise: the depths a record can carry are the oracle's bits
    for tau in PM.TAUS:
        rt = pick_target(gpu_ctx, sc.W, sc.H, tau)
        got = draw(r, sc.cam, rt, sort=False)
        PM.check_records(got, exp[tau], w, orc.n, (scene, blend))
        assert np.array_equal(rt.Download(), pixels_off), (scene, blend, tau, "pick output changed the pixels")
        x, y = np.argwhere(exp[tau].crossed & exp[tau].decidable)[0][::-1]
        d, s, t = rt.PickAt(int(x), int(y))
        assert (np.float32(d).view(np.uint32), s, t) == (got["depth"][y, x].view(np.uint32), got["splat"][y, x], 0) and s < orc.n
        rt.Dispose()
    plain.Dispose(); r.OnDisable()


# ---- 3. tile shapes, 4. sort modes, 5. frames in flight: the same bits --------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(33, 17), (1, 1)], ids=["33x17", "1x1"])
@pytest.mark.parametrize("blend", [0, 1], ids=["exact", "fast"])
def test_tile_shapes_give_the_same_records(gpu_ctx, size, blend):
    from common import default_camera
    W, H = size
    sc = PM.SCENES[0]
    cam = default_camera(W=W, H=H, radius=sc.radius)
    r = new_renderer(gpu_ctx, sc.asset, blend, opacity=sc.opacity_scale)
    rt = pick_target(gpu_ctx, W, H)
    r.SortPoints(cam)
    planes = []
    for shape in SHAPES:
        r.SetTileShape(*shape)
        planes.append(draw(r, cam, rt, sort=False))
        assert tile_of(r) == shape
    assert (planes[0]["splat"] != NONE).any(), "premise: something is crossed"
    assert same_records(planes[0], planes[1]) and same_records(planes[0], planes[2])
    r.OnDisable(); rt.Dispose()


def test_sort_modes_give_the_same_records(gpu_ctx):
    sc = PM.SCENES[1]
    planes = []
    for mode in (SortMode.Full, SortMode.Visible):
        r = new_renderer(gpu_ctx, sc.asset, 0, sort_mode=mode, opacity=sc.opacity_scale)
        rt = pick_target(gpu_ctx, sc.W, sc.H, 0.95)
        planes.append(draw(r, sc.cam, rt))
        r.OnDisable(); rt.Dispose()
    assert (planes[0]["splat"] != NONE).any()
    assert same_records(planes[0], planes[1])


def test_frames_in_flight_give_the_same_records(gpu_ctx):
    from common import default_camera
    sc = PM.SCENES[0]
    cams = [default_camera(W=sc.W, H=sc.H, radius=sc.radius, az=az) for az in (25.0, 110.0, 250.0, 300.0)]
    out = []
    for frames in (1, 2):
        r = new_renderer(gpu_ctx, sc.asset, 0, sort_mode=SortMode.Visible, opacity=sc.opacity_scale)
        if frames > 1:
            r.SetFramesInFlight(frames)
            assert r.FramesInFlight() == (frames, True)
        rt = pick_target(gpu_ctx, sc.W, sc.H)
        out.append([draw(r, cam, rt) for cam in cams])             # the same target on alternating lanes: its records are doubled like its pixels
        r.OnDisable(); rt.Dispose()
    for k, (a, b) in enumerate(zip(*out)):
        assert (a["splat"] != NONE).any()
        assert same_records(a, b), (k, int((PM.record_words(a) != PM.record_words(b)).any(axis=-1).sum()))
    assert not same_records(out[0][0], out[0][1])                  # premise: the cameras see different surfaces


# ---- 6. crafted scenes: every pixel decidable, the whole plane exact -----------------------------------------------------------------------------------------
BIG_DOT = 0.3                                                       # a dot of opacity 0.3: one dot stays below tau = 0.5, the second on the same pixel crosses (0.51)


@functools.lru_cache(maxsize=None)
def crafted_scene(tile) -> K.Scene:
    """Tile (1, 1) of a 3 x 3-tile target with partial last tiles.  Quadrant (0, 0): an opaque square first of all -- it crosses and finishes in one fragment.
    The other quadrants but the last: squares too, so those waves finish in the first batch.  Then 2 NT + 9 dots behind the squares (they add exactly 0) fill
    two staging batches.  The LAST quadrant holds, in the first batch, faint dots (alpha 0.005: covered, never near tau) and, behind everything else of the
    tile -- in the third batch -- the square that crosses it, and a second square behind that one, which must not take the record over.
    Tile (0, 0): pixels four apart with one, two and three dots of opacity 0.3: one dot leaves the pixel below tau ("none"), the second crosses it."""
    tw, th = tile
    nt = tw * th
    W, H = 3 * tw - 5, 3 * th - 3
    b = K.Builder(W, H)
    rng = np.random.default_rng(tw * 10 + th)
    x0, y0 = tw, th
    quads = K.quadrants_of(tile)
    late = quads[-1]
    col = lambda n: rng.uniform(0.2, 1.0, (n, 3))
    first = b.add(x0 + 4.0, y0 + 4.0, 3.0, K.SQUARE_SIGMA, K.SQUARE_SIGMA * 1.02, col(1), K.SQUARE_OPACITY)
    early = [q for q in quads[1:] if q != late]
    squares = b.add([x0 + 8 * qx + 4.0 for qx, _ in early], [y0 + 8 * qy + 4.0 for _, qy in early], 3.001 + 1.0e-3 * np.arange(len(early)),
                    K.SQUARE_SIGMA, K.SQUARE_SIGMA * 1.02, col(len(early)), K.SQUARE_OPACITY)
    lx0, ly0 = x0 + 8 * late[0], y0 + 8 * late[1]
    faint = b.add(lx0 + np.arange(8) + 0.5, ly0 + (np.arange(8) * 3) % 8 + 0.5, 3.05 + 1.0e-4 * np.arange(8), K.DOT_SIGMA[0], K.DOT_SIGMA[1], col(8), K.DOT_OPACITY)
    pix = np.array([(x0 + 8 * qx + i, y0 + 8 * qy + j) for qx, qy in [quads[0]] + early for j in range(8) for i in range(8)])
    nfill = 2 * nt + 9
    sel = pix[rng.integers(0, len(pix), nfill)]
    fill = b.add(sel[:, 0] + 0.5, sel[:, 1] + 0.5, 3.1 + 1.0e-4 * np.arange(nfill), K.DOT_SIGMA[0], K.DOT_SIGMA[1], col(nfill), K.DOT_OPACITY)
    crosser = b.add(lx0 + 4.0, ly0 + 4.0, 3.5, K.SQUARE_SIGMA, K.SQUARE_SIGMA * 1.02, col(1), K.SQUARE_OPACITY)
    behind = b.add(lx0 + 4.0, ly0 + 4.0, 3.6, K.SQUARE_SIGMA, K.SQUARE_SIGMA * 1.02, col(1), K.SQUARE_OPACITY)
    px = np.array([2.5, 6.5, 6.5, 10.5, 10.5, 10.5])
    depth = np.array([4.0, 4.0, 4.1, 4.0, 4.1, 4.2])
    dots = b.add(px, np.full(6, 5.5), depth, K.DOT_SIGMA[0], K.DOT_SIGMA[1], col(6), BIG_DOT)
    return K.Scene(f"pick_{tw}x{th}", W, H, b.build(), dict(tile=tile, first=first, squares=squares, faint=faint, fill=fill, crosser=crosser, behind=behind, dots=dots,
                                                            late=(lx0, ly0), origin=(x0, y0)))


def oracle_of(scene: K.Scene, sort=True, deleted_bits=None):
    orc = O.Oracle(scene.asset)
    tr = camera.Transform()
    if sort:
        orc.sort(camera.sort_matrix(scene.cam, tr.localToWorldMatrix))
    P = camera.frame_params(scene.cam, tr)
    orc.calc_view(P, deleted_bits=deleted_bits)
    return orc, P


@pytest.mark.parametrize("blend", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("tile", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_crafted_scene_every_pixel_exact(gpu_ctx, tile, blend):
    sc = crafted_scene(tile)
    m = sc.meta
    nt = tile[0] * tile[1]
    orc, P = oracle_of(sc)
    e = PM.expected(orc, P, blend, (0.5,))[0.5]
    assert not e.ambiguous.any(), "premise: no prefix alpha of the crafted scene comes near tau"
    # premises, from the oracle alone: what the scene claims
    order = PM.draw_order(orc, P)
    on_tile = K.tile_list(orc.raster_records(P)[1], order, tile, 1, 1)
    assert list(on_tile).index(int(m["crosser"][0])) > 2 * nt, "the crossing splat sits behind more than 2 NT records of its tile's list"
    (lx0, ly0), (x0, y0) = m["late"], m["origin"]
    want = e.records
    assert (want["splat"][ly0:ly0 + 8, lx0:lx0 + 8] == m["crosser"][0]).all() and (want["splat"][y0:y0 + 8, x0:x0 + 8] == m["first"][0]).all()
    assert int(order[0]) == int(m["first"][0])
    d = m["dots"]
    assert want["splat"][5, 2] == NONE and e.covered[5, 2] and want["splat"][5, 6] == d[2] and want["splat"][5, 10] == d[4]
    assert e.covered[ly0:ly0 + 8, lx0:lx0 + 8].all() and (e.covered & ~e.crossed).sum() >= 8
    r = new_renderer(gpu_ctx, sc.asset, blend, tile=tile)
    rt = pick_target(gpu_ctx, sc.W, sc.H)
    got = draw(r, sc.cam, rt)
    assert tile_of(r) == tile
    assert_exact(got, want, (sc.name, blend))
    r.OnDisable(); rt.Dispose()


# ---- 7. clear, two objects, scene depth ---------------------------------------------------------------------------------------------------------------------
def test_a_clear_resets_the_records_of_tiles_the_next_draw_leaves_empty(gpu_ctx):
    sc = crafted_scene((16, 16))
    m = sc.meta
    r = new_renderer(gpu_ctx, sc.asset, 0, tile=(16, 16))
    rt = pick_target(gpu_ctx, sc.W, sc.H)
    full = draw(r, sc.cam, rt)
    assert (full["splat"][16:32, 16:32] != NONE).all()
    keep = np.zeros(sc.asset.splatCount, bool)
    keep[m["dots"]] = True                                         # only tile (0, 0) keeps a list
    r.SetDeletedBits(EM.pack_bits(~keep, (sc.asset.splatCount + 31) // 32))
    got = draw(r, sc.cam, rt)
    orc, P = oracle_of(sc, deleted_bits=EM.pack_bits(~keep, (sc.asset.splatCount + 31) // 32))
    e = PM.expected(orc, P, 0, (0.5,))[0.5]
    assert not e.ambiguous.any() and e.crossed.sum() == 2
    assert_exact(got, e.records, "after the clear")
    rt.Clear()                                                     # ... and a clear that no draw folds in
    assert same_records(rt.DownloadPick(), PM.none_records(sc.H, sc.W))
    r.OnDisable(); rt.Dispose()


@functools.lru_cache(maxsize=None)
def two_object_scenes():
    """A (tag 1): a square on (12, 12) and a dot of 0.3 on pixel (26, 10).  B (tag 2), behind A: squares on (12, 12), (28, 12) and (12, 28)."""
    W, H = 48, 40
    a = K.Builder(W, H)
    a.add(12.0, 12.0, 3.0, K.SQUARE_SIGMA, K.SQUARE_SIGMA * 1.02, (0.9, 0.2, 0.1), K.SQUARE_OPACITY)
    a.add(26.5, 10.5, 3.1, K.DOT_SIGMA[0], K.DOT_SIGMA[1], (0.2, 0.9, 0.1), BIG_DOT)
    b = K.Builder(W, H)
    b.add([12.0, 28.0, 12.0], [12.0, 12.0, 28.0], [5.0, 5.1, 5.2], K.SQUARE_SIGMA, K.SQUARE_SIGMA * 1.02, (0.1, 0.3, 0.9), K.SQUARE_OPACITY)
    return K.Scene("two_a", W, H, a.build(), {}), K.Scene("two_b", W, H, b.build(), {})


@pytest.mark.parametrize("blend", [0, 1], ids=["exact", "fast"])
def test_two_renderers_share_a_target_by_their_tags(gpu_ctx, blend):
    sa, sb = two_object_scenes()
    ra, rb = new_renderer(gpu_ctx, sa.asset, blend, tag=1), new_renderer(gpu_ctx, sb.asset, blend)
    rb.SetPickTag(2)
    rt = pick_target(gpu_ctx, sa.W, sa.H)
    first = draw(ra, sa.cam, rt)
    pixels_a = rt.Download()
    got = draw(rb, sb.cam, rt, clear=False)
    oa, Pa = oracle_of(sa)
    ea = PM.expected(oa, Pa, blend, (0.5,), tag=1)[0.5]
    assert_exact(first, ea.records, "object A")
    ob, Pb = oracle_of(sb)
    eb = PM.expected(ob, Pb, blend, (0.5,), tag=2, start=pixels_a, start_records=ea.records)[0.5]
    assert not ea.ambiguous.any() and not eb.ambiguous.any()
    assert_exact(got, eb.records, "object B onto A")
    # ... and stated without the oracle: A's square keeps its record, the pixel A left at 0.3 and B's own squares carry B's tag
    assert (got["tag"][8:16, 8:16] == 1).all() and (got["splat"][8:16, 8:16] == 0).all()
    assert tuple(got[10, 26])[1:3] == (1, 2) and first["splat"][10, 26] == NONE
    assert (got["tag"][24:32, 8:16] == 2).all() and (got["splat"][24:32, 8:16] == 2).all()
    ra.OnDisable(); rb.OnDisable(); rt.Dispose()


def test_scene_depth_in_front_of_the_crossing_splat(gpu_ctx):
    """Index order IS the draw order here (no sort): the far square (depth 5) is drawn before the near one (depth 3).  Without a depth attachment the far
    one crosses; behind a scene depth of 4 it is discarded and the near one -- the next survivor -- is recorded; behind one of 2 nothing is."""
    W, H = 32, 24
    b = K.Builder(W, H)
    b.add([12.0, 12.0], [12.0, 12.0], [5.0, 3.0], K.SQUARE_SIGMA, K.SQUARE_SIGMA * 1.02, [(0.9, 0.2, 0.1), (0.1, 0.3, 0.9)], K.SQUARE_OPACITY)
    sc = K.Scene("depth", W, H, b.build(), {})
    depth = np.full((H, W), 100.0, np.float32)
    depth[:, 10:14] = 4.0
    depth[:, 14:] = 2.0
    r = new_renderer(gpu_ctx, sc.asset, 0)
    rt = pick_target(gpu_ctx, W, H)
    rt.SetSceneDepth(depth)
    got = draw(r, sc.cam, rt, sort=False)
    orc, P = oracle_of(sc, sort=False)
    e = PM.expected(orc, P, 0, (0.5,), scene_depth=depth)[0.5]
    assert not e.ambiguous.any()
    assert_exact(got, e.records, "scene depth")
    assert (got["splat"][8:16, 8:10] == 0).all() and (got["splat"][8:16, 10:14] == 1).all() and (got["splat"][8:16, 14:16] == NONE).all()
    assert (got["depth"][8:16, 10:14] < 4.0).all() and (got["depth"][8:16, 8:10] > 4.0).all()
    r.OnDisable(); rt.Dispose()


# ---- 8. highlight, deleted and cut splats ---------------------------------------------------------------------------------------------------------------------
def test_the_crossing_follows_the_highlight_s_raised_opacity(gpu_ctx):
    """One soft splat of opacity 0.2, centred on a pixel centre: unselected it never reaches tau = 0.6.  Selected and highlighted its fragments blend
    saturate(e + 0.3) where e = exp(-|q|^2) > 7/255 (1.0 on the ring 7/255 < e < 10/255): crossed exactly where e >= 0.3 or on the ring.  The expectation is
    that formula over the splat's stated geometry (lambda = sigma^2 + 0.3 per axis, q = d / sqrt(2 lambda)), with a margin around each threshold."""
    W, H, tau = 48, 40, 0.6
    cx, cy, sx, sy = 24.5, 20.5, 5.0, 4.0
    b = K.Builder(W, H)
    s = b.add(cx, cy, 5.0, sx, sy, (0.3, 0.6, 0.9), 0.2)
    sc = K.Scene("hl", W, H, b.build(), {})
    yy, xx = np.mgrid[0:H, 0:W]
    q2x, q2y = (xx + 0.5 - cx) ** 2 / (2 * (sx * sx + 0.3)), (yy + 0.5 - cy) ** 2 / (2 * (sy * sy + 0.3))
    e = np.exp(-(q2x + q2y))
    in_quad = (q2x <= 4.0 * 0.95) & (q2y <= 4.0 * 0.95)
    must = in_quad & (e > 0.33)
    never = (e < 0.27) & (e > 11.5 / 255) | (e < 6.0 / 255) | (q2x > 4.0 * 1.05) | (q2y > 4.0 * 1.05)
    ring = in_quad & (e > 7.6 / 255) & (e < 9.4 / 255)
    assert must.sum() > 50 and ring.sum() > 20 and (never & in_quad).sum() > 100
    r = new_renderer(gpu_ctx, sc.asset, 0, highlight=True)
    rt = pick_target(gpu_ctx, W, H, tau)
    plain = draw(r, sc.cam, rt)
    assert same_records(plain, PM.none_records(H, W)), "unselected, opacity 0.2 never reaches 0.6"
    r.UploadSelectedBits(EM.pack_bits(np.array([True]), 1))
    for blend in (0, 1):
        r.blendMode = blend
        got = draw(r, sc.cam, rt)
        assert (got["splat"][must | ring] == s[0]).all() and (got["splat"][never] == NONE).all(), blend
        w = r.DownloadView()["pos"][:, 3]
        assert PM.consistent(got, w, 1).all()
    r.OnDisable(); rt.Dispose()


def test_deleted_and_cut_splats_are_never_recorded(gpu_ctx):
    sc = PM.SCENES[0]
    orc0, P, exp = PM.scene_expected(sc.name, 0)
    n = sc.asset.splatCount
    seen = np.unique(exp[0.5].records["splat"][exp[0.5].crossed])
    deleted = np.zeros(n, bool)
    deleted[seen[::2]] = True                                      # half the splats the surface is made of
    words = EM.pack_bits(deleted, (n + 31) // 32)
    cuts = EM.cutout_lists()["ellipsoid"]
    r = new_renderer(gpu_ctx, sc.asset, 0, opacity=sc.opacity_scale)
    r.SetDeletedBits(words)
    r.m_Cutouts = cuts
    rt = pick_target(gpu_ctx, sc.W, sc.H)
    got = draw(r, sc.cam, rt)
    model = EM.EditModel(sc.asset)
    model.set_cutouts(cuts, r.transform.localToWorldMatrix)
    assert model.cut.sum() > 100 and (~model.cut).sum() > 100
    orc = O.Oracle(sc.asset)
    orc.sort(camera.sort_matrix(sc.cam, r.transform.localToWorldMatrix))
    arr, cnt = shader_data_array(cuts, r.transform.localToWorldMatrix)
    orc.calc_view(P, arr, cnt, deleted_bits=words)
    e = PM.expected(orc, P, 0, (0.5,))[0.5]
    PM.check_records(got, e, orc0.view["pos"][:, 3], n, "deleted + cut")
    named = got["splat"][got["splat"] != NONE]
    assert len(named) > 200 and not deleted[named].any() and not model.cut[named].any()
    r.OnDisable(); rt.Dispose()


# ---- 9. EditSelectSurface ------------------------------------------------------------------------------------------------------------------------------------
def test_edit_select_surface_against_the_numpy_twin(gpu_ctx):
    sc = PM.SCENES[0]
    n = sc.asset.splatCount
    r = new_renderer(gpu_ctx, sc.asset, 0, tag=5, opacity=sc.opacity_scale)
    rt = pick_target(gpu_ctx, sc.W, sc.H)
    rec = draw(r, sc.cam, rt)
    assert (rec["tag"][rec["splat"] != NONE] == 5).all()
    model = EM.EditModel(sc.asset)
    model._ensure()

    def step(rect, subtract, what, tag=5):
        r.EditSelectSurface(rt, rect, subtract)
        model.sel = PM.select_surface(rec, model.sel, rect, tag, n, deleted=model.deleted, cut=model.cut, subtract=subtract)
        sel = r.DownloadEditBits()[0]
        assert np.array_equal(sel, model.sel), (what, np.flatnonzero(sel != model.sel)[:8])
        assert np.array_equal(EM.info_words(edit_info(r)), model.info()), what
        assert r.editSelectedSplats == int(model.info()[0]), what
        return EM.popcount(model.sel)

    a = step((10, 8, 40, 30), False, "rectangle")
    assert a > 50
    y, x = np.argwhere(rec["splat"] != NONE)[-1]
    b = step((int(x), int(y), int(x), int(y)), False, "click")
    assert b in (a, a + 1) and (model.sel[int(rec["splat"][y, x]) >> 5] >> (int(rec["splat"][y, x]) & 31)) & 1
    c = step((20, 12, 30, 20), True, "subtract")
    assert c < b
    d = step((-20, -7, 12, 9), False, "partly outside")
    assert d > c
    assert step((sc.W, 0, sc.W + 9, 5), False, "wholly outside") == d
    r.SetPickTag(6)                                                # the records carry 5: nothing of the target is this renderer's any more
    assert step((0, 0, sc.W - 1, sc.H - 1), False, "tag mismatch", tag=6) == d
    r.SetPickTag(5)
    # a splat deleted after the draw is skipped: delete what is selected, deselect, select the whole target
    r.EditDeleteSelected(); model.delete_selected()
    e = step((0, 0, sc.W - 1, sc.H - 1), False, "after a delete")
    assert 0 < e and not (model.sel & model.deleted).any() and int(model.info()[1]) == d
    r.OnDisable(); rt.Dispose()


# ---- 10. refusals leave the state untouched ---------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx):
    sc = PM.SCENES[1]
    lib = _lib.lib()
    r = new_renderer(gpu_ctx, sc.asset, 0, opacity=sc.opacity_scale)
    rt = pick_target(gpu_ctx, sc.W, sc.H, 0.95)
    want = draw(r, sc.cam, rt)
    pixels = rt.Download()
    for bad in (0.0, float("nan"), 1.0 + 2.0 ** -20, -0.5, float("inf")):
        assert lib.gs_target_set_pick_output(rt._h, 1, C.c_float(bad)) == BAD, bad
    assert same_records(draw(r, sc.cam, rt), want), "a refused threshold changed the threshold or the records"
    for mode in (RenderMode.DebugPoints, RenderMode.DebugPointIndices, RenderMode.DebugBoxes, RenderMode.DebugChunkBounds):
        r.m_RenderMode = mode
        with pytest.raises(GsError) as ex:
            r.Draw(sc.cam, rt)
        assert ex.value.code == BAD, mode
    r.m_RenderMode = RenderMode.Splats
    assert same_records(rt.DownloadPick(), want) and np.array_equal(rt.Download(), pixels), "a refused debug draw touched the target"
    buf = np.zeros(sc.W * sc.H * 16, np.uint8)
    assert lib.gs_target_download_pick(rt._h, _p(buf), C.c_size_t(buf.nbytes - 16)) == BAD and not buf.any()
    rec = _abi.gs_pick_record(1.0, 2, 3, 4)
    for x, y in ((sc.W, 0), (0, sc.H), (2 ** 32 - 1, 0)):
        assert lib.gs_target_pick_at(rt._h, C.c_uint32(x), C.c_uint32(y), C.byref(rec)) == BAD
    assert (rec.depth, rec.splat, rec.tag, rec.zero) == (1.0, 2, 3, 4)
    with pytest.raises(GsError):
        rt.PickAt(-1, 0)
    off = RenderTarget(gpu_ctx, sc.W, sc.H)                         # a target without pick output has no records to hand out
    assert lib.gs_target_download_pick(off._h, _p(buf), C.c_size_t(buf.nbytes)) == BAD
    assert lib.gs_renderer_edit_select_surface(r._r_h, off._h, 0, 0, 1, 1, 0) == BAD
    assert lib.gs_renderer_edit_select_surface(r._r_h, rt._h, 5, 0, 4, 1, 0) == BAD
    ptr = C.c_void_p()
    assert lib.gs_target_pick_device_ptr(off._h, C.byref(ptr)) == BAD and not ptr.value
    _lib.check(lib.gs_target_pick_device_ptr(rt._h, C.byref(ptr)), "gs_target_pick_device_ptr")
    assert ptr.value
    assert same_records(rt.DownloadPick(), want)
    rt.SetPickOutput(False)
    assert lib.gs_target_download_pick(rt._h, _p(buf), C.c_size_t(buf.nbytes)) == BAD
    rt.SetPickOutput(True, 1.0)                                     # 1.0 itself is a threshold; the records start as "none"
    assert same_records(rt.DownloadPick(), PM.none_records(sc.H, sc.W))
    off.Dispose(); r.OnDisable(); rt.Dispose()
