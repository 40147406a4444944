"""What the -m gpu suites share to drive a renderer (helper, not a test): making one, drawing frames and comparing them, downloading its state and
holding it to the models, baking against the yardstick, and the lock-step rig of the edit suites.  Imports without a GPU; nothing here makes a context."""
import ctypes as C

import numpy as np

import bake_model as BM
import copy_model as CM
import edit_model as EM
import oracle_lib as O
from builders import CAMS
from common import RT_TOL, rt_err, views_equal
from unitygaussiansplatting_amd import _abi, _lib, asset as A, camera, creator
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget, SortMode

f32 = np.float32
BAD = _abi.GS_ERR_INVALID_ARGUMENT
CAM = CAMS[0]                                                      # default_camera(az=25.0)


# ---- renderers ------------------------------------------------------------------------------------------------------------------------------------
def make_renderer(ctx, asset, tr=None, mode=None, frames=None) -> GaussianSplatRenderer:
    """a renderer with its resources; mode / frames None: what the host layer's defaults (and its environment) say"""
    r = GaussianSplatRenderer(ctx, asset, tr)
    if mode is not None:
        r.sortMode = mode
    if frames is not None:
        r.framesInFlight = frames
    r.CreateResourcesForAsset()
    return r


def pinned_renderer(ctx, asset, tr=None, mode=SortMode.Full, frames=1) -> GaussianSplatRenderer:
    """the form of the edit suites: the sort mode and the frames in flight are the test's, whatever the environment says"""
    return make_renderer(ctx, asset, tr, mode, frames)


def fptr(v):
    a = np.ascontiguousarray(v, f32).reshape(-1)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def native_count(r) -> int:
    n = C.c_uint32(0)
    _lib.check(_lib.lib().gs_renderer_splat_count(r._r_h, C.byref(n)), "gs_renderer_splat_count")
    return int(n.value)


def edit_info(r) -> _abi.gs_edit_info:
    info = _abi.gs_edit_info()
    _lib.check(_lib.lib().gs_renderer_edit_info(r._r_h, C.byref(info)), "gs_renderer_edit_info")
    return info


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------------
def draw_frame(r, cam, rt) -> None:
    r.SortPoints(cam); r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)


def frame_of(r, ctx, cam=CAM):
    rt = RenderTarget(ctx, cam.pixelWidth, cam.pixelHeight)
    draw_frame(r, cam, rt)
    out = (r.DownloadOrder(), r.DownloadView(), rt.Download())
    rt.Dispose()
    return out


def same_frame(a, b) -> bool:
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8)) and np.array_equal(a[2], b[2])


def frames_of(r, ctx, cams=CAMS):
    """SortPoints / CalcViewData / Draw on every camera: [(view records, frame)] and the order buffer at the end"""
    out = []
    for cam in cams:
        rt = RenderTarget(ctx, cam.pixelWidth, cam.pixelHeight)
        draw_frame(r, cam, rt)
        out.append((r.DownloadView(), rt.Download()))
        rt.Dispose()
    return out, r.DownloadOrder()


def oracle_frames(asset, words, tr, cams=CAMS):
    orc = O.Oracle(asset)
    probe = GaussianSplatRenderer.__new__(GaussianSplatRenderer)   # no context: FrameParams reads the transform and the serialized fields only
    probe.transform, probe.m_SplatScale, probe.m_OpacityScale, probe.m_SHOrder, probe.m_SHOnly = tr, 1.0, 1.0, 3, False
    out = []
    for cam in cams:
        orc.sort(camera.sort_matrix(cam, tr.localToWorldMatrix))
        P = probe.FrameParams(cam)
        view = orc.calc_view(P, deleted_bits=words).copy()
        out.append((view, orc.draw(P, 0)))
    return out, orc.order.copy()


def assert_same_frames(got, want, what, bits=True):
    (gf, go), (wf, wo) = got, want
    assert np.array_equal(go, wo), (what, "order")
    for k, ((gv, gi), (wv, wi)) in enumerate(zip(gf, wf)):
        if bits:
            assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)) or views_equal(gv, wv), (what, k, "view")
            assert np.array_equal(gi, wi), (what, k, "frame", int((gi != wi).sum()))
        else:
            assert views_equal(gv, wv), (what, k, "view vs oracle")
            e = rt_err(gi, wi)
            print(what, "camera", k, "rt_err vs oracle", e)
            assert e <= RT_TOL, (what, k, e)


def check_raster_records(r, orc, P):
    """rec / rect / visibility of the PER-FRAME calc_view launch (FULL = false: early cull, chunk cull, colour only for visible
    splats) against the oracle's prepare() -- the view-parity tests only ever read the on-demand full kernel."""
    recs, rects, vis = r.DownloadRasterRecords()
    orecs, orects, ovis = orc.raster_records(P)
    assert np.array_equal(vis, ovis), "visibility bits differ"
    assert np.array_equal(rects, orects), "tile rectangles differ"
    m = (np.unpackbits(ovis.view(np.uint8), bitorder="little")[:orc.n]).astype(bool)
    assert np.array_equal(recs[m], orecs[m]), "blend records of visible splats differ"
    return int(m.sum())


# ---- the renderer's state against the copy model ----------------------------------------------------------------------------------------------------
def download(r) -> CM.Blobs:
    pos, other, color, sh = r.DownloadSplatData()
    return CM.Blobs(r.splatCount, pos, other, color, sh, r.DownloadEditBits()[2])


def check_state(r, want: CM.Blobs, what, tails=None, selected=None, order=None):
    """everything the renderer holds against the model.  tails: the bytes an unresized renderer's blobs carry behind whole records (the asset's)"""
    assert native_count(r) == want.n == r.splatCount, what
    got = download(r)
    for k, name in enumerate(("pos", "other", "color", "sh")):
        g, w = getattr(got, name), getattr(want, name)
        tail = b"" if tails is None else tails[k]
        assert len(g) == len(w) + len(tail), (what, name, len(g), len(w))
        assert np.array_equal(g[:len(w)], w), (what, name, np.flatnonzero(g[:len(w)] != w)[:8])
        assert g[len(w):].tobytes() == tail, (what, name, "tail")
    sel, md, deleted = r.DownloadEditBits()
    assert np.array_equal(deleted, want.deleted_words()), (what, "deleted", deleted, want.deleted_words())
    zeros = np.zeros(want.words, np.uint32)
    assert np.array_equal(sel, zeros if selected is None else selected[0]) and np.array_equal(md, zeros if selected is None else selected[1]), (what, "selection")
    if order is not None:
        assert np.array_equal(r.DownloadOrder(), order), (what, "order")
    return got


def asset_tails(asset):
    n = asset.splatCount
    w, h = A.CalcTextureSize(n)
    sizes = (12 * n, 16 * n, w * h * 16, 192 * n)
    return [np.ascontiguousarray(b, np.uint8)[s:].tobytes() for b, s in zip((asset.posData, asset.otherData, asset.colorData, asset.shData), sizes)]


# ---- the bake against the yardstick -------------------------------------------------------------------------------------------------------------------
def bake(r, formats, morton=True):
    fp, fs, fc, fsh = formats
    return r.EditBakeAsset(formatPos=fp, formatScale=fs, formatColor=fc, formatSH=fsh, morton=morton)


def yardstick(dec_alive, formats, morton=True, ctx=None) -> A.GaussianSplatAsset:
    """the yardstick of a Cluster* SH target: the native importer (ctx: its assignment passes on the GPU) over finite input free of -0"""
    raw = BM.columns(dec_alive)
    BM.assert_no_negative_zero(raw)
    assert all(np.isfinite(np.asarray(c)).all() for c in (raw.pos, raw.scale, raw.dc0, raw.opacity, raw.sh, raw.rot)), "a yardstick input is not finite"
    fp, fs, fc, fsh = formats
    return creator.CreateAssetFromSplatsNative(raw, formatPos=fp, formatScale=fs, formatColor=fc, formatSH=fsh, linearize=False, morton=morton, name="yardstick",
                                               context=ctx)


def check_bake(r, dec_alive, formats, what, morton=True, want=None):
    """one bake against the yardstick (want: one made otherwise than by bake_model); returns the yardstick asset"""
    want = BM.yardstick(dec_alive, formats, morton) if want is None else want
    g = bake(r, formats, morton)
    try:
        assert g.splatCount == len(dec_alive), (what, g.splatCount, len(dec_alive))
        BM.assert_same_asset(g.Download(), want, what)
    finally:
        g.Dispose()
    return want


def keep_only(r, n: int, src: np.ndarray) -> None:
    """deleted bits that leave exactly the splats `src` alive"""
    flags = np.ones(n, bool)
    flags[src] = False
    r.SetDeletedBits(EM.pack_bits(flags, (n + 31) // 32))


# ---- the lock-step rig of the edit suites ---------------------------------------------------------------------------------------------------------------
class Rig:
    """one renderer and the model of its edit state, moved in lock step; every step ends with the comparison"""

    def __init__(self, ctx, asset, transform=None):
        self.r = GaussianSplatRenderer(ctx, asset, transform)
        self.r.CreateResourcesForAsset()
        self.m = EM.EditModel(asset)
        self.lib = _lib.lib()
        self.steps = 0
        self.check("fresh")

    def close(self):
        self.r.DisposeResourcesForAsset()

    def raw_info(self) -> np.ndarray:
        return EM.info_words(edit_info(self.r))

    def check(self, what):
        self.steps += 1
        got, want = self.r.DownloadEditBits(), self.m.bits()
        for name, g, w in zip(("selected", "mouse-down", "deleted"), got, want):
            assert np.array_equal(g, w), f"step {self.steps} ({what}): {name} words differ at {np.flatnonzero(g != w)[:8]}"
        gi, wi = self.raw_info(), self.m.info()
        assert np.array_equal(gi, wi), f"step {self.steps} ({what}): info {gi.tolist()} != {wi.tolist()}"
        r = self.r
        if r.m_GpuEditSelected:                                    # the host mirror's fields are that record decoded (UpdateEditCountsAndBounds)
            r.UpdateEditCountsAndBounds()
            mirror = (r.editSelectedSplats, r.editDeletedSplats, r.editCutSplats)
            assert mirror == tuple(int(v) for v in wi[:3]), f"step {self.steps} ({what}): the host mirror's counts {mirror} != info {wi[:3].tolist()}"

    # -- the calls, on both sides ---------------------------------------------------------------------------------------------------------
    def select_all(self):
        self.r.EditSelectAll(); self.m.select_all(); self.check("select all")

    def deselect_all(self):
        self.r.EditDeselectAll(); self.m.deselect_all(); self.check("deselect all")

    def invert(self):
        self.r.EditInvertSelection(); self.m.invert_selection(); self.check("invert")

    def store(self):
        self.r.EditStoreSelectionMouseDown(); self.m.store_selection(); self.check("store")

    def update(self, cam, rect, subtract):
        x0, y0, x1, y1 = rect
        self.r.EditUpdateSelection((x0, y1), (x1, y0), cam, subtract)      # rectMin = (x_min, y_max), rectMax = (x_max, y_min): GaussianSplatRenderer.cs:835
        self.m.update_selection(self.r.FrameParams(cam), rect, subtract)
        self.check(f"update {rect} subtract={subtract}")

    def delete(self):
        self.r.EditDeleteSelected(); self.m.delete_selected(); self.check("delete")
        if self.m.info()[1] != 0:
            assert self.r.editModified, f"step {self.steps} (delete): {self.m.info()[1]} splats deleted and editModified is {self.r.editModified}"      # GaussianSplatRenderer.cs:902-903

    def upload_selected(self, words):
        self.r.UploadSelectedBits(words); self.m.upload_selected(words); self.check("upload selected")

    def set_cutouts(self, cuts):
        self.r.m_Cutouts = cuts
        self.r.UpdateCutoutsBuffer()
        self.m.set_cutouts(cuts, self.r.transform.localToWorldMatrix)
        self.check("set cutouts")

    def set_deleted_bits(self, words):
        self.r.SetDeletedBits(words); self.m.set_deleted_bits(words); self.check("set deleted bits")

    def release(self):
        _lib.check(self.lib.gs_renderer_edit_release(self.r._r_h), "gs_renderer_edit_release")
        self.r.m_GpuEditSelected = False
        self.m.release()
        self.check("release")
