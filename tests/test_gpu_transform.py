"""Moving, rotating and scaling the selection on the GPU (csrc/gs_edit.hip's transform kernels through the gs_renderer_edit_* calls and
GaussianSplatRenderer.Edit*) against the numpy model of the reference's three kernels (tests/transform_model.py; its premises and its codec are asserted
on the CPU by tests/test_transform_model.py).  After EVERY call the renderer's current pos / other blobs (DownloadPosOther: every byte, a NaN position
equal to a NaN), the three bit buffers and the nine words of gs_renderer_edit_info are compared with the model."""
import numpy as np
import pytest

import edit_model as EM
import export_model as XM
import oracle_lib as O
import transform_model as TM
from builders import TOOL, pos_only_asset
from common import RT_TOL, default_camera, rt_err, small_asset, views_equal
from gpu_rig import BAD, Rig, draw_frame, fptr
from unitygaussiansplatting_amd import _lib, camera
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget, SortMode
from vissort_model import visible_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
CENTRE = (0.3, -0.2, 0.1)
Q1 = (0.18257419, 0.36514837, 0.54772256, 0.73029674)
Q2 = (-0.5, 0.5, 0.5, 0.5)


class TRig(Rig):
    """gpu_rig.Rig over a TransformModel: the blobs are part of every comparison"""

    def __init__(self, ctx, asset, transform=None, sort_mode=None):
        self.r = GaussianSplatRenderer(ctx, asset, transform)
        if sort_mode is not None:
            self.r.sortMode = sort_mode
        self.r.CreateResourcesForAsset()
        self.m = TM.TransformModel(asset)
        self.lib = _lib.lib()
        self.steps = 0
        self.check("fresh")

    def check(self, what):
        super().check(what)
        pos, other = self.r.DownloadPosOther()
        wp, wo = self.m.blobs()
        assert TM.blobs_equal(pos, wp, floats=self.m.pos_gate), f"step {self.steps} ({what}): pos differs at bytes {np.flatnonzero(pos != wp)[:8]}"
        assert TM.blobs_equal(other, wo, floats=False), f"step {self.steps} ({what}): other differs at bytes {np.flatnonzero(other != wo)[:8]}"

    def store_pos_other(self):
        self.r.EditStorePosMouseDown(); self.r.EditStoreOtherMouseDown()
        self.m.store_pos(); self.m.store_other()
        self.check("store pos / other")

    def translate(self, d):
        self.r.EditTranslateSelection(d)
        assert self.m.translate(d) and self.r.editModified
        self.check(f"translate {d}")

    def rotate(self, q, tr=TOOL, centre=CENTRE):
        self.r.EditRotateSelection(centre, tr.localToWorldMatrix, tr.worldToLocalMatrix, q)
        assert self.m.rotate(centre, tr.localToWorldMatrix, tr.worldToLocalMatrix, q)
        self.check(f"rotate {q}")

    def scale(self, s, tr=TOOL, centre=CENTRE):
        self.r.EditScaleSelection(centre, tr.localToWorldMatrix, tr.worldToLocalMatrix, s)
        assert self.m.scale(centre, tr.localToWorldMatrix, tr.worldToLocalMatrix, s)
        self.check(f"scale {s}")

    def release(self):
        super().release()
        self.r.m_GpuEditPosMouseDown = self.r.m_GpuEditOtherMouseDown = False

    # the raw calls, for their return codes
    def c_rotate(self, q=Q1):
        (_, c), (_, a), (_, b), (_, r) = fptr(CENTRE), fptr(TOOL.localToWorldMatrix), fptr(TOOL.worldToLocalMatrix), fptr(q)
        return self.lib.gs_renderer_edit_rotate_selection(self.r._r_h, c, a, b, r)

    def c_scale(self, s=(2.0, 2.0, 2.0)):
        (_, c), (_, a), (_, b), (_, v) = fptr(CENTRE), fptr(TOOL.localToWorldMatrix), fptr(TOOL.worldToLocalMatrix), fptr(s)
        return self.lib.gs_renderer_edit_scale_selection(self.r._r_h, c, a, b, v)

    def c_translate(self, d=(0.5, 0.25, -1.0)):
        return self.lib.gs_renderer_edit_translate_selection(self.r._r_h, fptr(d)[1])


def drag(rig: TRig):
    """translate; mouse down; rotate; rotate again from the same mouse-down state; scale (a negative and a zero component); translate again"""
    rig.translate((0.25, -0.5, 0.125))
    rig.store_pos_other()
    rig.rotate(Q1)
    first = rig.m.pos_blob.copy()
    rig.rotate(Q2)
    if rig.m.pos_gate and rig.m.selected().any():
        assert not np.array_equal(first, rig.m.pos_blob)           # the result depends on the last call only (the model reads the mouse-down copy)
    rig.scale((1.5, -0.5, 0.0))
    rig.translate((-1.0, 0.0, 2.0e-3))


def wave_kinds(words, n):
    """(a wave -- 64 splats, two words -- without a selected bit exists, a wave with some but not all of its splats selected exists)"""
    sel = EM.unpack_bits(words, n)
    empty = mixed = False
    for w0 in range(0, n, 64):
        s = sel[w0:w0 + 64]
        empty |= not s.any()
        mixed |= bool(s.any() and not s.all())
    return empty, mixed


# ---- 1. sizes and selections at the seams of the kernel shape ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513])
def test_seams(gpu_ctx, n):
    rig = TRig(gpu_ctx, EM.point_asset(n))
    nw = rig.m.nw
    selections = [("none", np.zeros(nw, np.uint32))]
    for bit in sorted({b for b in (0, 31, 32, 63, 64, n - 1) if b < n}):
        flags = np.zeros(n, bool); flags[bit] = True
        selections.append((f"bit {bit}", EM.pack_bits(flags, nw)))
    alt = np.zeros(nw, np.uint32); alt[0::2] = 0xFFFFFFFF
    selections.append(("alternating words", alt))
    selections.append(("random half", EM.pack_bits(np.random.default_rng(n).random(n) < 0.5, nw)))
    empty = mixed = False
    for name, words in selections:
        rig.upload_selected(words)
        e, m = wave_kinds(words, n)
        empty |= e and bool(words.any()); mixed |= m
        drag(rig)
    rig.select_all()                                               # tail bits set: nothing at >= N is written (the blobs hold N records, compared to the byte)
    if n % 32:
        assert EM.popcount(rig.m.bits()[0]) > n
    drag(rig)
    if n >= 255:
        assert empty and mixed                                     # premise: some launch had a wave that left early, and one with both kinds of lanes
    rig.close()


# ---- 2. the format gates, and the mouse-down copies --------------------------------------------------------------------------------------
def test_a_chunked_asset_is_left_alone(gpu_ctx):
    a = small_asset(257, 5, "Medium")
    rig = TRig(gpu_ctx, a)
    assert not rig.m.pos_gate and not rig.m.rot_gate
    rig.select_all()
    rig.store_pos_other()
    assert rig.c_translate() == 0 and rig.c_rotate() == 0 and rig.c_scale() == 0
    rig.m.translate((0, 0, 0))
    rig.check("after the three calls")
    pos, other = rig.r.DownloadPosOther()
    assert np.array_equal(pos, a.posData) and np.array_equal(other, a.otherData)
    drag(rig)                                                      # through the Python methods too
    rig.close()


def test_rotate_with_only_the_position_gate(gpu_ctx):
    a = pos_only_asset(257)
    rig = TRig(gpu_ctx, a)
    assert rig.m.pos_gate and not rig.m.rot_gate
    rig.upload_selected(EM.pack_bits(np.random.default_rng(3).random(257) < 0.5, rig.m.nw))
    before = rig.m.pos_blob.copy()
    drag(rig)
    pos, other = rig.r.DownloadPosOther()
    assert np.array_equal(other, a.otherData) and not np.array_equal(pos, before)
    rig.close()


def test_rotate_and_scale_need_the_mouse_down_copies(gpu_ctx):
    rig = TRig(gpu_ctx, EM.point_asset(257))
    rig.select_all()
    assert rig.c_rotate() == BAD and b"mouse-down" in rig.lib.gs_last_error_string()
    assert rig.c_scale() == BAD
    rig.r.EditRotateSelection(CENTRE, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, Q1)      # the Python methods return silently, like the C#
    rig.r.EditScaleSelection(CENTRE, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, (2.0, 2.0, 2.0))
    rig.check("refused")
    rig.r.EditStorePosMouseDown(); rig.m.store_pos()
    assert rig.c_rotate() == BAD                                   # both copies
    rig.check("still refused")
    rig.scale((2.0, 0.5, 1.0))
    rig.store_pos_other()
    rig.rotate(Q1)
    moved = rig.m.pos_blob.copy()
    rig.release()
    assert rig.c_rotate() == BAD and rig.c_scale() == BAD
    rig.m._ensure()                                                # (the refused calls made the selection buffers again: EnsureEditingBuffers comes first)
    rig.r.m_GpuEditSelected = True
    rig.check("after the release")
    assert np.array_equal(rig.r.DownloadPosOther()[0], moved)      # the private blobs are the renderer's data now
    rig.close()


# ---- 3. the asset and other renderers never see an edit ----------------------------------------------------------------------------------------
def _frame(r, cam, rt):
    draw_frame(r, cam, rt)
    return rt.Download()


def test_other_renderers_over_the_asset_are_untouched(gpu_ctx):
    a = scene_asset(3000)
    rig = TRig(gpu_ctx, a)
    cam = default_camera()
    other = GaussianSplatRenderer(gpu_ctx, a)
    other.ShareResourcesOf(rig.r)
    rt = RenderTarget(gpu_ctx, 320, 200)
    before = _frame(other, cam, rt)
    mine_before = _frame(rig.r, cam, rt)
    rig.update(cam, EM.PREMISE_RECT, False)
    assert rig.m.info()[0] > 100
    drag(rig)
    pos, oth = other.DownloadPosOther()
    assert np.array_equal(pos, a.posData) and np.array_equal(oth, a.otherData)
    assert np.array_equal(_frame(other, cam, rt), before)
    assert rt_err(_frame(rig.r, cam, rt), mine_before) > 16 * RT_TOL      # (the move is visible on the renderer that made it)
    late = GaussianSplatRenderer(gpu_ctx, a)
    late.ShareResourcesOf(rig.r)
    pos, oth = late.DownloadPosOther()
    assert np.array_equal(pos, a.posData) and np.array_equal(oth, a.otherData)
    assert np.array_equal(_frame(late, cam, rt), before)
    late.DisposeResourcesForAsset(); other.DisposeResourcesForAsset()
    rt.Dispose(); rig.close()


# ---- 4. frames after a move --------------------------------------------------------------------------------------------------------------------
def scene_asset(n, seed=21):
    """a small all-fp32, chunk-less scene with real footprints: seeded positions, anisotropic scales, rotations, colours, opacities"""
    import crafted
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) * 4.0 - 2.0).astype(f32)
    scale = rng.uniform(0.02, 0.09, (n, 3)).astype(f32)
    return crafted.asset(pos, scale, rot=rng.standard_normal((n, 4)), rgb=rng.random((n, 3)), opacity=rng.uniform(0.3, 1.0, n))


@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("mode", [SortMode.Full, SortMode.Visible])
def test_frames_after_a_move(gpu_ctx, mode, blend):
    a = scene_asset(3000)
    rig = TRig(gpu_ctx, a, sort_mode=mode)
    r = rig.r
    r.blendMode = blend
    cam0, cam1 = default_camera(), default_camera(az=70.0, elev=-15.0)
    rt = RenderTarget(gpu_ctx, 320, 200)
    old = O.Oracle(a)
    old.sort(camera.sort_matrix(cam0, r.transform.localToWorldMatrix))
    before = _frame(r, cam0, rt)
    rig.update(cam0, EM.PREMISE_RECT, False)
    assert 100 < rig.m.info()[0] < 2900
    rig.translate((0.4, 0.3, -0.2))
    rig.store_pos_other()
    rig.rotate(Q1)
    orc = O.Oracle(rig.m.current_asset())
    orc.order[:] = old.order                                       # the reference's stable sort continues from the order before the move
    orc.sort(camera.sort_matrix(cam1, r.transform.localToWorldMatrix))
    P = r.FrameParams(cam1)
    want_view = orc.calc_view(P).copy()
    want = orc.draw(P, blend)
    got = _frame(r, cam1, rt)
    assert views_equal(r.DownloadView(), want_view)
    assert np.array_equal(r.DownloadOrder(), orc.order)
    e = rt_err(got, want)
    print("frame after the move: rt_err", e)
    assert e <= RT_TOL
    stale = O.Oracle(a); stale.order[:] = old.order; stale.sort(camera.sort_matrix(cam1, r.transform.localToWorldMatrix)); stale.calc_view(P)
    assert rt_err(stale.draw(P, blend), want) > 16 * RT_TOL and not np.array_equal(before, got)      # the move is visible
    rt.Dispose(); rig.close()


# ---- 5. GS_SORT_VISIBLE: the history of sorts of the old positions --------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [None, 3])
def test_visible_order_across_a_move(gpu_ctx, limit):
    a = scene_asset(3000)
    rig = TRig(gpu_ctx, a, sort_mode=SortMode.Visible)
    r = rig.r
    if limit:
        r.SetSortHistoryLimit(limit)
    rt = RenderTarget(gpu_ctx, 320, 200)
    orc = O.Oracle(a)
    cams = [default_camera(az=7.0 * k, elev=5.0 + 3 * k) for k in range(9)]

    def frame(k, cam):
        orc.sort(camera.sort_matrix(cam, r.transform.localToWorldMatrix))
        r.SortPoints(cam); r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
        P = r.FrameParams(cam); orc.calc_view(P); vis = visible_bits(orc, P)
        got, want = r.DownloadVisibleOrder(), orc.order[vis[orc.order]]
        assert np.array_equal(got, want), f"frame {k}: visible order differs"

    for k in range(4):
        frame(k, cams[k])
    rig.update(cams[3], EM.PREMISE_RECT, False)
    rig.store_pos_other()
    for step in range(2):                                          # two moves, frames in between
        r.CalcViewData(cams[3])                                    # (a per-frame launch: the view buffer is not materialised)
        if step == 0:
            rig.translate((0.4, 0.3, -0.2))
        else:
            rig.rotate(Q2)
        with pytest.raises(_lib.GsError) as err:
            r.DownloadView()
        assert err.value.code == BAD and "calc_view has not run since the splats were moved" in str(err.value)
        moved = O.Oracle(rig.m.current_asset())
        moved.order[:] = orc.order
        orc = moved
        for k in range(4 + 3 * step, 7 + 3 * step - (1 if step else 0)):
            frame(k, cams[k])
        assert views_equal(r.DownloadView(), orc.view)             # after a calc_view the view buffer can be had again
    assert np.array_equal(r.DownloadOrder(), orc.order)
    rt.Dispose(); rig.close()


# ---- 6. frames in flight ------------------------------------------------------------------------------------------------------------------------
def test_a_move_between_frames_in_flight(gpu_ctx):
    a = scene_asset(3000)
    sel = EM.pack_bits(np.random.default_rng(9).random(3000) < 0.4, (3000 + 31) // 32)
    cams = [default_camera(az=10.0), default_camera(az=20.0), default_camera(az=20.0), default_camera(az=35.0), default_camera(az=50.0)]
    lib = _lib.lib()

    def run(frames_in_flight):
        r = GaussianSplatRenderer(gpu_ctx, a)
        r.sortMode = SortMode.Visible
        r.CreateResourcesForAsset()
        if frames_in_flight > 1:
            r.SetFramesInFlight(frames_in_flight)
            assert r.FramesInFlight() == (frames_in_flight, True)
        r.UploadSelectedBits(sel)
        r.EditStorePosMouseDown(); r.EditStoreOtherMouseDown()
        rts = [RenderTarget(gpu_ctx, 320, 200) for _ in cams]
        d, (_, c), (_, m0), (_, m1), (_, q) = fptr((0.4, 0.3, -0.2)), fptr(CENTRE), fptr(TOOL.localToWorldMatrix), fptr(TOOL.worldToLocalMatrix), fptr(Q1)
        for k, cam in enumerate(cams):
            r.SortPoints(cam); r.CalcViewData(cam); rts[k].Clear(); r.Draw(cam, rts[k])
            if k == 1:                                             # between frame 1 and frame 2 (the same camera): the raw asynchronous calls, nothing waits
                _lib.check(lib.gs_renderer_edit_translate_selection(r._r_h, d[1]), "translate")
                _lib.check(lib.gs_renderer_edit_rotate_selection(r._r_h, c, m0, m1, q), "rotate")
        out = [t.Download() for t in rts]
        blobs = r.DownloadPosOther()
        for t in rts:
            t.Dispose()
        r.DisposeResourcesForAsset()
        return out, blobs

    want, wb = run(1)
    got, gb = run(2)
    for k in range(len(cams)):
        assert np.array_equal(got[k], want[k]), f"frame {k}"
    assert np.array_equal(gb[0], wb[0]) and np.array_equal(gb[1], wb[1])
    assert rt_err(want[2], want[1]) > 16 * RT_TOL                  # frame 1 shows the old positions, frame 2 (the same camera) the new
    m = TM.TransformModel(a)
    m.upload_selected(sel); m.store_pos(); m.store_other()
    m.translate((0.4, 0.3, -0.2)); m.rotate(CENTRE, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, Q1)
    assert TM.blobs_equal(gb[0], m.pos_blob, floats=True) and TM.blobs_equal(gb[1], m.other_blob, floats=False)


# ---- 7. export after a move ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bake", [False, True])
def test_export_after_a_move(gpu_ctx, bake):
    a = scene_asset(3000)
    tr = camera.Transform(**XM.BAKE_TRANSFORM)
    rig = TRig(gpu_ctx, a, transform=tr)
    cam = default_camera()
    rig.update(cam, EM.PREMISE_RECT, False)
    doomed = int(rig.m.info()[0])
    assert doomed > 100
    rig.delete()                                                   # deleted, then moved: select all takes the deleted splats along
    rig.select_all()
    rig.translate((0.4, 0.3, -0.2))
    rig.store_pos_other()
    rig.rotate(Q1)
    rig.scale((1.5, -0.5, 0.25))
    xm = XM.ExportModel(rig.m.current_asset())
    xm.edit.set_deleted_bits(rig.m.bits()[2])
    want = xm.export_alive(tr, bake)
    got = rig.r.ExportAlive(bake)
    assert len(want) == 3000 - doomed == len(got)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    moved_pos = rig.m.pos_rows()[~EM.unpack_bits(rig.m.bits()[2], 3000)]
    if not bake:
        assert np.array_equal(got[:, 0:3].view(np.uint32), moved_pos.view(np.uint32))      # the new positions, none of a deleted splat
    rig.close()
