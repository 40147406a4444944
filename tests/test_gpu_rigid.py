"""The rigid rotate / scale of the selection on the GPU (csrc/gs_edit.hip's RIGID transform kernels through gs_renderer_edit_set_rigid_transforms,
gs_renderer_edit_store_sh_mouse_down and the rotate / scale calls) against the numpy twin (tests/rigid_model.py; held to the host build of the
shipped lines, to the merge and to the physics by tests/test_rigid_model.py).  After EVERY call the renderer's pos, other and SH blobs are compared
with the model bit for bit, the colour blob with the asset's, and the bit buffers and counts as in every edit suite."""
import numpy as np
import pytest

import bake_model as BM
import copy_model as CM
import edit_model as EM
import export_model as XM
import oracle_lib as O
import rigid_model as RM
import spz_export_model as SM
import transform_model as TM
from builders import TOOL
from common import RT_TOL, default_camera, rt_err, small_asset, views_equal
from gpu_rig import BAD, Rig, check_bake, draw_frame, fptr
from unitygaussiansplatting_amd import _lib, camera
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
f32 = np.float32
CENTRE = (0.3, -0.2, 0.1)
Q1 = (0.18257419, 0.36514837, 0.54772256, 0.73029674)
Q2 = (-1.0, 1.0, 1.0, 1.0)                                         # not of unit length: the call normalises it
TURN = camera.Transform(position=(0.2, -0.1, 0.3), rotation=(0.1, 0.2, 0.05, 0.9695))      # a tool frame that is a rotation: L is one too


class RRig(Rig):
    """gpu_rig.Rig over a RigidModel: the three blobs a transform may write are part of every comparison, and the one it may not"""

    def __init__(self, ctx, asset, transform=None, sort_mode=None, rigid=True):
        self.r = GaussianSplatRenderer(ctx, asset, transform)
        if sort_mode is not None:
            self.r.sortMode = sort_mode
        self.r.rigidTransforms = rigid                             # applied when the resources are made
        self.r.CreateResourcesForAsset()
        self.m = RM.RigidModel(asset, rigid)
        self.color0 = np.ascontiguousarray(asset.colorData, np.uint8).copy()
        self.lib = _lib.lib()
        self.steps = 0
        self.check("fresh")

    def check(self, what):
        super().check(what)
        pos, other, color, sh = self.r.DownloadSplatData()
        for name, g, w in zip(("pos", "other", "sh"), (pos, other, sh), self.m.blobs3()):
            assert TM.blobs_equal(g, w, floats=name != "other"), f"step {self.steps} ({what}): {name} differs at bytes {np.flatnonzero(g != w)[:8]}"
        assert np.array_equal(color, self.color0), f"step {self.steps} ({what}): the colour blob changed"
        if self.m.rot_gate:                                        # the last 12 bytes of every SH record are the asset's
            tail = lambda b: np.ascontiguousarray(b, np.uint8)[:self.m.n * 192].reshape(-1, 192)[:, 180:]
            assert np.array_equal(tail(sh), tail(self.m.sh_asset)), f"step {self.steps} ({what}): the tail of an SH record was written"

    def set_rigid(self, on):
        self.r.EditSetRigidTransforms(on); self.m.set_rigid(on)

    def store3(self):
        self.r.EditStorePosMouseDown(); self.r.EditStoreOtherMouseDown(); self.r.EditStoreSHMouseDown()
        self.m.store_pos(); self.m.store_other(); self.m.store_sh()
        self.check("store pos / other / sh")

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
        self.r.m_GpuEditPosMouseDown = self.r.m_GpuEditOtherMouseDown = self.r.m_GpuEditSHMouseDown = False

    # the raw calls, for their return codes
    def c_rotate(self, q=Q1, tr=TOOL, o2w=None):
        (_, c), (_, a), (_, b), (_, r) = fptr(CENTRE), fptr(tr.localToWorldMatrix if o2w is None else o2w), fptr(tr.worldToLocalMatrix), fptr(q)
        return self.lib.gs_renderer_edit_rotate_selection(self.r._r_h, c, a, b, r)

    def c_scale(self, s=(2.0, 2.0, 2.0)):
        (_, c), (_, a), (_, b), (_, v) = fptr(CENTRE), fptr(TOOL.localToWorldMatrix), fptr(TOOL.worldToLocalMatrix), fptr(s)
        return self.lib.gs_renderer_edit_scale_selection(self.r._r_h, c, a, b, v)


def drag(rig: RRig):
    """mouse down; rotate; rotate again from the same mouse-down state (the second delta alone); a uniform scale, a negative one, a non-uniform one;
    a new mouse down, after which a rotate composes with what is there"""
    at_mouse_down = rig.m.current_asset()
    rig.store3()
    rig.rotate(Q1)
    once = [b.copy() for b in rig.m.blobs3()]
    rig.rotate(Q2)
    if rig.m.selected().any() and rig.m.rot_gate:
        alone = RM.RigidModel(at_mouse_down, True)
        alone.upload_selected(rig.m.bits()[0]); alone.store_pos(); alone.store_other(); alone.store_sh()
        assert alone.rotate(CENTRE, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, Q2)
        assert all(np.array_equal(a, b) for a, b in zip(alone.blobs3(), rig.m.blobs3()))         # not the composition with Q1
        assert not np.array_equal(once[2], rig.m.sh_blob) and not np.array_equal(once[1], rig.m.other_blob)
    rig.scale((2.0, 2.0, 2.0))
    rig.scale((-0.5, -0.5, -0.5))
    rig.scale((1.5, -0.5, 0.25))
    rig.store3()
    before = rig.m.sh_blob.copy()
    rig.rotate(Q1, TURN)
    if rig.m.selected().any() and rig.m.rot_gate:
        assert not np.array_equal(before, rig.m.sh_blob)


def selections(rig, n):
    nw = rig.m.nw
    out = [("none", np.zeros(nw, np.uint32))]
    for name, picks in (("splat 0", [0]), ("splats 31 and 32", [31, 32]), ("the last splat", [n - 1])):
        if max(picks) < n:
            flags = np.zeros(n, bool); flags[picks] = True
            out.append((name, EM.pack_bits(flags, nw)))
    tail = EM.pack_bits(np.random.default_rng(n).random(n) < 0.5, nw)
    tail[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32) if n % 32 else np.uint32(0)         # the bits of the last word beyond N, set
    out.append(("random half with the tail bits set", tail))
    return out


# ---- 1. sizes and selections at the seams of the kernel shape -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 300])
def test_seams(gpu_ctx, n):
    a = small_asset(n, 5, "VeryHigh")
    rig = RRig(gpu_ctx, a)
    assert rig.m.pos_gate and rig.m.rot_gate
    for name, words in selections(rig, n):
        rig.upload_selected(words)
        unselected = ~rig.m.selected()
        before = [b.copy() for b in rig.m.blobs3()]
        drag(rig)
        pos, other, _, sh = rig.r.DownloadSplatData()
        for b0, b1, stride in zip(before, (pos, other, sh), (12, 16, 192)):
            rec = lambda b: np.ascontiguousarray(b, np.uint8)[:n * stride].reshape(n, stride)
            assert np.array_equal(rec(b0)[unselected], rec(b1)[unselected]), (name, stride)      # unselected records: byte for byte
    rig.select_all()                                               # the tail bits set by the kernel itself
    if n % 32:
        assert EM.popcount(rig.m.bits()[0]) > n
    drag(rig)
    if n == 300:                                                   # a rectangle selection through a camera
        rig.deselect_all(); rig.store()
        rig.update(default_camera(), EM.PREMISE_RECT, False)
        assert 0 < rig.m.info()[0] < n
        drag(rig)
    rig.close()


# ---- 2. the setting, the copies, the gates ----------------------------------------------------------------------------------------------------------
def test_setting_off_is_the_reference(gpu_ctx):
    a = small_asset(300, 5, "VeryHigh")
    rig = RRig(gpu_ctx, a, rigid=False)
    ref = TM.TransformModel(a)
    words = EM.pack_bits(np.random.default_rng(3).random(300) < 0.5, rig.m.nw)
    rig.upload_selected(words); ref.upload_selected(words)
    rig.store3(); ref.store_pos(); ref.store_other()
    rig.rotate(Q1); rig.scale((2.0, 2.0, 2.0))
    ref.rotate(CENTRE, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, Q1); ref.scale(CENTRE, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, (2.0, 2.0, 2.0))
    pos, other, _, sh = rig.r.DownloadSplatData()
    assert TM.blobs_equal(pos, ref.pos_blob, floats=True) and np.array_equal(other, ref.other_blob) and np.array_equal(sh, np.asarray(a.shData, np.uint8))
    rig.set_rigid(True)                                            # switched on and off on the same renderer
    rig.rotate(Q1)
    assert not np.array_equal(rig.m.other_blob, ref.other_blob) and not np.array_equal(rig.m.sh_blob, sh)
    rig.set_rigid(False)
    rig.rotate(Q1)                                                 # the reference's rotation word again; the SH stay where the rigid call left them
    assert np.array_equal(rig.m.other_blob, ref.other_blob)
    rig.close()


def test_error_paths(gpu_ctx):
    rig = RRig(gpu_ctx, small_asset(33, 5, "VeryHigh"))
    rig.select_all()
    assert rig.c_rotate() == BAD and b"mouse-down" in rig.lib.gs_last_error_string()
    rig.r.EditStorePosMouseDown(); rig.m.store_pos()
    assert rig.c_scale() == BAD                                    # the uniform handle reads the other copy
    assert rig.c_scale((2.0, 2.0, 1.0)) == 0                       # ... a non-uniform scale is the reference's and does not
    assert rig.m.scale(CENTRE, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, (2.0, 2.0, 1.0))
    rig.check("non-uniform scale")
    rig.r.EditStoreOtherMouseDown(); rig.m.store_other()
    assert rig.c_rotate() == BAD and b"sh" in rig.lib.gs_last_error_string()       # all three
    rig.r.EditRotateSelection(CENTRE, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, Q1)      # the Python method returns silently
    rig.check("refused")
    rig.store3()
    assert rig.c_rotate((0.0, 0.0, 0.0, 0.0)) == BAD and rig.c_rotate((np.nan, 0.0, 0.0, 1.0)) == BAD and rig.c_rotate((np.inf, 0.0, 0.0, 1.0)) == BAD
    zero_row = np.array(TOOL.localToWorldMatrix, f32); zero_row[1, :3] = 0.0
    nan_row = np.array(TOOL.localToWorldMatrix, f32); nan_row[2, 0] = np.nan
    assert rig.c_rotate(o2w=zero_row) == BAD and rig.c_rotate(o2w=nan_row) == BAD
    rig.check("refused arguments change nothing")
    rig.set_rigid(False)
    assert rig.c_rotate((0.0, 0.0, 0.0, 0.0)) == 0                 # errors of the rigid mode only
    assert rig.m.rotate(CENTRE, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, (0.0, 0.0, 0.0, 0.0))
    rig.check("the reference's rotate takes any delta")
    rig.set_rigid(True)
    rig.rotate(Q1)
    rig.release()
    assert rig.c_rotate() == BAD and rig.c_scale() == BAD
    assert rig.lib.gs_renderer_edit_store_sh_mouse_down(None) == BAD and rig.lib.gs_renderer_edit_set_rigid_transforms(None, 1) == BAD
    rig.close()


def test_a_medium_asset_is_left_alone(gpu_ctx):
    a = small_asset(300, 5, "Medium")
    rig = RRig(gpu_ctx, a)
    assert not rig.m.pos_gate and not rig.m.rot_gate
    rig.select_all()
    rig.store3()
    assert rig.c_rotate() == 0 and rig.c_scale() == 0
    rig.rotate(Q1); rig.scale((2.0, 2.0, 2.0))                     # through the Python methods too
    pos, other, color, sh = rig.r.DownloadSplatData()
    for got, want in zip((pos, other, color, sh), (a.posData, a.otherData, a.colorData, a.shData)):
        assert np.array_equal(got, np.asarray(want, np.uint8))
    rig.close()


def test_a_resize_keeps_the_setting_and_drops_the_copies(gpu_ctx):
    a = small_asset(300, 5, "VeryHigh")
    rig = RRig(gpu_ctx, a)
    rig.select_all(); rig.store3(); rig.rotate(Q1)
    r = rig.r
    r.EditSetSplatCount(310)
    assert not r.m_GpuEditSHMouseDown and r.splatCount == 310
    r.EditSelectAll()
    assert rig.c_rotate() == BAD                                   # the mouse-down state went with the old buffers ...
    r.EditStorePosMouseDown(); r.EditStoreOtherMouseDown()
    assert rig.c_rotate() == BAD and b"sh" in rig.lib.gs_last_error_string()       # ... and the setting stayed: the rigid form asks for the third copy
    pos, other, color, sh = r.DownloadSplatData()
    m = RM.RigidModel(CM.Blobs(310, pos, other, color, sh).asset(), True)
    m.select_all(); m.store_pos(); m.store_other(); m.store_sh()
    r.EditStoreSHMouseDown()
    r.EditRotateSelection(CENTRE, TURN.localToWorldMatrix, TURN.worldToLocalMatrix, Q2)
    assert m.rotate(CENTRE, TURN.localToWorldMatrix, TURN.worldToLocalMatrix, Q2)
    got = r.DownloadSplatData()
    assert TM.blobs_equal(got[0], m.pos_blob, floats=True) and np.array_equal(got[1], m.other_blob) and TM.blobs_equal(got[3], m.sh_blob, floats=True)
    assert np.array_equal(got[2], color)
    r.DisposeResourcesForAsset()


# ---- 3. frames -----------------------------------------------------------------------------------------------------------------------------------------
def _frame(r, cam, rt):
    draw_frame(r, cam, rt)
    return rt.Download()


@pytest.mark.parametrize("mode", [SortMode.Full, SortMode.Visible])
def test_frames_after_a_rigid_rotate(gpu_ctx, mode):
    """the frame equals the oracle's over the model's blobs (GS_SORT_VISIBLE: through the consolidated base), and another renderer over the same asset
    draws the bits it drew before"""
    a = small_asset(300, 5, "VeryHigh")
    rig = RRig(gpu_ctx, a, sort_mode=mode)
    r = rig.r
    cam0, cam1 = default_camera(), default_camera(az=70.0, elev=-15.0)
    rt = RenderTarget(gpu_ctx, 320, 200)
    other = GaussianSplatRenderer(gpu_ctx, a)
    other.ShareResourcesOf(r)
    untouched = _frame(other, cam0, rt)
    old = O.Oracle(a)
    old.sort(camera.sort_matrix(cam0, r.transform.localToWorldMatrix))
    before = _frame(r, cam0, rt)
    rig.update(cam0, EM.PREMISE_RECT, False)
    assert 10 < rig.m.info()[0] < 290
    rig.store3()
    rig.rotate(axis_quarter_turn(), TURN, centre=(0.0, 0.0, 0.0))
    rig.scale((1.5, 1.5, 1.5), TURN, centre=(0.0, 0.0, 0.0))
    orc = O.Oracle(rig.m.current_asset())
    orc.order[:] = old.order                                       # the reference's stable sort continues from the order before the move
    orc.sort(camera.sort_matrix(cam1, r.transform.localToWorldMatrix))
    P = r.FrameParams(cam1)
    want_view = orc.calc_view(P).copy()
    want = orc.draw(P, 0)
    got = _frame(r, cam1, rt)
    assert views_equal(r.DownloadView(), want_view)
    assert np.array_equal(r.DownloadOrder(), orc.order)
    e = rt_err(got, want)
    print("frame after the rigid rotate: rt_err", e)
    assert e <= RT_TOL
    # the same edit in reference mode is another frame: the orientation and the SH are what this one is about
    ref = TM.TransformModel(a)
    ref.upload_selected(rig.m.bits()[0]); ref.store_pos(); ref.store_other()
    ref.rotate((0.0, 0.0, 0.0), TURN.localToWorldMatrix, TURN.worldToLocalMatrix, axis_quarter_turn())
    ref.scale((0.0, 0.0, 0.0), TURN.localToWorldMatrix, TURN.worldToLocalMatrix, (1.5, 1.5, 1.5))
    stale = O.Oracle(ref.current_asset()); stale.order[:] = old.order; stale.sort(camera.sort_matrix(cam1, r.transform.localToWorldMatrix)); stale.calc_view(P)
    assert rt_err(stale.draw(P, 0), want) > 16 * RT_TOL and not np.array_equal(before, got)
    assert np.array_equal(_frame(other, cam0, rt), untouched)      # the asset is untouched
    pos, oth, color, sh = other.DownloadSplatData()
    for g, w in zip((pos, oth, color, sh), (a.posData, a.otherData, a.colorData, a.shData)):
        assert np.array_equal(g, np.asarray(w, np.uint8))
    other.DisposeResourcesForAsset()
    rt.Dispose(); rig.close()


def axis_quarter_turn():
    s = np.sin(np.pi / 4.0) / np.sqrt(1.0 + 4.0 + 0.25)
    return tuple(np.array([1.0 * s, 2.0 * s, -0.5 * s, np.cos(np.pi / 4.0)], f32))


def test_a_rigid_rotate_between_frames_in_flight(gpu_ctx):
    a = small_asset(300, 5, "VeryHigh")
    sel = EM.pack_bits(np.random.default_rng(9).random(300) < 0.4, (300 + 31) // 32)
    cams = [default_camera(az=10.0), default_camera(az=20.0), default_camera(az=20.0), default_camera(az=35.0), default_camera(az=50.0)]
    lib = _lib.lib()

    def run(frames_in_flight):
        r = GaussianSplatRenderer(gpu_ctx, a)
        r.sortMode = SortMode.Visible
        r.rigidTransforms = True
        r.CreateResourcesForAsset()
        if frames_in_flight > 1:
            r.SetFramesInFlight(frames_in_flight)
            assert r.FramesInFlight() == (frames_in_flight, True)
        r.UploadSelectedBits(sel)
        r.EditStorePosMouseDown(); r.EditStoreOtherMouseDown(); r.EditStoreSHMouseDown()
        rts = [RenderTarget(gpu_ctx, 320, 200) for _ in cams]
        (_, c), (_, m0), (_, m1), (_, q), (_, s) = fptr(CENTRE), fptr(TURN.localToWorldMatrix), fptr(TURN.worldToLocalMatrix), fptr(Q1), fptr((1.25, 1.25, 1.25))
        for k, cam in enumerate(cams):
            r.SortPoints(cam); r.CalcViewData(cam); rts[k].Clear(); r.Draw(cam, rts[k])
            if k == 1:                                             # between frame 1 and frame 2 (the same camera): the raw asynchronous calls, nothing waits
                _lib.check(lib.gs_renderer_edit_rotate_selection(r._r_h, c, m0, m1, q), "rotate")
            if k == 3:
                _lib.check(lib.gs_renderer_edit_scale_selection(r._r_h, c, m0, m1, s), "scale")
        out = [t.Download() for t in rts]
        blobs = r.DownloadSplatData()
        for t in rts:
            t.Dispose()
        r.DisposeResourcesForAsset()
        return out, blobs

    want, wb = run(1)
    got, gb = run(2)
    for k in range(len(cams)):
        assert np.array_equal(got[k], want[k]), f"frame {k}"
    assert all(np.array_equal(g, w) for g, w in zip(gb, wb))
    assert rt_err(want[2], want[1]) > 16 * RT_TOL                  # frame 1 shows the old splats, frame 2 (the same camera) the new
    m = RM.RigidModel(a, True)
    m.upload_selected(sel); m.store_pos(); m.store_other(); m.store_sh()
    m.rotate(CENTRE, TURN.localToWorldMatrix, TURN.worldToLocalMatrix, Q1)
    want_after_rotate = m.sh_blob.copy()
    m.scale(CENTRE, TURN.localToWorldMatrix, TURN.worldToLocalMatrix, (1.25, 1.25, 1.25))
    assert TM.blobs_equal(gb[0], m.pos_blob, floats=True) and np.array_equal(gb[1], m.other_blob) and TM.blobs_equal(gb[3], want_after_rotate, floats=True)


# ---- 4. every reader sees the private SH blob ----------------------------------------------------------------------------------------------------------
def test_exports_and_the_bake_after_a_rigid_rotate(gpu_ctx, tmp_path):
    a = small_asset(300, 5, "VeryHigh")
    tr = camera.Transform(**XM.BAKE_TRANSFORM)
    rig = RRig(gpu_ctx, a, transform=tr)
    cam = default_camera()
    rig.update(cam, EM.PREMISE_RECT, False)
    assert rig.m.info()[0] > 10
    rig.delete()
    rig.select_all()
    rig.store3()
    rig.rotate(Q1, TURN)
    rig.scale((0.75, 0.75, 0.75), TURN)
    now = rig.m.current_asset()
    xm = XM.ExportModel(now)
    xm.edit.set_deleted_bits(rig.m.bits()[2])
    untouched = XM.ExportModel(a)
    untouched.edit.set_deleted_bits(rig.m.bits()[2])
    for bake in (False, True):
        want = xm.export_alive(tr, bake)
        got = rig.r.ExportAlive(bake)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), bake
        assert not np.array_equal(want[:, 9:54], untouched.export_alive(tr, bake)[:, 9:54])      # the f_rest columns are the rotated ones
        path = str(tmp_path / f"rigid{int(bake)}.ply")
        assert rig.r.ExportPlyFile(path, bake) == len(want)
        from unitygaussiansplatting_amd import creator
        back = creator.ReadPLY(path)
        assert np.array_equal(np.ascontiguousarray(back.sh, f32).view(np.uint32), np.ascontiguousarray(XM.columns(want).sh, f32).view(np.uint32))
        body, f = SM.body(want, xm.dec[xm.alive(), 10], 3, None)
        gbody, alive, used = rig.r.ExportSpzBody(bake, 3, None, 0)
        assert alive == len(want) and used == f and np.array_equal(gbody, body), bake
    alive = ~EM.unpack_bits(rig.m.bits()[2], 300)
    check_bake(rig.r, CM.decode(now)[alive], BM.VERY_HIGH, "after a rigid rotate")
    rig.close()
