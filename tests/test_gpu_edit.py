"""Selection and deletion on the GPU (csrc/gs_edit.hip through the gs_renderer_edit_* calls and GaussianSplatRenderer.Edit*) against the numpy model of the
reference's seven kernels (tests/edit_model.py; its premises are asserted on the CPU by tests/test_edit_model.py).  After EVERY call the three bit buffers
(DownloadEditBits) and gs_renderer_edit_info are compared with the model: every bit, and every float's bit pattern."""
import ctypes as C

import numpy as np
import pytest

import edit_model as EM
import oracle_lib as O
from common import RT_TOL, default_camera, rt_err, small_asset, views_equal
from gpu_rig import Rig
from unitygaussiansplatting_amd import _lib, camera
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
f32 = np.float32
OFF_SCREEN = (-900.0, -900.0, -800.0, -800.0)
EMPTY = (200.0, 50.0, 100.0, 150.0)                 # x_min > x_max
WHOLE = (0.0, 0.0, 320.0, 200.0)
SECOND_RECT = (150.5, 20.0, 310.0, 120.25)          # overlaps the premise rectangle


def walk(rig: Rig, cam):
    """select all, invert, rectangle add, store, rectangle subtract, delete, info -- and what they leave for one another"""
    rig.select_all()
    rig.invert()                                                   # -> nothing (but the tail bits stay cleared)
    rig.update(cam, EM.PREMISE_RECT, False)
    rig.store()
    rig.update(cam, SECOND_RECT, True)                             # the stored selection minus the second rectangle
    rig.update(cam, SECOND_RECT, False)                            # ... plus it
    rig.invert()
    rig.delete()
    rig.select_all()                                               # deleted splats may be selected again; info does not count them
    rig.update(cam, WHOLE, True)
    rig.delete()


# ---- 1. sizes at the seams of the kernel shape ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257])
def test_sizes_at_the_seams_fp32(gpu_ctx, n):
    rig = Rig(gpu_ctx, EM.point_asset(n))
    cam = default_camera()
    if n >= 255:                                                   # the rectangles split the splats
        h = rig.m.hits(rig.r.FrameParams(cam), EM.PREMISE_RECT)
        assert 0 < int(h.sum()) < n
    walk(rig, cam)
    if n == 33:
        rig.select_all()
        assert rig.raw_info()[0] == 64 - int(EM.popcount(rig.m.bits()[2]))      # the tail bits are counted
    rig.close()


@pytest.mark.parametrize("n,quality", [(257, "Medium"), (20011, "Medium"), (20011, "VeryHigh")])
def test_sizes_chunked_and_large(gpu_ctx, n, quality):
    a = small_asset(n, 5, quality)
    assert (a.chunkData is not None and len(a.chunkData) > 0) == (quality == "Medium")      # Medium: chunked Norm11, partial last chunk
    rig = Rig(gpu_ctx, a)
    walk(rig, default_camera())
    assert rig.m.info()[1] > 0
    rig.close()


# ---- 2. rectangles ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["orbit", "inside"])
def test_rectangles(gpu_ctx, which):
    rig = Rig(gpu_ctx, small_asset(20011, 5, "Medium"))
    cam = default_camera() if which == "orbit" else EM.inside_camera()
    for rect in (WHOLE, EMPTY, EM.PREMISE_RECT, OFF_SCREEN):
        rig.update(cam, rect, False)
    # the mouse-down copy is empty, so what is selected is what projects into the off-screen rectangle: nothing from outside the scene; from inside it a
    # few splats far off the axis, in front of the camera (w > 0) all the same
    off = int(rig.m.hits(rig.r.FrameParams(cam), OFF_SCREEN).sum())
    assert rig.m.info()[0] == off and (off == 0 if which == "orbit" else off < 100)
    rig.update(cam, EM.PREMISE_RECT, False)
    assert rig.m.info()[0] >= 100
    rig.select_all()
    rig.store()
    for rect in (EM.PREMISE_RECT, EMPTY, OFF_SCREEN, WHOLE):
        rig.update(cam, rect, True)                                # subtract after select-all
    assert 0 < rig.m.info()[0] < 20011 + 21                        # what the whole screen leaves: behind the camera or outside it (+ the 21 tail bits)
    rig.close()


# ---- 3. cutouts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EM.cutout_lists()))
@pytest.mark.parametrize("asset_name", ["5003 Medium", "257 points"])
def test_cutouts(gpu_ctx, asset_name, name):
    a = small_asset(5003, 5, "Medium") if asset_name == "5003 Medium" else EM.point_asset(257)
    rig = Rig(gpu_ctx, a)
    cam = default_camera()
    rig.set_cutouts(EM.cutout_lists()[name])
    rig.select_all()
    if name != "none":
        assert rig.m.info()[2] == int(rig.m.cut.sum()) > 0         # editCutSplats
    rig.invert()
    rig.update(cam, WHOLE, False)
    rig.store()
    rig.update(cam, EM.PREMISE_RECT, True)
    # a selection from the host that includes cut splats and the tail bits: info drops the cut ones from the count and from the bounds
    words = np.random.default_rng(8).integers(0, 2 ** 32, rig.m.nw, dtype=np.uint64).astype(np.uint32)
    words[-1] |= np.uint32(0x80000000)
    rig.upload_selected(words)
    if name != "none":
        assert rig.m.info()[0] < EM.popcount(words)
    rig.delete()
    rig.set_cutouts(None)
    rig.select_all()
    rig.close()


# ---- 4. one NaN position -----------------------------------------------------------------------------------------------------------------------
def test_a_nan_position(gpu_ctx):
    n, k = 70, 41
    rig = Rig(gpu_ctx, EM.point_asset(n, nan_at=k))
    cam = default_camera()
    rig.update(cam, OFF_SCREEN, False)                             # selected by a rectangle nothing projects into ...
    assert EM.unpack_bits(rig.r.DownloadEditBits()[0], n).nonzero()[0].tolist() == [k]
    info = rig.raw_info()
    assert info[0] == 1 and info[3:6].view(f32).tolist() == [f32(1.0e38), f32(0.5), f32(1.0e38)]      # ... and never in the bounds
    rig.select_all()
    got = rig.raw_info()
    assert not np.isnan(got[3:9].view(f32)).any()
    rig.delete()
    rig.close()


# ---- 5. seeded call sequences ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_seeded_call_sequences(gpu_ctx, seed):
    rng = np.random.default_rng(1000 + seed)
    rig = Rig(gpu_ctx, small_asset(5003, 5, "Medium"))
    cams = [default_camera(), EM.inside_camera()]
    lists = list(EM.cutout_lists().values())
    ops = ["select_all", "deselect_all", "invert", "store", "update", "delete", "info", "set_cutouts", "set_deleted_bits", "set_deleted_bits_null", "release"]
    for _ in range(12):
        op = ops[int(rng.integers(len(ops)))]
        if op == "update":
            W, H = 320.0, 200.0
            x = np.sort(rng.uniform(-0.1 * W, 1.1 * W, 2)); y = np.sort(rng.uniform(-0.1 * H, 1.1 * H, 2))
            rig.update(cams[int(rng.integers(2))], (float(f32(x[0])), float(f32(y[0])), float(f32(x[1])), float(f32(y[1]))), bool(rng.integers(2)))
        elif op == "set_cutouts":
            rig.set_cutouts(lists[int(rng.integers(4))])
        elif op == "set_deleted_bits":
            rig.set_deleted_bits(rng.integers(0, 2 ** 32, rig.m.nw, dtype=np.uint64).astype(np.uint32) & rng.integers(0, 2 ** 32, rig.m.nw, dtype=np.uint64).astype(np.uint32))
        elif op == "set_deleted_bits_null":
            rig.set_deleted_bits(None)
        elif op == "info":
            rig.check("info")
        else:
            getattr(rig, op)()
    rig.close()


# ---- 6. deletion reaches the frame ---------------------------------------------------------------------------------------------------------------
def _oracle_frame(orc, P, bits):
    view = orc.calc_view(P, deleted_bits=bits).copy()
    return view, orc.draw(P, 0)


def test_deletion_reaches_the_frame(gpu_ctx):
    a = small_asset(20011, 5, "Medium")
    rig = Rig(gpu_ctx, a)
    r, cam = rig.r, default_camera()
    rt = RenderTarget(gpu_ctx, 320, 200)
    rig.update(cam, EM.PREMISE_RECT, False)
    rig.delete()
    assert r.editModified and r.editDeletedSplats == 5755
    orc = O.Oracle(a)
    orc.sort(camera.sort_matrix(cam, r.transform.localToWorldMatrix))
    P = r.FrameParams(cam)
    want_view, want = _oracle_frame(orc, P, rig.m.bits()[2])
    r.SortPoints(cam); r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
    assert views_equal(r.DownloadView(), want_view)
    e = rt_err(rt.Download(), want)
    print("frame after the delete: rt_err", e)
    assert e <= RT_TOL
    _, before = _oracle_frame(orc, P, None)
    assert rt_err(before, want) > 16 * RT_TOL                      # the delete is visible
    rt.Dispose(); rig.close()


def test_deletion_reaches_the_lanes(gpu_ctx):
    """GS_SORT_VISIBLE with two frames in flight: a frame dealt before the delete keeps the old bits, the two frames after it -- one per lane -- have the new ones.
    Nothing synchronises between the calls: the selection and the delete are the raw asynchronous entry points."""
    a = small_asset(20011, 5, "Medium")
    r = GaussianSplatRenderer(gpu_ctx, a)
    r.sortMode = SortMode.Visible
    r.CreateResourcesForAsset()
    r.SetFramesInFlight(2)
    assert r.FramesInFlight() == (2, True)
    m = EM.EditModel(a)
    cam = default_camera()
    P = r.FrameParams(cam)
    rts = [RenderTarget(gpu_ctx, 320, 200) for _ in range(3)]
    lib = _lib.lib()
    r.SortPoints(cam)
    r.CalcViewData(cam); rts[0].Clear(); r.Draw(cam, rts[0])      # dealt to lane 0 before the delete
    rect = (C.c_float * 4)(*EM.PREMISE_RECT)
    _lib.check(lib.gs_renderer_edit_update_selection(r._r_h, C.byref(P), rect, 0), "gs_renderer_edit_update_selection")
    _lib.check(lib.gs_renderer_edit_delete_selected(r._r_h), "gs_renderer_edit_delete_selected")
    m.update_selection(P, EM.PREMISE_RECT, False); m.delete_selected()
    views = []
    for k in (1, 2):                                               # lane 1, then lane 0
        r.CalcViewData(cam); rts[k].Clear(); r.Draw(cam, rts[k])
        views.append(r.DownloadView())
    orc = O.Oracle(a)
    orc.sort(camera.sort_matrix(cam, r.transform.localToWorldMatrix))
    _, old = _oracle_frame(orc, P, None)
    new_view, new = _oracle_frame(orc, P, m.bits()[2])
    assert rt_err(old, new) > 16 * RT_TOL
    imgs = [t.Download() for t in rts]
    errs = [rt_err(imgs[0], old), rt_err(imgs[1], new), rt_err(imgs[2], new)]
    print("rt_err before / after / after:", errs)
    assert max(errs) <= RT_TOL
    assert views_equal(views[0], new_view) and views_equal(views[1], new_view)
    got = r.DownloadEditBits()
    assert np.array_equal(got[2], m.bits()[2]) and not got[0].any()
    for t in rts:
        t.Dispose()
    r.DisposeResourcesForAsset()
