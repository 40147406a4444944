"""Selection and deletion on the CPU box: the C-ABI surface of the gs_renderer_edit_* calls, known answers of the numpy model the GPU tests are held to
(tests/edit_model.py), the premises of the cases those tests use -- asserted, so that no case passes vacuously -- and the host build of the kernels'
per-splat arithmetic (csrc/gs_device_math.h through tests/edit_host_harness.cpp) against the model, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import edit_model as EM
from common import default_camera, small_asset
from harness import build_harness
from unitygaussiansplatting_amd import _abi, _lib, camera
from unitygaussiansplatting_amd.cutout import shader_data_array
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

f32 = np.float32


point_asset = EM.point_asset


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_edit_entry_points_validate_a_null_renderer():
    lib = _lib.lib()
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    assert C.sizeof(_abi.gs_edit_info) == 36
    info, P = _abi.gs_edit_info(), _abi.gs_frame_params()
    rect, w = (C.c_float * 4)(0, 0, 1, 1), (C.c_uint32 * 1)(0)
    assert lib.gs_renderer_edit_select_all(None) == bad
    assert lib.gs_renderer_edit_deselect_all(None) == bad
    assert lib.gs_renderer_edit_invert_selection(None) == bad
    assert lib.gs_renderer_edit_store_selection(None) == bad
    assert lib.gs_renderer_edit_update_selection(None, C.byref(P), rect, 0) == bad
    assert lib.gs_renderer_edit_delete_selected(None) == bad
    assert lib.gs_renderer_edit_info(None, C.byref(info)) == bad
    assert lib.gs_renderer_edit_upload_selected_bits(None, w, 1) == bad
    assert lib.gs_renderer_edit_download_bits(None, w, None, None, 1) == bad
    assert lib.gs_renderer_edit_release(None) == bad
    assert lib.gs_abi_version() == 9                             # additions to ABI 9


def test_renderer_mirrors_the_edit_methods():
    for name in ("EnsureEditingBuffers", "EditStoreSelectionMouseDown", "EditUpdateSelection", "EditDeleteSelected", "EditSelectAll", "EditDeselectAll",
                 "EditInvertSelection", "UpdateEditCountsAndBounds", "DownloadEditBits", "UploadSelectedBits"):
        assert callable(getattr(GaussianSplatRenderer, name)), name
    r = GaussianSplatRenderer.__new__(GaussianSplatRenderer)      # no context: the fields only
    r.m_GpuEditSelected = False
    r.UpdateEditCountsAndBounds()                                 # no edit buffers: zeros (GaussianSplatRenderer.cs:707-715)
    assert (r.editSelectedSplats, r.editDeletedSplats, r.editCutSplats, r.editModified) == (0, 0, 0, False)
    assert not r.editSelectedBounds.extents.any() and not r.editSelectedBounds.center.any()


# ---- 2. known answers of the model ------------------------------------------------------------------------------------------------------
def test_select_all_counts_the_tail_bits_of_the_last_word():
    m = EM.EditModel(point_asset(33))
    assert not m.info().any()                                      # before any edit call
    m.select_all()
    assert m.bits()[0].tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
    info = m.info()
    assert info[0] == 64 and info[1] == 0 and info[2] == 0         # the reference's quirk: 64 selected of 33
    want_lo, want_hi = m.pos.min(axis=0), m.pos.max(axis=0)        # ... but the bounds are of the 33 positions
    assert info[3:6].view(f32).tolist() == want_lo.tolist() and info[6:9].view(f32).tolist() == want_hi.tolist()
    m.invert_selection()
    assert m.bits()[0].tolist() == [0, 0] and m.info()[0] == 0
    assert m.info()[3:6].view(f32).tolist() == [f32(1.0e38)] * 3 and m.info()[6:9].view(f32).tolist() == [f32(-1.0e38)] * 3


def test_sortable_uint_round_trip():
    vals = np.array([0.0, -0.0, 1.0, -1.0, 1.0e38, -1.0e38, np.inf, -np.inf, 1.0e-45, -1.0e-45, 3.4028235e38, 0.3], f32)
    u = EM.float_to_sortable_uint(vals)
    assert np.array_equal(EM.sortable_uint_to_float(u).view(np.uint32), vals.view(np.uint32))
    order = np.argsort(u, kind="stable")
    assert np.array_equal(np.sort(vals.astype(np.float64)), vals[order].astype(np.float64))      # monotonic
    assert u[1] < u[0]                                             # -0 sorts below +0
    assert EM.INIT_MIN == int(u[4]) and EM.INIT_MAX == int(u[5])


def test_a_nan_position_is_selected_by_any_rectangle_and_never_in_the_bounds():
    n, k = 70, 41
    m = EM.EditModel(point_asset(n, nan_at=k))
    assert np.isnan(m.pos[k, 0]) and np.isnan(m.pos[k, 2]) and m.pos[k, 1] == f32(0.5)
    cam = default_camera()
    P = camera.frame_params(cam, camera.Transform())
    for rect in ((-5000.0, -5000.0, -4000.0, -4000.0), (10.0, 10.0, 5.0, 5.0), EM.PREMISE_RECT):
        assert m.hits(P, rect)[k]
    m.update_selection(P, (-5000.0, -5000.0, -4000.0, -4000.0), False)
    assert EM.unpack_bits(m.bits()[0], n).nonzero()[0].tolist() == [k]
    info = m.info()
    assert info[0] == 1
    # x and z of the only selected splat are NaN: dropped; its y is kept
    assert info[3:6].view(f32).tolist() == [f32(1.0e38), f32(0.5), f32(1.0e38)] and info[6:9].view(f32).tolist() == [f32(-1.0e38), f32(0.5), f32(-1.0e38)]


def test_delete_then_info():
    m = EM.EditModel(small_asset(20011, 5, "Medium"))
    P = camera.frame_params(default_camera(), camera.Transform())
    first = EM.pack_bits(np.arange(m.n) % 7 == 0, m.nw)
    m.set_deleted_bits(first)
    m.update_selection(P, EM.PREMISE_RECT, False)
    sel = m.bits()[0].copy()
    assert m.info()[0] == EM.popcount(sel & ~first)                # deleted splats do not count as selected
    m.delete_selected()
    info = m.info()
    assert info[0] == 0 and info[1] == EM.popcount(first | sel) and not m.bits()[0].any()
    assert np.array_equal(m.bits()[2], first | sel)


# ---- 3. premises of the GPU cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality,hits_want", [("Medium", 5755), ("VeryHigh", 5754)])
def test_premises_of_the_rectangle_cases(quality, hits_want):
    m = EM.EditModel(small_asset(20011, 5, quality))
    tr = camera.Transform()
    P = camera.frame_params(default_camera(), tr)
    hits = int(m.hits(P, EM.PREMISE_RECT).sum())
    print(quality, "orbit camera hits", hits)
    assert hits == hits_want
    Pi = camera.frame_params(EM.inside_camera(), tr)
    w = m.clip_positions(Pi)[:, 3]
    front, behind, hin = int((w > 0).sum()), int((w <= 0).sum()), int(m.hits(Pi, EM.PREMISE_RECT).sum())
    print(quality, "inside camera: front", front, "behind", behind, "hits", hin)
    assert hin >= 100 and behind >= 1000
    assert front + behind == m.n
    assert not m.hits(P, (-900.0, -900.0, -800.0, -800.0)).any() and not m.hits(P, (200.0, 50.0, 100.0, 150.0)).any()      # off screen / empty
    whole = m.hits(P, (0.0, 0.0, 320.0, 200.0))
    assert hits < int(whole.sum()) <= m.n


@pytest.mark.parametrize("n,quality", [(20011, "Medium"), (20011, "VeryHigh"), (5003, "Medium"), (257, "points")])
def test_every_cutout_list_leaves_a_tenth_on_each_side(n, quality):
    m = EM.EditModel(point_asset(n) if quality == "points" else small_asset(n, 5, quality))
    seen = {}
    for name, cuts in EM.cutout_lists().items():
        m.set_cutouts(cuts, camera.Transform().localToWorldMatrix)
        c = int(m.cut.sum())
        seen[name] = m.cut.copy()
        print(n, quality, name, "cut", c)
        if cuts is None:
            assert c == 0
        else:
            assert 0.1 * n <= c <= 0.9 * n, (name, c)
    assert len({v.tobytes() for v in seen.values()}) == 4          # four different cut sets: every entry of every list decides something


# ---- 4. the host build of the kernels' arithmetic against the model ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def eh(tmp_path_factory):
    return C.CDLL(build_harness(tmp_path_factory.mktemp("eh"), "edit_host_harness.cpp"))


@pytest.mark.parametrize("quality", ["Medium", "VeryHigh"])
def test_host_build_of_the_edit_arithmetic_equals_the_model(eh, quality):
    m = EM.EditModel(small_asset(3001, 9, quality))
    n = m.n
    rng = np.random.default_rng(2024)
    lists = list(EM.cutout_lists().values())
    transforms = [camera.Transform(), camera.Transform(position=(0.1, -0.2, 0.3), rotation=(0.1, 0.2, 0.05, 0.9695), scale=(1.0, 1.0, 1.0)),
                  camera.Transform(position=(-0.3, 0.1, 0.0), scale=(1.0, 1.0, -1.0))]
    hit, cut = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    lo, hi = np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32)
    total_hits = total_behind = 0
    for case in range(200):
        tr = transforms[case % 3]
        cuts = lists[(case // 3) % 4]
        m.set_cutouts(cuts, tr.localToWorldMatrix)
        W, H = int(rng.integers(16, 700)), int(rng.integers(16, 500))
        eye = rng.standard_normal(3) * rng.choice([0.5, 3.0, 7.0])
        cam = camera.Camera(position=tuple(eye), target=tuple(rng.standard_normal(3) * 0.7), fieldOfView=float(rng.uniform(25.0, 100.0)),
                            pixelWidth=W, pixelHeight=H)
        P = camera.frame_params(cam, tr)
        x0, x1 = np.sort(rng.uniform(-0.2 * W, 1.2 * W, 2))
        y0, y1 = np.sort(rng.uniform(-0.2 * H, 1.2 * H, 2))
        rect = np.array([x0, y0, x1, y1], f32) if case % 17 else np.array([x1, y0, x0, y1], f32)      # (every 17th: empty)
        arr, cnt = shader_data_array(cuts, tr.localToWorldMatrix)
        eh.eh_eval(C.byref(m.orc.desc), C.byref(P), rect.ctypes.data_as(C.c_void_p), arr, C.c_uint32(cnt), hit.ctypes.data_as(C.c_void_p),
                   cut.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p))
        want = m.hits(P, rect)
        assert np.array_equal(cut.astype(bool), m.cut), case
        assert np.array_equal(hit.astype(bool), want), case
        assert np.array_equal(lo, m.lo) and np.array_equal(hi, m.hi), case
        total_hits += int(want.sum())
        total_behind += int((m.clip_positions(P)[:, 3] <= 0).sum())
    assert total_hits > 20 * 200 and total_behind > 20 * 200, (total_hits, total_behind)
