"""The export on the GPU (csrc/gs_export.hip through the gs_renderer_edit_export_* calls and GaussianSplatRenderer.EditExportData / ExportAlive /
ExportPlyFile) against the numpy model of CSExportData and ExportPlyFile (tests/export_model.py; its premises are asserted on the CPU by
tests/test_export_model.py): every record bit for bit, every file byte for byte."""
import ctypes as C
import functools

import numpy as np
import pytest

import edit_model as EM
import export_model as XM
from common import PRESETS, default_camera, same_bits, small_asset
from gpu_rig import edit_info, make_renderer
from unitygaussiansplatting_amd import _abi, _lib, camera, creator
from unitygaussiansplatting_amd._lib import GsError
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
f32 = np.float32


@functools.lru_cache(maxsize=None)
def model_of(kind: str, n: int) -> XM.ExportModel:
    """one model (one oracle decode) per asset, shared by the tests that use the asset"""
    return XM.ExportModel(asset_of(kind, n))


def asset_of(kind: str, n: int):
    return EM.point_asset(n) if kind == "points" else small_asset(n, 5, kind)


def set_pattern(r: GaussianSplatRenderer, m: XM.ExportModel, name: str) -> None:
    words, cuts = XM.pattern(name, m.n)
    r.SetDeletedBits(words)
    r.m_Cutouts = cuts
    r.UpdateCutoutsBuffer()
    XM.apply_pattern(m, name, r.transform.localToWorldMatrix)


def three_outputs(r, path, bake=False):
    data, alive = r.EditExportData(bake), r.ExportAlive(bake)
    count = r.ExportPlyFile(path, bake)
    with open(path, "rb") as f:
        return data, alive, count, f.read()


def check_against_the_model(r, m, tmp_path, what, bake=False):
    tr = r.transform
    want_all, want_alive = m.export_data(tr, bake), m.export_alive(tr, bake)
    path = str(tmp_path / "out.ply")
    data, alive, count, blob = three_outputs(r, path, bake)
    assert same_bits(data, want_all), (what, np.argwhere(data.view(np.uint32) != want_all.view(np.uint32))[:6])
    assert same_bits(alive, want_alive), (what, alive.shape, want_alive.shape)
    assert count == len(want_alive)
    ref_path = str(tmp_path / "want.ply")
    creator.WritePLY(ref_path, XM.columns(want_alive))
    with open(ref_path, "rb") as f:
        assert blob == f.read(), what
    cols = XM.columns(want_alive)
    if len(want_alive) == 0:                                       # header only: the native importer refuses a file without vertices, the numpy one reads none
        with pytest.raises(GsError) as ei:
            creator.ReadPLYNative(path)
        assert ei.value.code == _abi.GS_ERR_INVALID_ASSET and len(creator.ReadPLY(path)) == 0
        return data, alive, blob
    back = creator.ReadPLYNative(path)
    for name in ("pos", "dc0", "sh", "opacity", "scale", "rot"):
        assert same_bits(getattr(back, name), getattr(cols, name)), (what, name)
    return data, alive, blob


# ---- 1. sizes at the seams, every pattern ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 255, 256, 257])
def test_sizes_at_the_seams(gpu_ctx, tmp_path, n):
    m = model_of("points" if n < 255 else "Medium", n)             # 255 .. 257: chunked Norm11 with a partial (or no) last chunk; 1, 33: fp32, chunk-less
    r = make_renderer(gpu_ctx, m.edit.asset)
    for name in XM.PATTERNS:
        set_pattern(r, m, name)
        _, alive, _ = check_against_the_model(r, m, tmp_path, (n, name))
        if name == "nothing deleted":
            assert len(alive) == n
        if name == "only the last alive":
            assert len(alive) == 1
    r.DisposeResourcesForAsset()


def test_the_tail_bits_of_33_splats(gpu_ctx, tmp_path):
    m = model_of("points", 33)
    m.edit.set_deleted_bits(None); m.edit.set_cutouts(None, camera.Transform().localToWorldMatrix); m.edit.release()
    r = make_renderer(gpu_ctx, m.edit.asset)
    r.EditSelectAll(); r.EditDeleteSelected()
    m.edit.select_all(); m.edit.delete_selected()
    assert r.DownloadEditBits()[2].tolist() == [0xFFFFFFFF, 0xFFFFFFFF] and r.editDeletedSplats == 64      # the bits beyond N are set and counted ...
    data, alive, blob = check_against_the_model(r, m, tmp_path, "tail bits")
    assert len(alive) == 0 and len(data) == 33                     # ... and the export writes no phantom
    assert blob.endswith(b"end_header\n") and b"element vertex 0\n" in blob
    m.edit.release(); m.edit.set_deleted_bits(None)
    r.DisposeResourcesForAsset()


# ---- 2. 20,000 splats (78 chunks + 32 splats) at every preset, every pattern ---------------------------------------------------------------
@pytest.mark.parametrize("name", XM.PATTERNS)
@pytest.mark.parametrize("quality", PRESETS)
def test_every_preset_and_pattern(gpu_ctx, tmp_path, quality, name):
    m = model_of(quality, 20000)
    r = make_renderer(gpu_ctx, m.edit.asset)
    set_pattern(r, m, name)
    _, alive, blob = check_against_the_model(r, m, tmp_path, (quality, name))
    want = XM.ALIVE_20000.get(name, XM.ALIVE_HALF_20000[quality])
    assert len(alive) == want
    r.EnsureEditingBuffers(); r.EditDeselectAll()                  # nothing selected: alive = N - deleted - cut of the edit info
    info = edit_info(r)
    assert info.selected == 0 and len(alive) == 20000 - info.deleted - info.cut
    if want == 0:
        assert blob.endswith(b"end_header\n")                      # header only
    r.DisposeResourcesForAsset()


def test_too_small_a_buffer_and_the_count_alone(gpu_ctx):
    m = model_of("Medium", 20000)
    r = make_renderer(gpu_ctx, m.edit.asset)
    set_pattern(r, m, "one chunk deleted")
    lib, p = _lib.lib(), r.ExportParams(False)
    buf = np.zeros((20000, 62), f32)
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    assert lib.gs_renderer_edit_export_data(r._r_h, C.byref(p), buf.ctypes.data, buf.nbytes - 1, 0) == bad
    alive = C.c_uint32(0)
    assert lib.gs_renderer_edit_export_alive(r._r_h, C.byref(p), None, 0, C.byref(alive)) == 0 and alive.value == 19744
    assert lib.gs_renderer_edit_export_alive(r._r_h, C.byref(p), buf.ctypes.data, 19743, C.byref(alive)) == bad
    assert not buf.any()
    assert lib.gs_renderer_edit_export_ply(r._r_h, C.byref(p), b"/nonexistent-directory/x.ply", C.byref(alive)) == bad
    r.DisposeResourcesForAsset()


# ---- 3. more chunks than one iteration of the scan's loop (1024 counts), by a non-multiple ---------------------------------------------------
def test_more_chunks_than_one_scan_iteration(gpu_ctx, tmp_path):
    m = model_of("Medium", 300000)                                 # 1172 chunks = 1024 + 148
    r = make_renderer(gpu_ctx, m.edit.asset)
    set_pattern(r, m, "half deleted under cutouts")
    _, alive, _ = check_against_the_model(r, m, tmp_path, "300000")
    assert 0 < len(alive) < 150000
    assert m.alive()[1024 * 256:].any() and m.alive()[:1024 * 256].any()
    r.DisposeResourcesForAsset()


# ---- 4. batching ------------------------------------------------------------------------------------------------------------------------------
def test_small_batches_give_the_same_bytes(gpu_ctx, tmp_path, monkeypatch):
    m = model_of("Medium", 20000)
    r = make_renderer(gpu_ctx, m.edit.asset)
    set_pattern(r, m, "half deleted under cutouts")
    data, alive, count, blob = three_outputs(r, str(tmp_path / "a.ply"))
    monkeypatch.setenv("GSPLAT_EXPORT_BATCH", "300")               # 300 splats -> 2 chunks per batch: 40 batches
    data2, alive2, count2, blob2 = three_outputs(r, str(tmp_path / "b.ply"))
    assert same_bits(data, data2) and same_bits(alive, alive2) and count == count2 and blob == blob2
    assert same_bits(alive, m.export_alive()) and count == XM.ALIVE_HALF_20000["Medium"]
    # the device-memory output of EditExportData: one launch over all N, the same bytes
    hip = C.CDLL("libamdhip64.so")                                 # (the runtime the library itself is linked against)
    dev, nbytes = C.c_void_p(), 20000 * 248
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(nbytes + 8)) == 0
    try:
        p = r.ExportParams(False)
        _lib.check(_lib.lib().gs_renderer_edit_export_data(r._r_h, C.byref(p), dev, nbytes, 1), "gs_renderer_edit_export_data")
        host = np.zeros((20000, 62), f32)
        assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), dev, C.c_size_t(nbytes), 2) == 0      # hipMemcpyDeviceToHost
        assert same_bits(host, data)
        odd = C.c_void_p(dev.value + 4)                            # records go out as dwordx2: a device buffer must be 8-byte aligned
        assert _lib.lib().gs_renderer_edit_export_data(r._r_h, C.byref(p), odd, nbytes, 1) == _abi.GS_ERR_INVALID_ARGUMENT
    finally:
        hip.hipFree(dev)
    r.DisposeResourcesForAsset()


# ---- 5. the baked transform -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", ["Medium", "VeryHigh"])
def test_baked_transform(gpu_ctx, tmp_path, quality):
    m = model_of(quality, 20000)
    tr = camera.Transform(**XM.BAKE_TRANSFORM)                     # rotated, non-uniformly scaled, mirrored in x
    r = make_renderer(gpu_ctx, m.edit.asset, tr)
    set_pattern(r, m, "half deleted under cutouts")
    data, alive, _ = check_against_the_model(r, m, tmp_path, ("baked", quality), bake=True)
    plain = r.EditExportData(False)
    assert same_bits(plain, m.export_data()) and same_bits(plain[:, 3:6], data[:, 3:6])      # the same splats are cut, baked or not
    assert not same_bits(plain[:, 9:54], data[:, 9:54]) and not same_bits(plain[:, 0:3], data[:, 0:3])
    r.DisposeResourcesForAsset()


# ---- 6. round trip through the importer --------------------------------------------------------------------------------------------------------
def test_round_trip_through_the_importer(gpu_ctx, tmp_path):
    """Export VeryHigh after a delete, re-import (VeryHigh, no Morton): positions and SH come back bit for bit; colour, opacity and scale within
    the bounds that follow from the documented bounds of LogDet (|LogDet(s) - ln s| <= e(s) = LOGDET_REL |ln s| + LOGDET_ABS) and ExpDet
    (relative error < 2^-22), with u = 2^-24:
      scale    s' = ExpDet(LogDet(s)):  |s' - s| <= s (exp(e(s)) (1 + 2^-22) - 1)
      opacity  q = v / (1 - v) carries <= 2 u relative (one subtraction, one division); l = LogDet(q); E = ExpDet(-l) has relative error
               rho <= exp(2.01 u + e(q)) (1 + 2^-22) - 1 against (1 - v) / v; v' = 1 / (1 + E) with two more roundings:
               |v' - v| <= v (1 - v) rho (1 + rho) + 2.01 u v
      colour   c' = ((c - 0.5) / k) k + 0.5, four roundings: |c' - c| <= 3.01 u |c - 0.5| + u max(|c|, |c'|)"""
    a = asset_of("VeryHigh", 20000)
    m = model_of("VeryHigh", 20000)
    r = make_renderer(gpu_ctx, a)
    set_pattern(r, m, "half deleted under cutouts")
    r.m_Cutouts = None; r.UpdateCutoutsBuffer()                    # the delete alone
    m.edit.set_cutouts(None, r.transform.localToWorldMatrix)
    path = str(tmp_path / "rt.ply")
    count = r.ExportPlyFile(path)
    keep = m.alive()
    assert count == int(keep.sum()) == 20000 - 10088
    back = creator.CreateAssetFromSplatsNative(creator.ReadPLYNative(path), "VeryHigh", morton=False)
    got = XM.ExportModel(back).dec
    orig = m.dec[keep]
    assert same_bits(got[:, 0:3], orig[:, 0:3]) and same_bits(got[:, 14:59], orig[:, 14:59])
    u = 2.0 ** -24
    e = lambda x: creator.LOGDET_REL * np.abs(np.log(x)) + creator.LOGDET_ABS
    s, s2 = orig[:, 7:10].astype(np.float64), got[:, 7:10].astype(np.float64)
    assert (s > 0).all() and (np.abs(s2 - s) <= s * (np.exp(e(s)) * (1 + 2.0 ** -22) - 1)).all()
    v, v2 = orig[:, 10].astype(np.float64), got[:, 10].astype(np.float64)
    assert ((v > 1e-4) & (v < 1 - 1e-4)).all()                    # away from the clamp of InvSigmoid and from ExpDet's
    rho = np.exp(2.01 * u + e(v / (1 - v))) * (1 + 2.0 ** -22) - 1
    assert (np.abs(v2 - v) <= v * (1 - v) * rho * (1 + rho) + 2.01 * u * v).all()
    c, c2 = orig[:, 11:14].astype(np.float64), got[:, 11:14].astype(np.float64)
    assert (np.abs(c2 - c) <= 3.01 * u * np.abs(c - 0.5) + u * np.maximum(np.abs(c), np.abs(c2))).all()
    print("round trip: max |ds| / s", float((np.abs(s2 - s) / s).max()), "max |dv|", float(np.abs(v2 - v).max()), "max |dc|", float(np.abs(c2 - c).max()))
    r.DisposeResourcesForAsset()


# ---- 7. with frames in flight ------------------------------------------------------------------------------------------------------------------
def test_export_between_frames_in_flight(gpu_ctx, tmp_path):
    a = asset_of("Medium", 20000)
    m = model_of("Medium", 20000)

    def frames(export_between: bool):
        r = GaussianSplatRenderer(gpu_ctx, a)
        r.sortMode = SortMode.Visible
        r.CreateResourcesForAsset()
        r.SetFramesInFlight(2)
        assert r.FramesInFlight() == (2, True)
        set_pattern(r, m, "half deleted under cutouts")
        rts = [RenderTarget(gpu_ctx, 320, 200) for _ in range(4)]
        outs = None
        for k, rt in enumerate(rts):
            cam = default_camera(az=25.0 + 9.0 * k)
            r.SortPoints(cam); r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
            if export_between and k == 1:
                outs = three_outputs(r, str(tmp_path / "f.ply"))
        imgs = [rt.Download() for rt in rts]
        for rt in rts:
            rt.Dispose()
        r.DisposeResourcesForAsset()
        return imgs, outs

    plain, _ = frames(False)
    imgs, (data, alive, count, blob) = frames(True)
    assert all(np.array_equal(x, y) for x, y in zip(plain, imgs))  # the frames are unchanged
    assert same_bits(data, m.export_data()) and same_bits(alive, m.export_alive()) and count == len(alive)
    want = str(tmp_path / "w.ply")
    creator.WritePLY(want, XM.columns(m.export_alive()))
    with open(want, "rb") as f:
        assert blob == f.read()
