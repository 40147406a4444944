"""The SPZ export on the GPU (csrc/gs_export.hip: the alive list and its bounds, then export_spz, through gs_renderer_edit_export_spz_body,
gs_renderer_edit_export_spz and GaussianSplatRenderer.ExportSpzBody / ExportSpzFile).  The expected body is always the numpy packer
(tests/spz_export_model.py) over ExportModel.export_alive plus the decoded linear opacity of the same splats, and equality is exact.  The bytes of
gzip are never compared: a file is gunzipped with Python's gzip and its body compared.  A lane is an object the C ABI never hands out, so its refusal
cannot be provoked from outside the library; the 10,000,000 cap is held on the CPU (tests/test_spz_export_model.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import crafted
import edit_model as EM
import export_model as XM
import spz_export_model as SM
from common import PRESETS, same_bits, small_asset
from gpu_rig import BAD, frame_of, make_renderer
from unitygaussiansplatting_amd import _lib, camera, creator, scenes
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

pytestmark = pytest.mark.gpu
f32 = np.float32
AUTO = None
FIELDS = ("pos", "dc0", "sh", "opacity", "scale", "rot")


@functools.lru_cache(maxsize=None)
def asset_of(kind: str, n: int):
    if kind == "points":
        return EM.point_asset(n)
    if kind == "Low":                                              # Cluster16k: the native importer builds the palette in a fraction of the numpy one's time
        return creator.CreateAssetFromSplatsNative(scenes.make_splats(n, 5, 3.0), "Low")
    return small_asset(n, 5, kind)


@functools.lru_cache(maxsize=None)
def model_of(kind: str, n: int) -> XM.ExportModel:
    """one model (one oracle decode) per asset, shared by the tests that use the asset; every test leaves it without deleted bits and cutouts"""
    return XM.ExportModel(asset_of(kind, n))


def set_pattern(r, m, name):
    words, cuts = XM.pattern(name, m.n)
    r.SetDeletedBits(words)
    r.m_Cutouts = cuts
    r.UpdateCutoutsBuffer()
    XM.apply_pattern(m, name, r.transform.localToWorldMatrix)


def want_body(m, r, bake=False, sh_level=3, fract=AUTO):
    """(body, fract_bits) of the model: the packer over the alive export records and the linear opacity the decode gives those splats"""
    return SM.body(m.export_alive(r.transform, bake), m.dec[m.alive(), 10], sh_level, fract)


def check_body(r, m, what, bake=False, sh_level=3, fract=AUTO, slice_bytes=0):
    want, f = want_body(m, r, bake, sh_level, fract)
    got, alive, used = r.ExportSpzBody(bake, sh_level, fract, slice_bytes)
    assert alive == int(m.alive().sum()) and used == f, (what, alive, used, f)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (what, len(got), len(want), np.flatnonzero(got[:len(want)] != want[:len(got)])[:8])
    return got


def check_ply_exports_unchanged(r, m, tmp_path, bake=False):
    """EditExportData / ExportPlyFile of the same renderer still give the existing model's bits"""
    assert same_bits(r.EditExportData(bake), m.export_data(r.transform, bake))
    path, ref = str(tmp_path / "after.ply"), str(tmp_path / "after_want.ply")
    want = m.export_alive(r.transform, bake)
    assert r.ExportPlyFile(path, bake) == len(want)
    creator.WritePLY(ref, XM.columns(want))
    with open(path, "rb") as a, open(ref, "rb") as b:
        assert a.read() == b.read()


def refused(r, path=None, bake=False, **kw):
    """the body call and the file call both answer GS_ERR_INVALID_ARGUMENT; the file call leaves no file"""
    p, s = r.ExportParams(bake), r.SpzParams(**kw)
    size, alive, fract = C.c_uint64(7), C.c_uint32(7), C.c_uint32(7)
    lib = _lib.lib()
    assert lib.gs_renderer_edit_export_spz_body(r._r_h, C.byref(p), C.byref(s), None, 0, C.byref(size), C.byref(alive), C.byref(fract)) == BAD
    assert (size.value, alive.value, fract.value) == (7, 7, 7)
    if path is not None:
        assert lib.gs_renderer_edit_export_spz(r._r_h, C.byref(p), C.byref(s), os.fsencode(path), C.byref(alive)) == BAD
        assert alive.value == 7 and not os.path.exists(path)
    return True


# ---- 1. alive counts at every seam, every pattern ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 256, 257, 513])
def test_alive_counts_at_every_seam(gpu_ctx, tmp_path, n):
    """n mod 4 != 0 (the column bases are unaligned in the file), a partial wave, a partial workgroup; fp32 and chunk-less below 255, Medium from there"""
    m = model_of("points" if n < 255 else "Medium", n)
    r = make_renderer(gpu_ctx, m.edit.asset)
    try:
        for name in XM.PATTERNS:
            set_pattern(r, m, name)
            left = int(m.alive().sum())
            path = str(tmp_path / "seam.spz")
            assert left == 0 or name not in ("everything deleted", "everything cut")
            if left == 0:                                          # the two patterns that leave nothing (and, at the smallest sizes, a half that is everything)
                assert refused(r, path), (n, name)
                continue
            body = check_body(r, m, (n, name))
            assert r.ExportSpzFile(path, level=1) == left
            assert np.array_equal(SM.read_gzip(path), body), (n, name)
            os.remove(path)
            if name == "nothing deleted":
                assert left == n and len(body) == 16 + 64 * n
        set_pattern(r, m, "half deleted under cutouts")
        check_ply_exports_unchanged(r, m, tmp_path)
    finally:
        set_pattern(r, m, "nothing deleted")
        r.DisposeResourcesForAsset()


# ---- 2. every preset as the source, every SH level, every kind of fract_bits ---------------------------------------------------------------------------
SMALLEST = {"VeryLow": 4500, "Low": 16500, "Medium": 300, "High": 300, "VeryHigh": 300}      # a Cluster* palette needs more splats than entries


@pytest.mark.parametrize("quality", PRESETS)
def test_every_preset_as_the_source(gpu_ctx, quality):
    m = model_of(quality, SMALLEST[quality])
    r = make_renderer(gpu_ctx, m.edit.asset)
    try:
        set_pattern(r, m, "half deleted under cutouts")
        assert 0 < m.alive().sum() < m.n
        for sh_level in range(4):
            for fract in (0, 12, 24, AUTO):
                check_body(r, m, (quality, sh_level, fract), sh_level=sh_level, fract=fract)
        set_pattern(r, m, "nothing deleted")
        check_body(r, m, (quality, "all"))
    finally:
        set_pattern(r, m, "nothing deleted")
        r.DisposeResourcesForAsset()


# ---- 3. values that clamp in every column -----------------------------------------------------------------------------------------------------------------
def clamping_asset(n=200):
    """fp32, chunk-less: positions beyond +-2^23 / 2^f for every f tried, scales outside e^-10 .. e^5.94 (and 0: the log is -inf), colour and SH far out
    of range (NaN and the infinities among the SH), opacity 0, 1 and beyond, rotations of every sign of w"""
    rng = np.random.default_rng(21)
    pos = (rng.normal(0, 1.0, (n, 3)) * 10.0 ** rng.uniform(-3, 8, (n, 1))).astype(f32)
    pos[:6] = [[8388607.0, -8388608.0, 8388608.0], [-8388609.0, 2047.99, -2048.0], [0.5, 1.5, -0.5], [1e30, -1e30, 0.0], [511.99997, 512.0, -512.0], [0.0, -0.0, 1e-30]]
    scale = np.exp(rng.uniform(-14, 9, (n, 3))).astype(f32)
    scale[:4] = [[0.0, np.exp(-10.0), np.exp(5.94)], [1e-30, 1e30, 1.0], [4.5e-5, 4.6e-5, 380.0], [379.0, 381.0, 3.0e38]]
    rgb = rng.uniform(-3.0, 4.0, (n, 3)).astype(f32)
    opacity = rng.uniform(-0.5, 1.5, n).astype(f32)
    opacity[:6] = [0.0, 1.0, 0.5, 1.0 / 255.0 * 0.5, 254.5 / 255.0, 2.0]
    rot = rng.normal(0, 1, (n, 4)).astype(f32)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    a = crafted.asset(pos, scale, rot, rgb, opacity)
    sh = rng.uniform(-2.5, 2.5, (n, 48)).astype(f32)
    sh[:5, :6] = [[np.nan, np.inf, -np.inf, 1.0, -1.0, 0.99609375], [127.5 / 128.0 - 1.0, -127.5 / 128.0, 0.0, -0.0, 1e-30, 3.0e38]] + [[0.0] * 6] * 3
    a.shData = sh.view(np.uint8).reshape(-1).copy()
    return a


def test_values_that_clamp_in_every_column(gpu_ctx):
    a = clamping_asset()
    m = XM.ExportModel(a)
    r = make_renderer(gpu_ctx, a)
    try:
        for fract in (0, 12, 24, AUTO):
            body = check_body(r, m, ("clamps", fract), fract=fract)
        assert want_body(m, r)[1] == 0                             # positions beyond 2^23: the automatic choice has nowhere to go
        cols = SM.split(body, m.n, 3)
        for c in (1, 2, 3, 5):
            assert cols[c].min() == 0 and cols[c].max() == 255     # both clamps of every 8-bit column are reached
        codes = cols[0].reshape(m.n, 3, 3).astype(np.int64)
        codes = codes[..., 0] | (codes[..., 1] << 8) | (codes[..., 2] << 16)
        assert (codes == 0x7fffff).any() and (codes == 0x800000).any()
    finally:
        r.DisposeResourcesForAsset()


# ---- 4. the baked transform ---------------------------------------------------------------------------------------------------------------------------------
def test_baked_transform(gpu_ctx, tmp_path):
    m = model_of("Medium", 513)
    for kw, f_baked in ((XM.BAKE_TRANSFORM, 12), (dict(XM.BAKE_TRANSFORM, scale=(-2500.0, 750.0, 1500.0)), None)):
        tr = camera.Transform(**kw)                                # rotated, non-uniformly scaled, mirrored in x
        r = make_renderer(gpu_ctx, m.edit.asset, tr)
        try:
            set_pattern(r, m, "one chunk deleted")              # 257 alive: the cutouts of the other patterns move with the renderer's matrix
            for sh_level in (0, 3):
                for fract in (AUTO, 12):
                    check_body(r, m, ("baked", sh_level, fract), bake=True, sh_level=sh_level, fract=fract)
            plain, baked = want_body(m, r, False), want_body(m, r, True)
            assert plain[1] == 12 and not np.array_equal(plain[0], baked[0])
            if f_baked is None:
                assert baked[1] < 12                               # the bounds are those of the positions AS EXPORTED: the scaled ones need more integer bits
            check_body(r, m, "unbaked")
            check_ply_exports_unchanged(r, m, tmp_path, bake=True)
        finally:
            set_pattern(r, m, "nothing deleted")
            r.DisposeResourcesForAsset()


# ---- 5. the file ----------------------------------------------------------------------------------------------------------------------------------------------
def same_splats(a, b) -> bool:
    return all(same_bits(getattr(a, name), getattr(b, name)) for name in FIELDS)


def test_the_file_in_slices(gpu_ctx, tmp_path):
    """about 2,000 alive splats at SH level 3 with slice_bytes = 4096: the 90 KB SH column spans 22 slices, every other column more than one"""
    m = model_of("Medium", 2300)
    r = make_renderer(gpu_ctx, m.edit.asset)
    try:
        set_pattern(r, m, "one chunk deleted")
        left = int(m.alive().sum())
        assert left == 2044
        for sh_level, level in ((3, -1), (0, 0), (1, 9), (2, 1)):
            path = str(tmp_path / f"out{sh_level}.spz")
            assert r.ExportSpzFile(path, shLevel=sh_level, level=level, sliceBytes=4096) == left
            body = check_body(r, m, ("file", sh_level), sh_level=sh_level, slice_bytes=4096)
            assert np.array_equal(SM.read_gzip(path), body)        # == export_spz_body == the model
            assert np.array_equal(check_body(r, m, ("one slice", sh_level), sh_level=sh_level), body)
            if sh_level in (1, 2):
                continue                                           # held by their bytes: the readers' run-on past 3k bytes is not the writer's concern
            native, numpy_reader = creator.ReadSPZNative(path), creator.ReadSPZ(path)
            assert len(numpy_reader) == left and same_splats(native, numpy_reader)
            ref = str(tmp_path / f"want{sh_level}.spz")
            SM.write_gzip(ref, want_body(m, r, sh_level=sh_level)[0])
            assert same_splats(numpy_reader, creator.ReadSPZ(ref))
            if sh_level == 3:
                g = creator.CreateGpuAssetFromFile(path, "Medium", context=gpu_ctx)
                r1 = GaussianSplatRenderer(gpu_ctx)
                try:
                    r1.CreateResourcesForGpuAsset(g)
                    assert r1.splatCount == left
                    assert frame_of(r1, gpu_ctx)[2].any()              # a renderer draws it
                finally:
                    r1.DisposeResourcesForAsset(); g.Dispose()
        check_ply_exports_unchanged(r, m, tmp_path)
    finally:
        set_pattern(r, m, "nothing deleted")
        r.DisposeResourcesForAsset()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_no_file_and_a_usable_renderer(gpu_ctx, tmp_path):
    m = model_of("Medium", 513)
    r = make_renderer(gpu_ctx, m.edit.asset)
    lib = _lib.lib()
    path = str(tmp_path / "refused.spz")
    try:
        set_pattern(r, m, "half deleted under cutouts")
        for kw in (dict(shLevel=4), dict(fractBits=25), dict(fractBits=0xfffffffe), dict(level=-2), dict(level=10), dict(sliceBytes=1), dict(sliceBytes=4095)):
            assert refused(r, path, **kw), kw
        p, s = r.ExportParams(False), r.SpzParams()
        size, alive, fract = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        for args in ((None, C.byref(p), C.byref(s)), (r._r_h, None, C.byref(s)), (r._r_h, C.byref(p), None)):
            assert lib.gs_renderer_edit_export_spz_body(*args, None, 0, C.byref(size), C.byref(alive), C.byref(fract)) == BAD
            assert lib.gs_renderer_edit_export_spz(*args, os.fsencode(path), C.byref(alive)) == BAD and not os.path.exists(path)
        assert lib.gs_renderer_edit_export_spz(r._r_h, C.byref(p), C.byref(s), None, C.byref(alive)) == BAD
        # a too-small buffer: nothing is written into it
        want, _ = want_body(m, r)
        assert lib.gs_renderer_edit_export_spz_body(r._r_h, C.byref(p), C.byref(s), None, 0, C.byref(size), C.byref(alive), C.byref(fract)) == 0
        assert (size.value, alive.value, fract.value) == (len(want), int(m.alive().sum()), 12)
        buf = np.full(len(want), 0xa5, np.uint8)
        assert lib.gs_renderer_edit_export_spz_body(r._r_h, C.byref(p), C.byref(s), buf.ctypes.data, len(want) - 1, C.byref(size), C.byref(alive), C.byref(fract)) == BAD
        assert (buf == 0xa5).all()
        assert lib.gs_renderer_edit_export_spz_body(r._r_h, C.byref(p), C.byref(s), buf.ctypes.data, len(want), C.byref(size), C.byref(alive), C.byref(fract)) == 0
        assert np.array_equal(buf, want)
        # a path that cannot be created
        assert lib.gs_renderer_edit_export_spz(r._r_h, C.byref(p), C.byref(s), b"/nonexistent-directory/x.spz", C.byref(alive)) == BAD
        # nothing alive
        for name in ("everything deleted", "everything cut"):
            set_pattern(r, m, name)
            assert refused(r, path), name
        set_pattern(r, m, "only the last alive")
        assert r.ExportSpzFile(path) == 1 and np.array_equal(SM.read_gzip(path), check_body(r, m, "one alive"))
        check_ply_exports_unchanged(r, m, tmp_path)
    finally:
        set_pattern(r, m, "nothing deleted")
        r.DisposeResourcesForAsset()
