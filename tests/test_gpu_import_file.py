"""A PLY or SPZ file straight into a device asset (gs_splat_file_open + gs_import_file_to_asset through creator.CreateGpuAssetFromFile: the sources
BakePlyRowsSource / BakeSpzSource of csrc/gs_bake.hip read the file's own bytes) against the host route over the same file --
creator.CreateAssetFromSplatsNative(ReadPLYNative | ReadSPZNative, linearize = PLY): the five blobs of GpuAsset.Download() byte for byte and the
bounds bit for bit, for every PLY layout a reader may meet, sizes around a chunk, slices that cut rows, every preset through both kinds, and SPZ files
of every SH level.  The importer suites' premises (finite values, no -0 among the extremes) are asserted on every input."""
import ctypes as C

import numpy as np
import pytest

import file_cases as FC
from common import small_asset
from gpu_rig import BAD, frame_of, pinned_renderer as make_renderer, same_frame
from unitygaussiansplatting_amd import _abi, _lib, asset as A, creator, scenes
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

pytestmark = pytest.mark.gpu
SF = A.SHFormat
MEDIUM = dict(quality="Medium")
PRESETS = {
    "VeryHigh": (700, dict(quality="VeryHigh")),
    "High": (700, dict(quality="High")),
    "Medium": (700, MEDIUM),
    "VeryLow": (4500, dict(quality="VeryLow")),                     # BC7 colour + the Cluster4k palette
    "LowCluster4k": (4500, dict(quality="Low", formatSH=SF.Cluster4k)),
}


def splats(n):
    return scenes.make_splats(n, 400 + n, 3.0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """path of the PLY (by layout) or SPZ (by level and fractional bits) of splats(n), each written once"""
    root, made = tmp_path_factory.mktemp("files"), {}

    def get(n, kind="inria", sh_level=3, fract_bits=12):
        key = (n, kind, sh_level, fract_bits)
        if key not in made:
            if kind == "spz":
                made[key] = str(root / f"{n}_{sh_level}_{fract_bits}.spz")
                creator.WriteSPZ(made[key], splats(n), fract_bits=fract_bits, sh_level=sh_level)
            else:
                made[key] = str(root / f"{n}_{kind}.ply")
                FC.write_ply(made[key], splats(n), kind=kind)
        return made[key]
    return get


# ---- 1. PLY layouts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FC.LAYOUTS)
def test_ply_layouts(gpu_ctx, files, kind):
    path = files(700, kind)
    _, _, info = FC.open_result(path)
    assert info.stride == {"inria": 248, "shuffled": 248, "no_rest": 68, "rest9": 104, "uchar": 249, "double_int": 256, "crlf": 248}[kind]
    FC.check_file(gpu_ctx, path, kind, **MEDIUM)


# ---- 2. sizes around a chunk, dword and byte path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["inria", "uchar"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sizes(gpu_ctx, files, n, kind):
    FC.check_file(gpu_ctx, files(n, kind), (n, kind), **MEDIUM)


# ---- 3. slices that cut rows ---------------------------------------------------------------------------------------------------------------------------
def test_small_slices(gpu_ctx, files):
    """700 rows of 249 bytes through slices of 4,096: 43 slices, a row across every boundary; the same bytes as through one slice"""
    path = files(700, "uchar")
    assert 700 * 249 // 4096 + 1 == 43 and all((k * 4096) % 249 for k in range(1, 43))
    want = FC.check_file(gpu_ctx, path, "one slice", slice_bytes=0, **MEDIUM)
    FC.check_file(gpu_ctx, path, "43 slices", slice_bytes=4096, want=want, **MEDIUM)
    FC.check_file(gpu_ctx, path, "slices of 4099", slice_bytes=4099, want=want, **MEDIUM)
    FC.check_file(gpu_ctx, files(700), "dword path, 43 slices", slice_bytes=4096, **MEDIUM)


# ---- 4. every preset through both kinds -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("morton", [True, False])
@pytest.mark.parametrize("kind", ["inria", "spz"])
@pytest.mark.parametrize("preset", list(PRESETS))
def test_presets(gpu_ctx, files, preset, kind, morton):
    n, fmt = PRESETS[preset]
    FC.check_file(gpu_ctx, files(n, kind), (preset, kind, morton), morton=morton, **fmt)


def test_very_low_through_the_byte_path(gpu_ctx, files):
    FC.check_file(gpu_ctx, files(4500, "uchar"), "VeryLow, stride 249", quality="VeryLow")


# ---- 5. SPZ ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fract_bits", [0, 12, 24])
@pytest.mark.parametrize("sh_level", [0, 1, 2, 3])
def test_spz_levels(gpu_ctx, files, sh_level, fract_bits):
    FC.check_file(gpu_ctx, files(300, "spz", sh_level, fract_bits), (sh_level, fract_bits), **MEDIUM)


def test_spz_of_one_splat(gpu_ctx, files):
    for sh_level in (0, 1, 3):
        FC.check_file(gpu_ctx, files(1, "spz", sh_level, 12), ("one splat", sh_level), **MEDIUM)


@pytest.mark.parametrize("sh_level", [3, 1])
def test_spz_crafted_columns(gpu_ctx, tmp_path, sh_level):
    """4,096 points whose scale, colour and alpha columns run through all 256 bytes, positions and rotations starting with the host harness's corner
    cases (tests/test_splat_file_model.py)"""
    path = str(tmp_path / "crafted.spz")
    FC.write_stream(path, FC.crafted_spz_stream(4096, sh_level, 12, seed=8))
    FC.check_file(gpu_ctx, path, ("crafted", sh_level), **MEDIUM)
    FC.check_file(gpu_ctx, path, ("crafted VeryHigh", sh_level), morton=False, quality="VeryHigh")


# ---- 6. a renderer over the asset -----------------------------------------------------------------------------------------------------------------------------
def test_renderer_over_an_asset_from_a_file(gpu_ctx, files):
    path = files(4500)
    host = FC.host_route(path, quality="VeryLow")
    g = creator.CreateGpuAssetFromFile(path, "VeryLow", context=gpu_ctx)
    r0 = make_renderer(gpu_ctx, host)
    r1 = GaussianSplatRenderer(gpu_ctx)
    try:
        r1.sortMode, r1.framesInFlight = r0.sortMode, r0.framesInFlight
        r1.CreateResourcesForGpuAsset(g)
        assert r1.splatCount == r0.splatCount == 4500
        a, b = frame_of(r1, gpu_ctx), frame_of(r0, gpu_ctx)
        assert same_frame(a, b) and a[2].any()
    finally:
        r1.DisposeResourcesForAsset(); r0.DisposeResourcesForAsset(); g.Dispose()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(gpu_ctx, files, tmp_path):
    lib = _lib.lib()
    ply, spz = files(700), files(300, "spz")
    hp, hs, closed = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for path, h in ((ply, hp), (spz, hs), (ply, closed)):
        assert lib.gs_splat_file_open(path.encode(), C.byref(h), None) == 0
    assert lib.gs_splat_file_close(closed) == 0
    other = make_renderer(gpu_ctx, small_asset(700, 5, "Medium"))
    try:
        before = frame_of(other, gpu_ctx)
        c = gpu_ctx._h
        F = _abi.gs_import_formats
        cases = [(None, hp, F(2, 2, 2, 3, 1, 1), 0), (c, None, F(2, 2, 2, 3, 1, 1), 0), (c, closed, F(2, 2, 2, 3, 1, 1), 0), (c, hp, None, 0),
                 (c, hp, F(2, 2, 2, 3, 0, 1), 0), (c, hs, F(2, 2, 2, 3, 1, 1), 0), (c, hp, F(2, 2, 2, 3, 2, 1), 0),       # linearize of the wrong kind
                 (c, hp, F(2, 2, 2, 3, 1, 1), 4095), (c, hp, F(2, 2, 2, 3, 1, 1), 1), (c, hs, F(2, 2, 2, 3, 0, 1), 100),      # slice_bytes below 4096
                 (c, hp, F(2, 2, 2, 3, 1, 2), 0), (c, hp, F(4, 2, 2, 3, 1, 1), 0), (c, hp, F(2, 2, 2, 9, 1, 1), 0),
                 (c, hp, F(2, 2, 2, int(SF.Cluster4k), 1, 1), 0)]                                                             # 700 splats, 4,096 entries
        for ctx_h, h, f, slice_bytes in cases:
            out = C.c_void_p(0x1234)
            rc = lib.gs_import_file_to_asset(ctx_h, h, C.byref(f) if f is not None else None, slice_bytes, C.byref(out), None, None)
            assert rc == BAD and not out, (slice_bytes, rc)
        assert lib.gs_import_file_to_asset(c, hp, C.byref(F(2, 2, 2, 3, 1, 1)), 0, None, None, None) == BAD
        # a file either reader refuses: the reader's error through the Python entry
        for _, bad_path in FC.refused_ply_files(tmp_path, splats(300))[:3] + FC.refused_spz_files(tmp_path, splats(300))[:3]:
            rc, text, _ = FC.reader_result(bad_path)
            with pytest.raises(_lib.GsError) as e:
                creator.CreateGpuAssetFromFile(bad_path, context=gpu_ctx)
            assert e.value.code == rc and text.decode() in str(e.value)
        # the handles that were refused still import, twice each: a handle may be read again
        for h, f, n in ((hp, F(2, 2, 2, 3, 1, 1), 700), (hs, F(2, 2, 2, 3, 0, 1), 300), (hp, F(2, 2, 2, 3, 1, 1), 700)):
            out, cnt = C.c_void_p(), C.c_uint32()
            assert lib.gs_import_file_to_asset(c, h, C.byref(f), 4096, C.byref(out), None, None) == 0 and out
            assert lib.gs_asset_splat_count(out, C.byref(cnt)) == 0 and cnt.value == n
            assert lib.gs_asset_destroy(out) == 0
        FC.check_file(gpu_ctx, ply, "after the refusals", **MEDIUM)
        assert same_frame(frame_of(other, gpu_ctx), before)
    finally:
        other.DisposeResourcesForAsset()
        assert lib.gs_splat_file_close(hp) == 0 and lib.gs_splat_file_close(hs) == 0


def test_a_file_cut_short_after_it_was_opened(gpu_ctx, tmp_path):
    """the rows are there at gs_splat_file_open and gone at the import: the reader's "fewer data bytes" error, and the next import succeeds"""
    lib = _lib.lib()
    path = str(tmp_path / "shrinking.ply")
    FC.write_ply(path, splats(700))
    h = C.c_void_p()
    assert lib.gs_splat_file_open(path.encode(), C.byref(h), None) == 0
    try:
        data = open(path, "rb").read()
        open(path, "wb").write(data[:-100 * 248])
        out = C.c_void_p(0x1234)
        f = _abi.gs_import_formats(2, 2, 2, 3, 1, 1)
        assert lib.gs_import_file_to_asset(gpu_ctx._h, h, C.byref(f), 4096, C.byref(out), None, None) == _abi.GS_ERR_INVALID_ASSET and not out
        assert b"fewer data bytes" in lib.gs_last_error_string()
        open(path, "wb").write(data)
        FC.check_file(gpu_ctx, path, "after the short read", **MEDIUM)
    finally:
        assert lib.gs_splat_file_close(h) == 0
