"""The bake on the CPU box: the C-ABI surface of gs_renderer_edit_bake_asset / gs_asset_download_blobs, and the host build of the bake's arithmetic
(tests/bake_host_harness.cpp over csrc/gs_device_math.h: the full decode, gsm::BakeLinearRecord, the chunk encode, the Morton key) against the
yardstick of tests/bake_model.py -- the native importer with linearize = 0 fed with the oracle's decode -- byte for byte: every target format, chunk
sizes 1 / 255 / 256, sources of all five presets; the Morton key against the importer's order, duplicates included; the premise of the degenerate
axis; and the harness as a stand-alone program under the host sanitizers."""
import ctypes as C

import numpy as np
import pytest

import bake_model as BM
from builders import decode_of
from common import PRESETS, small_asset
from harness import build_harness, run_under_sanitizers
from unitygaussiansplatting_amd import _abi, _lib, asset as A, creator, renderer
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuAsset

f32 = np.float32


@pytest.fixture(scope="module")
def bh(tmp_path_factory):
    return C.CDLL(build_harness(tmp_path_factory.mktemp("bh"), "bake_host_harness.cpp"))


def host_bake(bh, asset, src, formats, morton=True) -> A.GaussianSplatAsset:
    """the harness over the splats `src` of the asset, as an asset"""
    keep = []
    desc = _abi.make_asset_desc(asset, keep)
    src = np.ascontiguousarray(src, np.uint32)
    fp, fs, fc, fsh = formats
    fmt = _abi.gs_import_formats(int(fp), int(fs), int(fc), int(fsh), 0, int(morton))
    sizes = (C.c_uint64 * 5)()
    _lib.check(_lib.lib().gs_import_blob_sizes(len(src), C.byref(fmt), sizes), "gs_import_blob_sizes")
    blobs = [np.zeros(int(sz), np.uint8) if sz else None for sz in sizes]
    ptrs = (C.c_void_p * 5)(*[b.ctypes.data if b is not None else None for b in blobs])
    bounds = np.zeros(6, f32)
    four = np.array([int(fp), int(fs), int(fc), int(fsh)], np.uint32)
    bh.bh_bake(C.byref(desc), src.ctypes.data_as(C.c_void_p), C.c_uint32(len(src)), four.ctypes.data_as(C.c_void_p), C.c_uint32(int(morton)), ptrs,
               bounds.ctypes.data_as(C.c_void_p))
    return A.GaussianSplatAsset(splatCount=len(src), posFormat=A.VectorFormat(fp), scaleFormat=A.VectorFormat(fs), shFormat=A.SHFormat(fsh),
                                colorFormat=A.ColorFormat(fc), posData=blobs[0], otherData=blobs[1], colorData=blobs[2], shData=blobs[3], chunkData=blobs[4],
                                boundsMin=tuple(bounds[:3]), boundsMax=tuple(bounds[3:]))


# ---- 1. the ABI and the host layer -----------------------------------------------------------------------------------------------------------
def test_bake_entry_points_validate_their_arguments():
    lib = _lib.lib()
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    fmt = _abi.gs_import_formats(2, 2, 2, 3, 0, 1)
    out, alive = C.c_void_p(0x1234), C.c_uint32(7)
    some = C.create_string_buffer(64)
    assert lib.gs_renderer_edit_bake_asset(None, C.byref(fmt), C.byref(out), C.byref(alive), None, None) == bad
    assert not out and alive.value == 7                          # *out is NULL after a refusal
    out = C.c_void_p(0x1234)
    assert lib.gs_renderer_edit_bake_asset(None, None, C.byref(out), C.byref(alive), None, None) == bad and not out
    assert lib.gs_renderer_edit_bake_asset(some, None, C.byref(out), C.byref(alive), None, None) == bad       # (`some` is never dereferenced)
    assert lib.gs_renderer_edit_bake_asset(some, C.byref(fmt), None, C.byref(alive), None, None) == bad
    assert lib.gs_renderer_edit_bake_asset(some, C.byref(fmt), C.byref(out), None, None, None) == bad
    ptrs, sizes = (C.c_void_p * 5)(), (C.c_uint64 * 5)()
    assert lib.gs_asset_download_blobs(None, ptrs, sizes) == bad
    assert lib.gs_abi_version() == 9                             # additions to ABI 9


def test_renderer_mirrors_the_bake_methods():
    for name in ("EditBakeAsset", "CreateResourcesForGpuAsset", "BakeFormats"):
        assert callable(getattr(GaussianSplatRenderer, name)), name
    for name in ("Download", "Dispose"):
        assert callable(getattr(GpuAsset, name)), name
    r = GaussianSplatRenderer.__new__(GaussianSplatRenderer)       # no context: BakeFormats reads nothing of the renderer
    f = r.BakeFormats()
    assert (f.pos_format, f.scale_format, f.color_format, f.sh_format, f.linearize, f.morton) == (2, 2, 2, 3, 0, 1)
    f = r.BakeFormats("VeryHigh", formatSH=A.SHFormat.Float16, morton=False)
    assert (f.pos_format, f.scale_format, f.color_format, f.sh_format, f.linearize, f.morton) == (0, 0, 0, 1, 0, 0)
    assert renderer.GpuAsset is GpuAsset


# ---- 2. the chunk encode against the importer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alive", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("target", ["Medium", "VeryHigh"])
def test_chunk_sizes(bh, alive, target):
    """a lone splat, a chunk one short of full, a full chunk, a one-splat last chunk, three chunks: every second splat of the source dropped"""
    asset, dec = small_asset(1100, 5, "High"), decode_of(1100, "High")
    src = np.arange(alive, dtype=np.uint32) * 2 + 1
    formats = BM.MEDIUM if target == "Medium" else BM.VERY_HIGH
    BM.assert_same_asset(host_bake(bh, asset, src, formats), BM.yardstick(dec[src], formats), (alive, target))


@pytest.mark.parametrize("k", range(len(BM.FORMAT_TARGETS)))
def test_every_target_format(bh, k):
    formats = BM.FORMAT_TARGETS[k]
    asset, dec = small_asset(600, 5, "VeryHigh"), decode_of(600, "VeryHigh")
    src = np.arange(600, dtype=np.uint32)
    BM.assert_same_asset(host_bake(bh, asset, src, formats), BM.yardstick(dec, formats), formats)
    BM.assert_same_asset(host_bake(bh, asset, src, formats, morton=False), BM.yardstick(dec, formats, morton=False), (formats, "no morton"))


def test_format_targets_cover_the_enums():
    for col, enum, skip in ((0, A.VectorFormat, ()), (1, A.VectorFormat, ()), (2, A.ColorFormat, (A.ColorFormat.BC7,)), (3, A.SHFormat, tuple(f for f in A.SHFormat if f > A.SHFormat.Norm6))):
        assert {t[col] for t in BM.FORMAT_TARGETS} == {f for f in enum if f not in skip}


@pytest.mark.parametrize("quality", PRESETS)
def test_every_source_preset(bh, quality):
    """the first 513 splats of a 20,000-splat asset of each preset (a Cluster palette needs more splats than entries) into Medium"""
    asset, dec = small_asset(20000, 5, quality), decode_of(20000, quality)
    src = np.arange(513, dtype=np.uint32)
    BM.assert_same_asset(host_bake(bh, asset, src, BM.MEDIUM), BM.yardstick(dec[:513], BM.MEDIUM), quality)


# ---- 3. the Morton key ---------------------------------------------------------------------------------------------------------------------------
def importer_order(pos, morton=True) -> np.ndarray:
    """the order the native importer puts the positions in, read off an all-fp32 asset whose scales carry the input index"""
    n = len(pos)
    idx = np.arange(n, dtype=f32) + f32(1.0)
    raw = creator.InputSplatData(pos=np.ascontiguousarray(pos, f32), dc0=np.full((n, 3), 0.5, f32), sh=np.zeros((n, 15, 3), f32), opacity=np.full(n, 0.5, f32),
                                 scale=np.stack([idx, idx, idx], axis=1), rot=np.tile(np.array([0.5, 0.5, 0.5, 1.0], f32), (n, 1)))
    a = creator.CreateAssetFromSplatsNative(raw, "VeryHigh", linearize=False, morton=morton)
    order = a.otherData[:n * 16].view(f32).reshape(n, 4)[:, 1].astype(np.int64) - 1
    assert np.array_equal(a.posData[:n * 12].view(f32).reshape(n, 3), np.asarray(pos, f32)[order])
    return order


def harness_codes(bh, pos) -> np.ndarray:
    pos = np.ascontiguousarray(pos, f32)
    bounds = np.concatenate([pos.min(axis=0), pos.max(axis=0)]).astype(f32)
    codes = np.zeros(len(pos), np.uint64)
    bh.bh_morton(pos.ctypes.data_as(C.c_void_p), C.c_uint32(len(pos)), bounds.ctypes.data_as(C.c_void_p), codes.ctypes.data_as(C.c_void_p))
    assert np.array_equal(codes, BM.morton_codes(pos, bounds[:3], bounds[3:]))      # the numpy restatement the GPU tests' coplanar case orders by
    return codes


def duplicate_positions(n=1000, dup=200, seed=11) -> np.ndarray:
    """n random positions in which `dup` splats, spread over the array, share 3 exact positions"""
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) * 6.0 - 3.0).astype(f32)
    where = rng.permutation(n)[:dup]
    pos[where] = pos[where[:3]][np.arange(dup) % 3]
    return pos


def test_morton_key_orders_like_the_importer(bh):
    rng = np.random.default_rng(7)
    for what, pos in (("random", (rng.random((3000, 3)) * 6.0 - 3.0).astype(f32)), ("duplicates", duplicate_positions())):
        codes = harness_codes(bh, pos)
        if what == "duplicates":
            assert len(np.unique(codes)) <= len(pos) - 197
        assert np.array_equal(np.argsort(codes, kind="stable"), importer_order(pos)), what      # (code, rank): equal codes stay in input order


def coplanar_positions(n=700, seed=13) -> np.ndarray:
    pos = (np.random.default_rng(seed).random((n, 3)) * 4.0 - 2.0).astype(f32)
    pos[:, 1] = f32(0.75)                                          # one axis constant: max == min, 0 x inf
    return pos


def test_premise_degenerate_axis(bh):
    """On a coplanar cloud the importer's own Morton component is (uint)(NaN), which C++ leaves undefined.  The bake defines it as 0.  The GPU
    coplanar case stands on this host build giving the same: the importer's order = the model's order with that component forced to 0."""
    pos = coplanar_positions()
    codes = harness_codes(bh, pos)
    assert ((codes >> np.uint64(1)) & np.uint64(1)).max() == 0     # no y bit anywhere
    want = np.argsort(codes, kind="stable")
    assert np.array_equal(importer_order(pos), want)
    assert np.array_equal(importer_order(pos[want], morton=False), np.arange(len(pos)))


# ---- 4. the harness as a stand-alone program under the host sanitizers ---------------------------------------------------------------------------
def test_stand_alone_harness_runs_clean_under_the_host_sanitizers(tmp_path):
    out = run_under_sanitizers(tmp_path, "bake_host_harness.cpp", "BAKE_HARNESS_MAIN")
    assert out.returncode == 0 and "bake harness ok" in out.stdout, (out.stdout, out.stderr[-2000:])
