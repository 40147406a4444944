"""The bake to a Cluster* SH target on the CPU box: the host build of what it adds to csrc/gs_device_math.h (tests/bake_cluster_host_harness.cpp: the SH
rows the palette is computed from, gsm::BakeEmitOther's 8 / 10 / 12 / 18-byte `other` record, gsm::BakeEmitSHTableItem, the chunk encode that writes no
SH item) with the palette of gs_import_cluster_shs' host route in between -- the steps of the GPU bake, one for one -- against the yardstick of
tests/bake_model.py, the native importer, byte for byte; and the harness as a stand-alone program under the host sanitizers."""
import ctypes as C
import functools

import numpy as np
import pytest

import bake_model as BM
import copy_model as CM
from common import small_asset
from harness import build_harness, run_under_sanitizers
from unitygaussiansplatting_amd import _abi, _lib, asset as A, creator

f32 = np.float32
N = 4500
VF, CF, SF = A.VectorFormat, A.ColorFormat, A.SHFormat


@pytest.fixture(scope="module")
def bch(tmp_path_factory):
    lib = C.CDLL(build_harness(tmp_path_factory.mktemp("bch"), "bake_cluster_host_harness.cpp"))
    lib.bch_other.restype = C.c_uint32
    return lib


@functools.lru_cache(maxsize=None)
def source():
    asset = small_asset(N, 5, "VeryHigh")
    dec = CM.decode(asset)
    dec.setflags(write=False)
    return asset, dec


@functools.lru_cache(maxsize=None)
def palette_of(bch, morton: bool):
    """the rows in destination order and their Cluster4k palette: one per order, shared by the formats"""
    asset, _ = source()
    keep = []
    desc = _abi.make_asset_desc(asset, keep)
    src = np.arange(N, dtype=np.uint32)
    rows = np.zeros((N, 45), f32)
    bch.bch_sh_rows(C.byref(desc), src.ctypes.data_as(C.c_void_p), C.c_uint32(N), C.c_uint32(int(morton)), rows.ctypes.data_as(C.c_void_p))
    means, index = creator.ClusterSHsNative(rows, 4096)
    return rows, means, index


def host_bake(bch, formats, morton) -> A.GaussianSplatAsset:
    asset, _ = source()
    _, means, index = palette_of(bch, morton)
    keep = []
    desc = _abi.make_asset_desc(asset, keep)
    src = np.arange(N, dtype=np.uint32)
    fp, fs, fc, fsh = formats
    fmt = _abi.gs_import_formats(int(fp), int(fs), int(fc), int(fsh), 0, int(morton))
    sizes = (C.c_uint64 * 5)()
    _lib.check(_lib.lib().gs_import_blob_sizes(N, C.byref(fmt), sizes), "gs_import_blob_sizes")
    blobs = [np.zeros(int(sz), np.uint8) for sz in sizes]
    ptrs = (C.c_void_p * 5)(*[b.ctypes.data for b in blobs])
    bounds = np.zeros(6, f32)
    four = np.array([int(fp), int(fs), int(fc), int(fsh)], np.uint32)
    bch.bch_bake(C.byref(desc), src.ctypes.data_as(C.c_void_p), C.c_uint32(N), four.ctypes.data_as(C.c_void_p), C.c_uint32(int(morton)),
                 means.ctypes.data_as(C.c_void_p), C.c_uint32(len(means)), index.ctypes.data_as(C.c_void_p), ptrs, bounds.ctypes.data_as(C.c_void_p))
    return A.GaussianSplatAsset(splatCount=N, posFormat=VF(fp), scaleFormat=VF(fs), shFormat=SF(fsh), colorFormat=CF(fc), posData=blobs[0], otherData=blobs[1],
                                colorData=blobs[2], shData=blobs[3], chunkData=blobs[4], boundsMin=tuple(bounds[:3]), boundsMax=tuple(bounds[3:]))


def test_rows_are_the_decoded_sh_in_index_order(bch):
    rows, _, _ = palette_of(bch, False)
    assert np.array_equal(rows.view(np.uint32), np.ascontiguousarray(source()[1][:, 14:59]).view(np.uint32))
    assert np.isfinite(rows).all()


@pytest.mark.parametrize("scale,record", [(VF.Norm6, 8), (VF.Norm11, 10), (VF.Norm16, 12), (VF.Float32, 18)])
def test_every_other_record_size(bch, scale, record):
    """4,500 VeryHigh splats into Norm11 / scale / Norm8x4 / Cluster4k: the `other` record of 8, 10, 12 and 18 bytes, the table, no SH item"""
    formats = (VF.Norm11, scale, CF.Norm8x4, SF.Cluster4k)
    got = host_bake(bch, formats, True)
    assert len(got.otherData) == (N * record + 7) // 8 * 8 and len(got.shData) == 4096 * 96
    BM.assert_same_asset(got, BM.yardstick(source()[1], formats), formats)


def test_without_the_morton_order(bch):
    formats = (VF.Norm11, VF.Norm6, CF.Norm8x4, SF.Cluster4k)
    BM.assert_same_asset(host_bake(bch, formats, False), BM.yardstick(source()[1], formats, morton=False), "morton = 0")


def test_other_record_words(bch):
    """the record on its own: the index is the halfword right behind the scale, whichever half of a word that is, and touches nothing else"""
    scale = np.array([0.3, 0.6, 0.9], f32)
    for fmt, size in ((0, 12), (1, 6), (2, 4), (3, 2)):
        plain, with_index = np.zeros(20, np.uint8), np.zeros(20, np.uint8)
        assert bch.bch_other(C.c_uint32(0x89abcdef), scale.ctypes.data_as(C.c_void_p), C.c_uint32(fmt), C.c_uint32(0), C.c_uint32(0xffff), plain.ctypes.data_as(C.c_void_p)) == 4 + size
        assert bch.bch_other(C.c_uint32(0x89abcdef), scale.ctypes.data_as(C.c_void_p), C.c_uint32(fmt), C.c_uint32(1), C.c_uint32(0x1a2b3), with_index.ctypes.data_as(C.c_void_p)) == 6 + size
        assert np.array_equal(plain[:4 + size], with_index[:4 + size]) and plain[:4].view(np.uint32)[0] == 0x89abcdef
        assert not plain[4 + size:].any() and not with_index[6 + size:].any()
        assert with_index[4 + size:6 + size].view(np.uint16)[0] == 0xa2b3          # the low 16 bits of the index


def test_stand_alone_harness_runs_clean_under_the_host_sanitizers(tmp_path):
    out = run_under_sanitizers(tmp_path, "bake_cluster_host_harness.cpp", "BAKE_CLUSTER_HARNESS_MAIN")
    assert out.returncode == 0 and "bake cluster harness ok" in out.stdout, (out.stdout, out.stderr[-2000:])
