"""The GPU import on the CPU box: the host build of its arithmetic (tests/import_gpu_host_harness.cpp over csrc/gs_device_math.h: gsm::ImportExpDet,
gsm::ImportLinearize, gsm::ImportRecord, the BC7 mode-6 block encoder gsm::BC7* as one thread per block and as sixteen lanes per block, and the whole
pipeline run serially, on friendly input and on the twelve adversarial inputs that tests/test_gpu_import_edges.py gives the GPU) against the native
importer of the built library (gs_import_encode), byte for byte; the C-ABI surface of
gs_import_encode_to_asset; and the harness as a stand-alone program under the host sanitizers."""
import ctypes as C

import numpy as np
import pytest

import bake_model as BM
from builders import (BC7_TARGET, EDGE_FORMATS, EDGE_SEEDS, assert_import_premises, bc7_block_offset_of_splat, bc7_texel_of_lane, crafted_blocks, edge_case,
                      importer_blocks, linear_input)
from common import _p
from harness import build_harness, run_under_sanitizers
from unitygaussiansplatting_amd import _abi, _lib, asset as A, creator, scenes

f32 = np.float32
VF, CF, SF = A.VectorFormat, A.ColorFormat, A.SHFormat


class ImportSrc(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("pos", "dc0", "sh", "opacity", "scale", "rot")]


@pytest.fixture(scope="module")
def igh(tmp_path_factory):
    lib = C.CDLL(build_harness(tmp_path_factory.mktemp("igh"), "import_gpu_host_harness.cpp"))
    lib.igh_bc7_block_of_splat.restype = C.c_uint64
    lib.igh_bc7_texel_of_lane.restype = C.c_uint32
    return lib


def arrays_of(raw):
    n = len(raw)
    return [np.ascontiguousarray(a, f32) for a in (raw.pos, raw.dc0, np.asarray(raw.sh).reshape(n, 45), raw.opacity, raw.scale, raw.rot)]


def src_of(arrs) -> ImportSrc:
    return ImportSrc(*[a.ctypes.data for a in arrs])


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_validates_its_arguments_without_a_device():
    lib = _lib.lib()
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    fmt = _abi.gs_import_formats(2, 2, 2, 3, 1, 1)
    arrs = arrays_of(scenes.make_splats(16, 3, 1.0))
    inp = _abi.gs_import_input(16, *[a.ctypes.data for a in arrs])
    some = C.create_string_buffer(64)                            # never dereferenced: every refusal below comes first
    out = C.c_void_p(0x1234)
    assert lib.gs_import_encode_to_asset(None, C.byref(inp), 0, C.byref(fmt), C.byref(out), None, None) == bad and not out
    out = C.c_void_p(0x1234)
    assert lib.gs_import_encode_to_asset(some, None, 0, C.byref(fmt), C.byref(out), None, None) == bad and not out
    out = C.c_void_p(0x1234)
    assert lib.gs_import_encode_to_asset(some, C.byref(inp), 0, None, C.byref(out), None, None) == bad and not out
    assert lib.gs_import_encode_to_asset(some, C.byref(inp), 0, C.byref(fmt), None, None, None) == bad
    for k in range(6):                                            # a NULL array
        ptrs = [a.ctypes.data for a in arrs]
        ptrs[k] = None
        out = C.c_void_p(0x1234)
        assert lib.gs_import_encode_to_asset(some, C.byref(_abi.gs_import_input(16, *ptrs)), 0, C.byref(fmt), C.byref(out), None, None) == bad and not out
    refused = [(_abi.gs_import_input(0, *[a.ctypes.data for a in arrs]), 0, fmt), (inp, 2, fmt), (inp, 0, _abi.gs_import_formats(4, 2, 2, 3, 1, 1)),
               (inp, 0, _abi.gs_import_formats(2, 4, 2, 3, 1, 1)), (inp, 0, _abi.gs_import_formats(2, 2, 4, 3, 1, 1)), (inp, 0, _abi.gs_import_formats(2, 2, 2, 9, 1, 1)),
               (inp, 0, _abi.gs_import_formats(2, 2, 2, 3, 2, 1)), (inp, 0, _abi.gs_import_formats(2, 2, 2, 3, 1, 2)), (inp, 1, _abi.gs_import_formats(2, 2, 2, 8, 1, 1))]
    for i, kind, f in refused:
        out = C.c_void_p(0x1234)
        assert lib.gs_import_encode_to_asset(some, C.byref(i), kind, C.byref(f), C.byref(out), None, None) == bad and not out
    assert lib.gs_abi_version() == 9                             # an addition to ABI 9
    assert callable(creator.CreateGpuAssetFromSplats)


# ---- 2. the BC7 mode-6 block encoder --------------------------------------------------------------------------------------------------------------
def test_block_places_of_the_builders_are_the_headers(igh):
    """tests/builders.py lays the block set out with numpy restatements of gsm::BC7TexelOfLane and gsm::BC7BlockOfSplat"""
    assert [igh.igh_bc7_texel_of_lane(l) for l in range(16)] == bc7_texel_of_lane(np.arange(16)).tolist()
    at = np.concatenate([np.arange(0, 70000, 16), np.arange(440000, 446000)]).astype(np.uint32)
    assert [igh.igh_bc7_block_of_splat(int(i)) for i in at] == bc7_block_offset_of_splat(at).tolist()


def test_bc7_blocks_equal_the_importers(igh):
    texels, want = importer_blocks()
    nb = len(texels)
    assert nb >= 20000 + len(crafted_blocks())
    got, flags = np.zeros((nb, 16), np.uint8), np.zeros(nb, np.uint32)
    igh.igh_bc7_blocks(_p(texels), C.c_uint32(nb), _p(got), _p(flags))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:2]], want[bad[:2]])
    assert bytes(got[0]) == bytes([0x40] + [0] * 15)              # the all-zero block
    rnd = flags[len(crafted_blocks()):len(crafted_blocks()) + 20000]
    assert (rnd & 1).any() and not (rnd & 1).all()                # flipped and unflipped blocks
    for bit in (2, 4):
        assert (rnd & bit).any() and not (rnd & bit).all()        # both p-bit values, at either endpoint
    crafted = flags[:len(crafted_blocks())]
    assert crafted[5] & 1 and not crafted[6] & 1                  # texel 0 the brightest flips, the darkest does not


def test_bc7_sixteen_lane_formulation_gives_the_same_blocks(igh):
    texels, want = importer_blocks()
    got = np.zeros((len(texels), 16), np.uint8)
    igh.igh_bc7_blocks_lanes(_p(texels), C.c_uint32(len(texels)), _p(got))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:8])


# ---- 3. ImportLinearize / ImportRecord ---------------------------------------------------------------------------------------------------------------
def test_linearize_and_rotation_words_equal_the_importers(igh):
    n = 50000
    raw = scenes.make_splats(n, 23, 3.0)
    rng = np.random.default_rng(29)
    raw.rot[:] = rng.normal(size=(n, 4)).astype(f32)
    raw.rot[:64, 0] = raw.rot[:64, 1]                             # ties of the largest component
    edge = np.array([-1000.0, -200.0, -88.5, -88.0, -87.5, -87.0, -86.5, 86.5, 87.0, 87.5, 88.0, 88.5, 200.0, 1000.0, 0.0], f32)
    raw.scale[100:100 + len(edge), 0] = edge                      # exp_det's arguments at the clamp and beyond, in exp(scale)
    raw.opacity[200:200 + len(edge)] = edge                       # ... and in the sigmoid's exp(-opacity)
    arrs = arrays_of(raw)
    lin, word = np.zeros((n, 11), f32), np.zeros(n, np.uint32)
    igh.igh_linearize(C.byref(src_of(arrs)), C.c_uint32(n), C.c_uint32(1), _p(lin), _p(word))
    a = creator.CreateAssetFromSplatsNative(raw, "VeryHigh", linearize=True, morton=False)       # all fp32, unchunked: the linearised fields as they are
    other = a.otherData[:n * 16].view(np.uint32).reshape(n, 4)
    assert np.array_equal(word, other[:, 0])
    assert np.array_equal(lin[:, 3:6].view(np.uint32), other[:, 1:4])
    tex = a.colorData.view(f32).reshape(-1, 4)
    assert np.array_equal(np.ascontiguousarray(lin[:, [0, 1, 2, 6]]).view(np.uint32), tex[creator.SplatIndexToTextureIndex(np.arange(n))].view(np.uint32))
    assert np.isfinite(lin[:, :7]).all() and (lin[100:100 + len(edge), 3] > 0).all()
    # already linear input: the word is the importer's q(rot[k], 1023.5) | ... of the four floats as they are
    linraw = creator.LinearizeData(raw)
    arrs = arrays_of(linraw)
    igh.igh_linearize(C.byref(src_of(arrs)), C.c_uint32(n), C.c_uint32(0), _p(lin), _p(word))
    b = creator.CreateAssetFromSplatsNative(linraw, "VeryHigh", linearize=False, morton=False)
    assert np.array_equal(word, b.otherData[:n * 16].view(np.uint32).reshape(n, 4)[:, 0])
    x = np.concatenate([edge, np.linspace(-90, 90, 2001).astype(f32)])
    got = np.zeros(len(x), f32)
    igh.igh_exp(_p(x), C.c_uint32(len(x)), _p(got))
    assert np.array_equal(got.view(np.uint32), creator.ExpDet(x).astype(f32).view(np.uint32))


# ---- 4. the whole pipeline, serially ---------------------------------------------------------------------------------------------------------------------
def host_import(igh, raw, formats, linearize, morton=True) -> A.GaussianSplatAsset:
    n = len(raw)
    arrs = arrays_of(raw)
    src = src_of(arrs)
    fp, fs, fc, fsh = formats
    fmt = _abi.gs_import_formats(int(fp), int(fs), int(fc), int(fsh), int(linearize), int(morton))
    sizes = (C.c_uint64 * 5)()
    _lib.check(_lib.lib().gs_import_blob_sizes(n, C.byref(fmt), sizes), "gs_import_blob_sizes")
    blobs = [np.zeros(int(sz), np.uint8) if sz else None for sz in sizes]
    ptrs = (C.c_void_p * 5)(*[b.ctypes.data if b is not None else None for b in blobs])
    means, index, k = None, None, A.GetSHCount(SF(fsh), n) if fsh > SF.Norm6 else 0
    if k:
        rows = np.zeros((n, 45), f32)
        igh.igh_sh_rows(C.byref(src), C.c_uint32(n), C.c_uint32(int(linearize)), C.c_uint32(int(morton)), _p(rows))
        means, index = creator.ClusterSHsNative(rows, k)
    bounds = np.zeros(6, f32)
    four = np.array([int(fp), int(fs), int(fc), int(fsh)], np.uint32)
    igh.igh_import(C.byref(src), C.c_uint32(n), _p(four), C.c_uint32(int(linearize)), C.c_uint32(int(morton)), _p(means), C.c_uint32(k), _p(index), ptrs,
                   C.c_uint64(int(sizes[2])), _p(bounds))
    return A.GaussianSplatAsset(splatCount=n, posFormat=VF(fp), scaleFormat=VF(fs), shFormat=SF(fsh), colorFormat=CF(fc), posData=blobs[0], otherData=blobs[1],
                                colorData=blobs[2], shData=blobs[3], chunkData=blobs[4], boundsMin=tuple(bounds[:3]), boundsMax=tuple(bounds[3:]))


def want_of(raw, formats, linearize, morton=True) -> A.GaussianSplatAsset:
    fp, fs, fc, fsh = formats
    return creator.CreateAssetFromSplatsNative(raw, formatPos=fp, formatScale=fs, formatColor=fc, formatSH=fsh, linearize=linearize, morton=morton)


def input_of(n, linearize):
    raw = scenes.make_splats(n, 300 + n, 3.0)
    raw = raw if linearize else creator.LinearizeData(raw)
    BM.assert_no_negative_zero(creator.LinearizeData(raw) if linearize else raw)
    return raw


UNCLUSTERED = [creator.QUALITY[q] for q in ("VeryHigh", "High", "Medium")] + [BC7_TARGET, (VF.Norm6, VF.Float32, CF.BC7, SF.Float16)]


@pytest.mark.parametrize("linearize", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 700])
def test_serial_pipeline_equals_the_importer(igh, n, linearize):
    raw = input_of(n, linearize)
    for formats in UNCLUSTERED:
        BM.assert_same_asset(host_import(igh, raw, formats, linearize), want_of(raw, formats, linearize), (n, formats, linearize))
    BM.assert_same_asset(host_import(igh, raw, BC7_TARGET, linearize, morton=False), want_of(raw, BC7_TARGET, linearize, morton=False), (n, "no morton"))


@pytest.mark.parametrize("linearize", [True, False])
@pytest.mark.parametrize("quality", ["VeryLow", "CLUSTER4K"])
def test_serial_pipeline_equals_the_importer_clustered(igh, quality, linearize):
    """the Cluster* presets need more splats than table entries: 4,500 to Cluster4k -- VeryLow as it is, and Low's formats with a Cluster4k table"""
    raw = input_of(4500, linearize)
    formats = creator.QUALITY["VeryLow"] if quality == "VeryLow" else creator.QUALITY["Low"][:3] + (SF.Cluster4k,)
    BM.assert_same_asset(host_import(igh, raw, formats, linearize), want_of(raw, formats, linearize), (quality, linearize))


# the adversarial walk: the yardstick's side of tests/test_gpu_import_edges.py, held without a GPU
@pytest.mark.parametrize("seed", EDGE_SEEDS)
def test_serial_pipeline_equals_the_importer_on_adversarial_input(igh, seed):
    raw = edge_case(seed)
    for linearize in (True, False):
        src = raw if linearize else linear_input(raw)
        assert_import_premises(src, linearize)
        for morton in (True, False):
            for formats in EDGE_FORMATS:
                BM.assert_same_asset(host_import(igh, src, formats, linearize, morton), want_of(src, formats, linearize, morton), (seed, formats, linearize, morton))


def test_adversarial_inputs_hold_what_they_are_there_for():
    raws = [edge_case(seed) for seed in EDGE_SEEDS]
    rot, opacity, scale, sh = (np.concatenate([np.asarray(getattr(r, name)).reshape(len(r), -1) for r in raws]) for name in ("rot", "opacity", "scale", "sh"))
    assert (rot == 0).all(axis=1).any()                            # the zero quaternion: normalize() divides by 0
    low = opacity[opacity <= -88]
    lin = creator.Sigmoid(low)
    tiny = np.finfo(f32).tiny
    assert len(low) and ((lin > 0) & (lin < tiny)).any()            # 1 / (1 + exp(88)): the sigmoid's division lands in the denormals
    assert (scale < -87).any() and (scale > 88).any()              # both sides of exp's clamp
    assert ((sh != 0) & (np.abs(sh) < tiny)).any()                 # an SH denormal
    assert len({len(r) for r in raws}) >= 4                        # several of the sizes around the chunk boundaries


def test_bc7_tiles_past_the_last_chunk_hold_the_zero_block(igh):
    raw = input_of(257, True)
    a = host_import(igh, raw, BC7_TARGET, True)
    blocks = a.colorData.reshape(-1, 16)
    assert len(blocks) == 2048 * 16 // 16 and (blocks[:, 0] & 0x7f == 0x40).all()
    assert (blocks == np.array([0x40] + [0] * 15, np.uint8)).all(axis=1).sum() >= (128 - 2) * 16


# ---- 5. the harness as a stand-alone program under the host sanitizers -------------------------------------------------------------------------------------
def test_stand_alone_harness_runs_clean_under_the_host_sanitizers(tmp_path):
    out = run_under_sanitizers(tmp_path, "import_gpu_host_harness.cpp", "IMPORT_GPU_HARNESS_MAIN")
    assert out.returncode == 0 and "import gpu harness ok" in out.stdout, (out.stdout, out.stderr[-2000:])
