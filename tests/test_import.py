"""The native importer (gs_import_encode, csrc/gs_import.cpp) against the numpy importer (creator.py): the five blobs and
the bounds must be identical byte for byte, for every quality preset / format it supports, with and without LinearizeData and
the Morton reorder, for splat counts that do and do not fill the last chunk / texture tile.  No GPU needed (host code)."""
import ctypes as C

import numpy as np
import pytest

from builders import _same
from unitygaussiansplatting_amd import _lib, creator, scenes
from unitygaussiansplatting_amd import asset as A
from unitygaussiansplatting_amd._abi import gs_import_formats

@pytest.mark.parametrize("quality", ["Medium", "High", "VeryHigh"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 30_011])
def test_native_importer_matches_numpy_presets(quality, n):
    raw = scenes.make_splats(n, 100 + n, 3.0)
    _same(creator.CreateAssetFromSplats(raw, quality), creator.CreateAssetFromSplatsNative(raw, quality))


@pytest.mark.parametrize("fmt", [
    dict(formatPos=A.VectorFormat.Norm16, formatScale=A.VectorFormat.Norm6, formatSH=A.SHFormat.Float16, formatColor=A.ColorFormat.Float16x4),
    dict(formatPos=A.VectorFormat.Norm6, formatScale=A.VectorFormat.Float32, formatSH=A.SHFormat.Norm11, formatColor=A.ColorFormat.Float32x4),
    dict(formatPos=A.VectorFormat.Float32, formatScale=A.VectorFormat.Norm16, formatSH=A.SHFormat.Float32, formatColor=A.ColorFormat.Norm8x4),
    dict(formatPos=A.VectorFormat.Norm11, formatScale=A.VectorFormat.Norm11, formatSH=A.SHFormat.Norm6, formatColor=A.ColorFormat.Float16x4)])
@pytest.mark.parametrize("morton,linearize", [(True, True), (False, True), (True, False)])
def test_native_importer_matches_numpy_formats(fmt, morton, linearize):
    raw = scenes.make_splats(5_003, 9, 2.0)
    if not linearize:
        raw = creator.LinearizeData(raw)
    _same(creator.CreateAssetFromSplats(raw, "Medium", morton=morton, linearize=linearize, **fmt),
          creator.CreateAssetFromSplatsNative(raw, "Medium", morton=morton, linearize=linearize, **fmt))


def test_deterministic_exp_is_accurate_and_extreme_inputs_agree():
    x = np.concatenate([np.linspace(-30, 30, 200_001), [-87.0, -86.9, 88.0, 87.9, 0.0, -0.0, 1e-8, -1e-8]]).astype(np.float32)
    got = creator.ExpDet(x).astype(np.float64)
    want = np.exp(x.astype(np.float64))
    assert (np.abs(got - want) / want).max() < 2.0 ** -21
    # degenerate inputs: identical positions (empty bounds), zero quaternion component ties, huge / tiny scales and logits
    raw = scenes.make_splats(700, 3, 1.0)
    raw.pos[:300] = raw.pos[0]
    raw.rot[:50] = np.array([0.5, 0.5, 0.5, 0.5], np.float32)
    raw.scale[50:100] = np.float32(-20.0); raw.scale[100:150] = np.float32(3.0)
    raw.opacity[150:200] = np.float32(40.0); raw.opacity[200:250] = np.float32(-40.0)
    raw.sh[250:300] = np.float32(0.25)
    _same(creator.CreateAssetFromSplats(raw, "Medium"), creator.CreateAssetFromSplatsNative(raw, "Medium"))


def test_native_importer_argument_validation():
    lib = _lib.lib()
    sizes = (C.c_uint64 * 5)()
    ok = gs_import_formats(2, 2, 2, 3, 1, 1)
    assert lib.gs_import_blob_sizes(1000, C.byref(ok), sizes) == 0
    assert list(sizes) == [4000, 8000, 2048 * 16 * 4, 32000, 4 * 64]
    assert lib.gs_import_blob_sizes(0, C.byref(ok), sizes) == -1
    assert lib.gs_import_blob_sizes(1000, C.byref(gs_import_formats(2, 2, 3, 3, 1, 1)), sizes) == 0        # BC7: 1 byte per texel
    assert list(sizes)[2] == 2048 * 16
    assert lib.gs_import_blob_sizes(1000, C.byref(gs_import_formats(2, 2, 2, 8, 1, 1)), sizes) == -1       # Cluster4k needs > 4096 splats
    assert lib.gs_import_blob_sizes(5000, C.byref(gs_import_formats(2, 3, 2, 8, 1, 1)), sizes) == 0
    assert list(sizes)[1] == 5000 * 8 and list(sizes)[3] == 4096 * 96                                      # rot + Norm6 scale + u16 index; fp16 table
    assert lib.gs_import_blob_sizes(1000, C.byref(gs_import_formats(9, 2, 2, 3, 1, 1)), sizes) == -1
    assert lib.gs_import_encode(None, C.byref(ok), (C.c_void_p * 5)(), sizes, None, None) == -1
    with pytest.raises(_lib.GsError):
        creator.CreateAssetFromSplatsNative(scenes.make_splats(5000, 3, 2.0), "Low")          # Cluster16k with 5000 splats


@pytest.mark.parametrize("quality,n", [("VeryLow", 4_500), ("VeryLow", 9_001), ("Low", 17_000)])
def test_native_importer_matches_numpy_clustered_and_bc7(quality, n):
    """The VeryLow (BC7 colour + Cluster4k SH + Norm6 scale) and Low (Cluster16k) presets: SH palette, u16 indices and mode-6
    BC7 blocks byte for byte equal in the two importers (deterministic k-means, fp32 block encoder restated op for op)."""
    raw = scenes.make_splats(n, 200 + n, 3.0)
    a, b = creator.CreateAssetFromSplats(raw, quality), creator.CreateAssetFromSplatsNative(raw, quality)
    _same(a, b)
    k = A.GetSHCount(a.shFormat, n)
    assert len(a.shData) == k * 96 and len(np.unique(np.frombuffer(a.otherData[:n * 8], "<u2").reshape(n, 4)[:, 3])) > k // 8


def test_native_ply_reader_matches_numpy(tmp_path):
    raw = scenes.make_splats(3_001, 21, 2.0)
    path = str(tmp_path / "scene.ply")
    creator.WritePLY(path, raw)
    a, b = creator.ReadPLY(path), creator.ReadPLYNative(path)
    for nm in ("pos", "dc0", "sh", "opacity", "scale", "rot"):
        assert np.array_equal(getattr(a, nm), getattr(b, nm)), nm
    assert np.array_equal(b.pos, raw.pos) and np.array_equal(b.sh, raw.sh)
    # PLY in -> asset out, natively end to end, equals the numpy path
    _same(creator.CreateAssetFromSplats(a, "Medium"), creator.CreateAssetFromSplatsNative(b, "Medium"))
    # header rules of PLYFileReader.cs: ascii / big-endian files are refused, a missing required property too
    txt = open(path, "rb").read()
    bad = str(tmp_path / "ascii.ply")
    open(bad, "wb").write(txt.replace(b"binary_little_endian", b"ascii"))
    with pytest.raises(_lib.GsError):
        creator.ReadPLYNative(bad)
    bad2 = str(tmp_path / "noopacity.ply")
    open(bad2, "wb").write(txt.replace(b"property float opacity", b"property float opacitx"))
    with pytest.raises(_lib.GsError):
        creator.ReadPLYNative(bad2)
    with pytest.raises(_lib.GsError):
        creator.ReadPLYNative(str(tmp_path / "missing.ply"))
    # a file without f_rest_* properties: SH = 0 (GaussianFileReader.cs: absent attributes stay default)
    hdr, body = txt.split(b"end_header\n", 1)
    lines = [l for l in hdr.split(b"\n") if l and not l.startswith(b"property float f_rest_")]
    arr = np.frombuffer(body, "<f4").reshape(-1, 62)
    keep = [i for i, nm in enumerate(creator.PLY_ATTRS) if not nm.startswith("f_rest_")]
    slim = str(tmp_path / "slim.ply")
    open(slim, "wb").write(b"\n".join(lines) + b"\nend_header\n" + np.ascontiguousarray(arr[:, keep]).tobytes())
    c, d = creator.ReadPLY(slim), creator.ReadPLYNative(slim)
    assert np.array_equal(c.sh, d.sh) and not d.sh.any() and np.array_equal(c.rot, d.rot) and np.array_equal(d.pos, raw.pos)


@pytest.mark.parametrize("sh_level,fract_bits", [(3, 12), (2, 10), (1, 16), (0, 8)])
def test_spz_reader_native_matches_numpy_and_the_format(tmp_path, sh_level, fract_bits):
    """SPZFileReader.cs: the native reader (gs_spz_open) == the numpy restatement bit for bit; both recover what WriteSPZ
    quantised (positions to 2^-fract_bits, log-scales to 1/16, opacities and colours to a byte); the unpacked splats are
    already linear, so they encode with linearize = 0 -- natively and in numpy to the same bytes."""
    raw = scenes.make_splats(2_345, 31, 2.0)
    path = str(tmp_path / "scene.spz")
    creator.WriteSPZ(path, raw, fract_bits=fract_bits, sh_level=sh_level)
    a, b = creator.ReadSPZ(path), creator.ReadSPZNative(path)
    for nm in ("pos", "dc0", "sh", "opacity", "scale", "rot"):
        assert np.array_equal(getattr(a, nm), getattr(b, nm)), nm
    lin = creator.LinearizeData(raw)
    assert np.abs(a.pos - raw.pos).max() <= 0.5 / (1 << fract_bits) + 1e-6
    assert np.abs(np.log(a.scale) - np.clip(raw.scale, -10.0, 5.9)).max() <= 0.5 / 16 + 1e-4
    assert np.abs(a.opacity - lin.opacity).max() <= 0.5 / 255 + 1e-6
    assert np.abs(a.dc0 - np.clip(lin.dc0, 0.5 - 0.5 / 0.15 * 0.2820948, 0.5 + 0.5 / 0.15 * 0.2820948)).max() <= 0.0075
    k = {0: 0, 1: 3, 2: 8, 3: 15}[sh_level]
    if sh_level == 3:
        assert np.abs(a.sh - np.clip(raw.sh, -1.0, 127.0 / 128.0)).max() <= 0.5 / 128 + 1e-6
    else:
        assert k == 0 or np.abs(a.sh[:, :k] - raw.sh[:, :k]).max() <= 0.5 / 128 + 1e-6      # (the reference reads on into its neighbours' bytes beyond k)
    # rotation: the packed smallest-three decodes to the file's quaternion within a byte step
    _same(creator.CreateAssetFromSplats(a, "Medium", linearize=False), creator.CreateAssetFromSplatsNative(b, "Medium", linearize=False))
    assert creator.CreateAsset(path, "Medium").splatCount == len(raw)
    # header rules (:37-47, :72-77)
    import gzip, struct
    body = gzip.decompress(open(path, "rb").read())
    for bad_hdr in (struct.pack("<IIII", 0x12345678, 2, 10, 3), struct.pack("<IIII", creator.SPZ_MAGIC, 3, 10, 3),
                    struct.pack("<IIII", creator.SPZ_MAGIC, 2, 0, 3), struct.pack("<IIII", creator.SPZ_MAGIC, 2, 10, 4),
                    struct.pack("<IIII", creator.SPZ_MAGIC, 2, len(raw) + 1, sh_level | (fract_bits << 8))):
        bad = str(tmp_path / "bad.spz")
        open(bad, "wb").write(gzip.compress(bad_hdr + body[16:]))
        with pytest.raises(IOError):
            creator.ReadSPZ(bad)
        with pytest.raises(_lib.GsError):
            creator.ReadSPZNative(bad)
    notgz = str(tmp_path / "notgz.spz")
    open(notgz, "wb").write(body)
    with pytest.raises(IOError):
        creator.ReadSPZ(notgz)
    with pytest.raises(_lib.GsError):
        creator.ReadSPZNative(notgz)
