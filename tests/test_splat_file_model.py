"""The file sources of the GPU import on the CPU box: the host build of their arithmetic (tests/splat_file_host_harness.cpp over
csrc/gs_device_math.h: gsm::PlyRowRecord over a PLY's vertex rows as they lie in the file, gsm::SpzRecord over an SPZ's gunzipped stream) against the
arrays of the built library's readers (gs_ply_open / gs_spz_open) pushed through gsm::ImportRecord -- the records the array import encodes -- bit for
bit; and the harness as a stand-alone program under the host sanitizers."""
import ctypes as C
import gzip

import numpy as np
import pytest

import file_cases as FC
from harness import build_harness, run_under_sanitizers
from unitygaussiansplatting_amd import creator, scenes

f32 = np.float32


class ImportSrc(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("pos", "dc0", "sh", "opacity", "scale", "rot")]


@pytest.fixture(scope="module")
def sfh(tmp_path_factory):
    lib = C.CDLL(build_harness(tmp_path_factory.mktemp("sfh"), "splat_file_host_harness.cpp"))
    lib.sfh_record_bytes.restype = lib.sfh_ply_records.restype = C.c_uint32
    assert lib.sfh_record_bytes() == 56 * 4                       # pos 3, rot word, scale 3, colour 4, sh 45
    return lib


def import_records(sfh, raw, linearize) -> np.ndarray:
    """the records gsm::ImportRecord makes of the reader's six arrays: [n, 56] words"""
    n = len(raw)
    arrs = [np.ascontiguousarray(a, f32) for a in (raw.pos, raw.dc0, np.asarray(raw.sh).reshape(n, 45), raw.opacity, raw.scale, raw.rot)]
    src = ImportSrc(*[a.ctypes.data for a in arrs])
    out = np.zeros((n, 56), np.uint32)
    sfh.sfh_import_records(C.byref(src), n, int(linearize), out.ctypes.data_as(C.c_void_p))
    return out


def ply_records(sfh, rows, offsets, path):
    """path 2: the loads gsm::PlyRowLayout chooses for the layout; 1: the table's dword loads at most; 0: byte loads.  Returns the records, the
    positions and the layout's flags (aligned | inria << 1)"""
    n, stride = rows.shape
    rows = rows.copy()                                             # (a view into the file's bytes starts wherever the header ends)
    assert rows.ctypes.data % 4 == 0
    out, pos = np.zeros((n, 56), np.uint32), np.zeros((n, 3), f32)
    flags = sfh.sfh_ply_records(rows.ctypes.data_as(C.c_void_p), stride, (C.c_int32 * 62)(*offsets), path, n, out.ctypes.data_as(C.c_void_p),
                                pos.ctypes.data_as(C.c_void_p))
    return out, pos, flags


def spz_records(sfh, stream: bytes, n, sh_level, fract_bits):
    buf = np.frombuffer(stream, np.uint8).copy()
    out, pos = np.zeros((n, 56), np.uint32), np.zeros((n, 3), f32)
    sfh.sfh_spz_records(buf.ctypes.data_as(C.c_void_p), n, FC.SH_COEFFS[sh_level], fract_bits, out.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p))
    return out, pos


def assert_same_records(got, pos, want, what):
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, bad[:8], np.flatnonzero(got[bad[0]] != want[bad[0]]))
    assert np.array_equal(pos.view(np.uint32), want[:, :3]), what


# ---- PLY rows ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FC.LAYOUTS)
def test_ply_rows_give_the_records_of_the_readers_arrays(sfh, tmp_path, kind):
    raw = scenes.make_splats(700, 1100, 3.0)
    path = str(tmp_path / f"{kind}.ply")
    FC.write_ply(path, raw, kind=kind)
    _, _, info = FC.open_result(path)
    offsets = list(info.offsets)
    want = import_records(sfh, creator.ReadPLYNative(path), True)
    rows = FC.ply_rows(path, info.splat_count, info.stride)
    for path in (0, 1, 2):                                         # byte loads read any layout; dword loads the aligned ones; merged loads the INRIA one
        got, pos, flags = ply_records(sfh, rows, offsets, path)
        assert flags == {"uchar": 0, "inria": 3, "crlf": 3}.get(kind, 1), (kind, flags)
        assert (flags & 1) == FC.rows_aligned(info.stride, offsets)
        assert_same_records(got, pos, want, (kind, path))
    if kind in ("no_rest", "rest9"):
        sh = want[:, 11:].view(f32).reshape(-1, 15, 3)
        assert not sh[:, 9 if kind == "rest9" else 0:, 0].any() and (kind == "no_rest" or sh[:, :9, 0].any())      # f_rest_0..8: red, coefficients 0..8


def test_ply_rows_at_an_odd_address(sfh, tmp_path):
    """the rows of the stride-249 file start one byte into a buffer: every field of every row straddles dwords somewhere"""
    raw = scenes.make_splats(257, 1101, 3.0)
    path = str(tmp_path / "odd.ply")
    FC.write_ply(path, raw, kind="uchar")
    _, _, info = FC.open_result(path)
    want = import_records(sfh, creator.ReadPLYNative(path), True)
    rows = FC.ply_rows(path, info.splat_count, info.stride)
    buf = np.zeros(rows.size + 1, np.uint8)
    buf[1:] = rows.reshape(-1)
    out, pos = np.zeros((257, 56), np.uint32), np.zeros((257, 3), f32)
    assert sfh.sfh_ply_records(C.c_void_p(buf.ctypes.data + 1), 249, (C.c_int32 * 62)(*info.offsets), 2, 257, out.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p)) == 0
    assert_same_records(out, pos, want, "odd address")


# ---- SPZ columns --------------------------------------------------------------------------------------------------------------------------------------
def spz_case(sfh, tmp_path, stream, n, sh_level, fract_bits, what):
    path = str(tmp_path / "case.spz")
    FC.write_stream(path, stream)
    raw = creator.ReadSPZNative(path)
    assert len(raw) == n
    got, pos = spz_records(sfh, gzip.decompress(open(path, "rb").read()), n, sh_level, fract_bits)
    assert_same_records(got, pos, import_records(sfh, raw, False), what)
    return raw


@pytest.mark.parametrize("fract_bits", [0, 12, 24])
def test_spz_every_byte_of_scale_colour_alpha_and_sh(sfh, tmp_path, fract_bits):
    """1,024 points: each of the alpha, colour and scale columns runs through all 256 bytes four times, the level-3 SH column through all of them many
    times; the positions start with 0, 1, 0x7fffff, 0x800000, 0xffffff on every axis, the rotations with the four corner cases, then seeded samples"""
    n = 1024
    stream = FC.crafted_spz_stream(n, 3, fract_bits, seed=5 + fract_bits)
    cols = np.frombuffer(stream, np.uint8)
    for first, width in ((16 + n * 9, 1), (16 + n * 10, 3), (16 + n * 13, 3)):
        col = cols[first:first + n * width].reshape(n, width)
        for c in range(width):
            assert len(np.unique(col[:, c])) == 256
    assert len(np.unique(cols[16 + n * 19:])) == 256
    raw = spz_case(sfh, tmp_path, stream, n, 3, fract_bits, fract_bits)
    scale = f32(1.0) / f32(1 << fract_bits)
    assert raw.pos[0, 0] == 0 and raw.pos[1, 0] == scale and raw.pos[2, 0] == f32(0x7fffff) * scale and raw.pos[3, 0] == f32(-0x800000) * scale and raw.pos[4, 0] == -scale


def test_spz_rotations(sfh, tmp_path):
    """every rotation whose bytes are 0, 127, 128 or 255 on each axis, and a seeded 4,000"""
    rng = np.random.default_rng(99)
    corners = np.array([(a, b, c) for a in (0, 127, 128, 255) for b in (0, 127, 128, 255) for c in (0, 127, 128, 255)])
    assert all(r in corners.tolist() for r in map(list, FC.ROTATIONS))
    rot = np.concatenate([corners, rng.integers(0, 256, (4000, 3))])
    n = len(rot)
    stream = FC.spz_stream(n, 0, 12, rng.integers(0, 1 << 24, (n, 3)), rng.integers(0, 256, n), rng.integers(0, 256, (n, 3)), rng.integers(0, 256, (n, 3)), rot, [])
    spz_case(sfh, tmp_path, stream, n, 0, 12, "rotations")


@pytest.mark.parametrize("n", [1, 2, 5, 300])
@pytest.mark.parametrize("sh_level", [0, 1, 2, 3])
def test_spz_sh_levels_and_the_run_on_read(sfh, tmp_path, sh_level, n):
    """fifteen coefficients are read from i * 3 * shCoeffs whatever the level: below level 3 a splat reads on into its successors' bytes, and the
    last ones leave the array, where a byte reads as 128"""
    rng = np.random.default_rng(300 + sh_level)
    k = FC.SH_COEFFS[sh_level]
    sh = rng.integers(0, 256, n * 3 * k)
    sh[sh == 128] = 129                                            # so that a zero among the SH can only come from past the array
    stream = FC.spz_stream(n, sh_level, 12, rng.integers(0, 1 << 24, (n, 3)), rng.integers(0, 256, n), rng.integers(0, 256, (n, 3)), rng.integers(0, 256, (n, 3)),
                           rng.integers(0, 256, (n, 3)), sh)
    raw = spz_case(sfh, tmp_path, stream, n, sh_level, 12, (sh_level, n))
    last = np.asarray(raw.sh).reshape(n, 45)[-1]
    assert (last[:3 * k] != 0).all() and not last[3 * k:].any()
    if n > 1 and 0 < sh_level < 3:
        first = np.asarray(raw.sh).reshape(n, 45)[0]
        assert np.array_equal(first[3 * k:min(45, 6 * k)], np.asarray(raw.sh).reshape(n, 45)[1][:min(45, 6 * k) - 3 * k])


def test_written_spz_files(sfh, tmp_path):
    raw = scenes.make_splats(1000, 41, 2.0)
    for sh_level, fract_bits in ((3, 12), (1, 0), (2, 24)):
        path = str(tmp_path / f"w{sh_level}.spz")
        creator.WriteSPZ(path, raw, fract_bits=fract_bits, sh_level=sh_level)
        got, pos = spz_records(sfh, gzip.decompress(open(path, "rb").read()), 1000, sh_level, fract_bits)
        assert_same_records(got, pos, import_records(sfh, creator.ReadSPZNative(path), False), (sh_level, fract_bits))


# ---- the harness under the host sanitizers ----------------------------------------------------------------------------------------------------------
def test_harness_runs_clean_under_the_host_sanitizers(tmp_path):
    r = run_under_sanitizers(tmp_path, "splat_file_host_harness.cpp", "SPLAT_FILE_HARNESS_MAIN")
    assert r.returncode == 0 and "splat file harness ok" in r.stdout, (r.stdout, r.stderr[-2000:])
