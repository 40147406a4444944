"""gs_splat_file_open (csrc/gs_import.cpp) against the readers it shares its checks with, gs_ply_open and gs_spz_open: for every file either of them
refuses the same return code and the same gs_last_error_string text; for every file they read the same count, and a stride and a table of offsets
that give the reader's six arrays when applied in numpy to the file's own bytes.  Host code only: no GPU."""
import ctypes as C
import gzip

import numpy as np
import pytest

import file_cases as FC
from unitygaussiansplatting_amd import _abi, _lib, creator, scenes

RAW = scenes.make_splats(300, 17, 2.0)


def test_refused_ply_files_give_the_readers_error(tmp_path):
    cases = FC.refused_ply_files(tmp_path, RAW)
    assert len(cases) >= 10
    for what, path in cases:
        rc, text, _ = FC.reader_result(path)
        got_rc, got_text, _ = FC.open_result(path)
        assert rc != 0 and text, what
        assert (got_rc, got_text) == (rc, text), (what, got_rc, got_text, rc, text)


def test_refused_spz_files_give_the_readers_error(tmp_path):
    cases = FC.refused_spz_files(tmp_path, RAW)
    assert len(cases) >= 10
    for what, path in cases:
        rc, text, _ = FC.reader_result(path)
        got_rc, got_text, _ = FC.open_result(path)
        assert rc != 0 and text, what
        assert (got_rc, got_text) == (rc, text), (what, got_rc, got_text, rc, text)


def test_the_refusals_cover_every_message_of_the_readers(tmp_path):
    texts = {FC.reader_result(p)[1] for _, p in FC.refused_ply_files(tmp_path, RAW) + FC.refused_spz_files(tmp_path, RAW)}
    for part in (b"cannot be opened", b"binary, little endian", b"no vertices", b"required float property", b"fewer data bytes", b"not a gzip stream",
                 b"failed to read header", b"magic", b"version", b"splat count", b"SH level", b"fractional bits", b"smaller than it should be"):
        assert any(part in t for t in texts), part


@pytest.mark.parametrize("kind", FC.LAYOUTS)
def test_ply_offsets_reproduce_the_readers_arrays(tmp_path, kind):
    path = str(tmp_path / f"{kind}.ply")
    FC.write_ply(path, RAW, kind=kind)
    rc, _, count = FC.reader_result(path)
    got_rc, _, info = FC.open_result(path)
    assert rc == 0 and got_rc == 0
    props = FC.ply_layout(kind)
    assert info.kind == _abi.GS_SPLAT_FILE_PLY and info.splat_count == count == len(RAW)
    assert info.stride == FC.stride_of(props) and info.body_bytes == count * info.stride and info.sh_level == 0 and info.fract_bits == 0
    offsets = list(info.offsets)
    names = [nm for nm, t in props if t == "float"]
    for k, nm in enumerate(_abi.PLY_OFFSET_NAMES):
        assert (offsets[k] >= 0) == (nm in names), (kind, nm)
        assert offsets[k] < 0 or (offsets[k] + 4 <= info.stride), (kind, nm)
    assert FC.rows_aligned(info.stride, offsets) == (kind != "uchar")
    want = creator.ReadPLYNative(path)
    got = FC.arrays_from_rows(FC.ply_rows(path, count, info.stride), offsets)
    for nm in ("pos", "dc0", "sh", "opacity", "scale", "rot"):
        assert FC.same_bits(getattr(got, nm), getattr(want, nm)), (kind, nm)
    assert FC.same_bits(want.pos, RAW.pos) and FC.same_bits(want.rot, RAW.rot)


def test_the_first_float_property_of_a_name_wins_and_other_types_do_not_count(tmp_path):
    """two float `opacity` properties: the first is read; a uchar `x` before the float one is not x"""
    props = [("x", "uchar")] + FC.INRIA + [("opacity", "float")]
    path = str(tmp_path / "twice.ply")
    FC.write_ply(path, RAW, props)
    _, _, info = FC.open_result(path)
    offsets = list(info.offsets)
    assert offsets[0] == 1 and offsets[6] == 1 + 54 * 4 and info.stride == 1 + 63 * 4
    want = creator.ReadPLYNative(path)
    got = FC.arrays_from_rows(FC.ply_rows(path, len(RAW), info.stride), offsets)
    assert FC.same_bits(got.opacity, want.opacity) and FC.same_bits(got.pos, want.pos) and FC.same_bits(want.opacity, RAW.opacity)


def test_bytes_behind_the_rows_are_ignored(tmp_path):
    path = str(tmp_path / "tail.ply")
    FC.write_ply(path, RAW)
    open(path, "ab").write(b"trailing bytes")
    assert FC.reader_result(path)[0] == 0
    rc, _, info = FC.open_result(path)
    assert rc == 0 and info.body_bytes == len(RAW) * 248


@pytest.mark.parametrize("sh_level,fract_bits", [(0, 0), (1, 12), (2, 24), (3, 12)])
def test_spz_info(tmp_path, sh_level, fract_bits):
    path = str(tmp_path / "scene.spz")
    creator.WriteSPZ(path, RAW, fract_bits=fract_bits, sh_level=sh_level)
    rc, _, count = FC.reader_result(path)
    got_rc, _, info = FC.open_result(path)
    assert rc == 0 and got_rc == 0
    n = len(RAW)
    assert info.kind == _abi.GS_SPLAT_FILE_SPZ and info.splat_count == count == n and info.stride == 0
    assert (info.sh_level, info.fract_bits) == (sh_level, fract_bits)
    assert info.body_bytes == len(gzip.decompress(open(path, "rb").read())) == 16 + n * (9 + 1 + 3 + 3 + 3 + 3 * FC.SH_COEFFS[sh_level])
    assert all(o == -1 for o in info.offsets)


def test_the_kind_follows_the_extension(tmp_path):
    lib = _lib.lib()
    ply, spz = str(tmp_path / "A.PLY"), str(tmp_path / "b.SpZ")
    FC.write_ply(ply, RAW)
    creator.WriteSPZ(spz, RAW)
    assert FC.open_result(ply)[2].kind == _abi.GS_SPLAT_FILE_PLY and FC.open_result(spz)[2].kind == _abi.GS_SPLAT_FILE_SPZ
    other = str(tmp_path / "scene.txt")
    open(other, "wb").write(open(ply, "rb").read())
    rc, text, _ = FC.open_result(other)
    assert rc == _abi.GS_ERR_INVALID_ASSET and b"not a supported format" in text
    renamed = str(tmp_path / "really_a_ply.spz")                    # the extension decides, as in GaussianFileReader.ReadFile
    open(renamed, "wb").write(open(ply, "rb").read())
    assert FC.open_result(renamed)[:2] == FC.reader_result(renamed)[:2] and b"gzip" in FC.open_result(renamed)[1]
    out = C.c_void_p(0x1234)
    assert lib.gs_splat_file_open(None, C.byref(out), None) == _abi.GS_ERR_INVALID_ARGUMENT
    assert lib.gs_splat_file_open(ply.encode(), None, None) == _abi.GS_ERR_INVALID_ARGUMENT


def test_handles_close_once(tmp_path):
    lib = _lib.lib()
    path = str(tmp_path / "scene.ply")
    FC.write_ply(path, RAW)
    a, b = C.c_void_p(), C.c_void_p()
    assert lib.gs_splat_file_open(path.encode(), C.byref(a), None) == 0 and lib.gs_splat_file_open(path.encode(), C.byref(b), None) == 0
    assert a.value != b.value
    assert lib.gs_splat_file_close(a) == 0
    assert lib.gs_splat_file_close(a) == _abi.GS_ERR_INVALID_ARGUMENT and b"not an open" in lib.gs_last_error_string()
    assert lib.gs_splat_file_close(b) == 0 and lib.gs_splat_file_close(None) == 0
    # without a device: every refusal of the import comes before the context is touched
    fmt = _abi.gs_import_formats(2, 2, 2, 3, 1, 1)
    some = C.create_string_buffer(64)
    out = C.c_void_p(0x1234)
    assert lib.gs_import_file_to_asset(some, a, C.byref(fmt), 0, C.byref(out), None, None) == _abi.GS_ERR_INVALID_ARGUMENT and not out
    out = C.c_void_p(0x1234)
    assert lib.gs_import_file_to_asset(some, None, C.byref(fmt), 0, C.byref(out), None, None) == _abi.GS_ERR_INVALID_ARGUMENT and not out
    assert lib.gs_abi_version() == 9 and callable(creator.CreateGpuAssetFromFile)
