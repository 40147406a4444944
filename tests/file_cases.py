"""What the file-import suites share (helper, not a test): PLY files in the layouts a reader may meet, SPZ files made column by column, the files
both readers refuse, and the yardstick -- the host route over the same file: creator.CreateAssetFromSplatsNative(ReadPLYNative | ReadSPZNative,
linearize = PLY).  Everything is written where the caller says (pytest's tmp_path); nothing here needs a GPU."""
import ctypes as C
import gzip
import struct

import numpy as np

import bake_model as BM
from common import same_bits
from unitygaussiansplatting_amd import _abi, _lib, creator

f32 = np.float32
NP_OF = {"float": "<f4", "double": "<f8", "uchar": "u1"}          # the types the readers size; any other adds no bytes
REQUIRED = _abi.PLY_OFFSET_NAMES[:14]
INRIA = [(nm, "float") for nm in creator.PLY_ATTRS]


# ---- PLY ----------------------------------------------------------------------------------------------------------------------------------------
def ply_layout(kind: str):
    """the properties of a vertex row, in file order, as (name, type)"""
    if kind in ("inria", "crlf"):
        return list(INRIA)
    if kind == "shuffled":
        order = np.random.default_rng(6262).permutation(62)
        return [INRIA[i] for i in order]
    if kind == "no_rest":
        return [p for p in INRIA if not p[0].startswith("f_rest_")]
    if kind == "rest9":
        return [p for p in INRIA if not p[0].startswith("f_rest_") or int(p[0][7:]) < 9]
    if kind == "uchar":                                            # stride 249: every row but each fourth starts off a dword
        return INRIA[:9] + [("red", "uchar")] + INRIA[9:]
    if kind == "double_int":                                       # a double moves what follows by 8; the reader knows no int: no bytes (the file has none either)
        return INRIA[:3] + [("confidence", "double")] + INRIA[3:20] + [("label", "int")] + INRIA[20:]
    raise KeyError(kind)


LAYOUTS = ["inria", "shuffled", "no_rest", "rest9", "uchar", "double_int", "crlf"]


def stride_of(props) -> int:
    return sum(np.dtype(NP_OF[t]).itemsize for _, t in props if t in NP_OF)


def write_ply(path, raw, props=None, eol=None, kind="inria") -> None:
    """raw (PLY-domain) splats as a binary little-endian PLY with the rows laid out as `props` say; normals and foreign properties get seeded values"""
    props = ply_layout(kind) if props is None else props
    eol = ("\r\n" if kind == "crlf" else "\n") if eol is None else eol
    n = len(raw)
    rng = np.random.default_rng(n + len(props))
    vals = {"x": raw.pos[:, 0], "y": raw.pos[:, 1], "z": raw.pos[:, 2], "opacity": raw.opacity}
    rest = np.asarray(raw.sh, f32).transpose(0, 2, 1).reshape(n, 45)                      # channel-major: the file's order
    for k in range(3): vals[f"f_dc_{k}"] = raw.dc0[:, k]; vals[f"scale_{k}"] = raw.scale[:, k]
    for k in range(4): vals[f"rot_{k}"] = raw.rot[:, k]
    for k in range(45): vals[f"f_rest_{k}"] = rest[:, k]
    dt = np.dtype([(f"{i}_{nm}", NP_OF[t]) for i, (nm, t) in enumerate(props) if t in NP_OF])
    body = np.zeros(n, dt)
    for i, (nm, t) in enumerate(props):
        if t not in NP_OF:
            continue
        body[f"{i}_{nm}"] = vals[nm] if t == "float" and nm in vals else (rng.integers(0, 200, n) if t == "uchar" else rng.normal(size=n))
    hdr = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"] + [f"property {t} {nm}" for nm, t in props] + ["end_header"]
    with open(path, "wb") as f:
        f.write((eol.join(hdr) + eol).encode("ascii"))
        f.write(body.tobytes())


def ply_rows(path, count, stride) -> np.ndarray:
    """the vertex rows of a PLY file as they lie in it: [count, stride] bytes"""
    data = open(path, "rb").read()
    at = data.index(b"end_header") + len(b"end_header")
    at += 2 if data[at:at + 2] == b"\r\n" else 1
    return np.frombuffer(data, np.uint8, count * stride, at).reshape(count, stride)


def field_of(rows, off) -> np.ndarray:
    """the float at byte `off` of every row; zeros when absent"""
    if off < 0:
        return np.zeros(len(rows), f32)
    return np.ascontiguousarray(rows[:, off:off + 4]).view("<f4").reshape(-1)


def arrays_from_rows(rows, offsets) -> creator.InputSplatData:
    """the reader's six arrays, made of the rows with the offsets gs_splat_file_open reports"""
    col = lambda k: field_of(rows, offsets[k])
    rest = np.stack([col(14 + k) for k in range(45)], 1)
    return creator.InputSplatData(pos=np.stack([col(0), col(1), col(2)], 1), dc0=np.stack([col(3), col(4), col(5)], 1),
                                  sh=rest.reshape(-1, 3, 15).transpose(0, 2, 1).copy(), opacity=col(6), scale=np.stack([col(7), col(8), col(9)], 1),
                                  rot=np.stack([col(10), col(11), col(12), col(13)], 1))


def rows_aligned(stride, offsets) -> bool:
    return stride % 4 == 0 and all(o % 4 == 0 for o in offsets[:59] if o >= 0)


# ---- SPZ ----------------------------------------------------------------------------------------------------------------------------------------
SH_COEFFS = {0: 0, 1: 3, 2: 8, 3: 15}
POSITIONS_24 = [0, 1, 0x7fffff, 0x800000, 0xffffff]
ROTATIONS = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (127, 128, 127)]


def spz_stream(n, sh_level, fract_bits, pos24, alpha, col, scale, rot, sh, header=None) -> bytes:
    """the gunzipped stream of an SPZ file from its columns: pos24 [n, 3] integers below 2^24, the rest bytes"""
    p = np.asarray(pos24, np.int64).reshape(n, 3)
    pos_b = np.stack([(p >> s) & 0xff for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    cols = [np.asarray(a, np.uint8).reshape(-1) for a in (alpha, col, scale, rot, sh)]
    assert [len(c) for c in cols] == [n, n * 3, n * 3, n * 3, n * 3 * SH_COEFFS[sh_level]]
    hdr = struct.pack("<IIII", creator.SPZ_MAGIC, 2, n, sh_level | (fract_bits << 8)) if header is None else header
    return hdr + pos_b.tobytes() + b"".join(c.tobytes() for c in cols)


def write_stream(path, stream: bytes) -> None:
    with open(path, "wb") as f:
        f.write(gzip.compress(stream, compresslevel=1))


def crafted_spz_stream(n, sh_level, fract_bits, seed=1) -> bytes:
    """n >= 256 points whose alpha, colour and scale columns each run through all 256 byte values (and the SH column too, where it has 256 bytes);
    the 24-bit positions and the rotations begin with the corner values, then a seeded sample"""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    pos = rng.integers(0, 1 << 24, (n, 3))
    for c in range(3):
        pos[:len(POSITIONS_24), c] = np.roll(POSITIONS_24, c)
    rot = rng.integers(0, 256, (n, 3))
    rot[:len(ROTATIONS)] = ROTATIONS
    odd = lambda m, a: (i * m + a) % 256                            # an odd multiplier: a permutation of the bytes every 256 points
    col = np.stack([odd(1, 0), odd(3, 85), odd(7, 170)], 1)
    scale = np.stack([odd(5, 1), odd(9, 2), odd(11, 3)], 1)
    k = SH_COEFFS[sh_level]
    sh = (np.arange(n * 3 * k, dtype=np.int64) * 37 + 11) % 256
    return spz_stream(n, sh_level, fract_bits, pos, odd(13, 7), col, scale, rot, sh)


# ---- the files the readers refuse -----------------------------------------------------------------------------------------------------------------
def refused_ply_files(tmp, raw):
    """(what, path) of PLY files gs_ply_open refuses, made from a good one"""
    good = str(tmp / "good.ply")
    write_ply(good, raw)
    txt = open(good, "rb").read()
    out = []

    def add(what, data):
        p = str(tmp / f"{what}.ply")
        open(p, "wb").write(data)
        out.append((what, p))
    add("ascii", txt.replace(b"binary_little_endian", b"ascii"))
    add("big_endian", txt.replace(b"binary_little_endian", b"binary_big_endian"))
    add("no_opacity", txt.replace(b"property float opacity", b"property float opacitx"))
    add("double_opacity", txt.replace(b"property float opacity", b"property double opacity"))
    add("no_rot_3", txt.replace(b"property float rot_3\n", b""))
    add("zero_vertices", txt.replace(f"element vertex {len(raw)}".encode(), b"element vertex 0"))
    add("negative_vertices", txt.replace(f"element vertex {len(raw)}".encode(), b"element vertex -4"))
    add("truncated_body", txt[:-5])
    add("header_only", txt[:txt.index(b"end_header") + 11])
    add("empty", b"")
    out.append(("missing", str(tmp / "missing.ply")))
    return out


def refused_spz_files(tmp, raw, sh_level=3, fract_bits=12):
    good = str(tmp / "good.spz")
    creator.WriteSPZ(good, raw, fract_bits=fract_bits, sh_level=sh_level)
    stream = gzip.decompress(open(good, "rb").read())
    n, M = len(raw), creator.SPZ_MAGIC
    out = []

    def add(what, data, gz=True):
        p = str(tmp / f"{what}.spz")
        open(p, "wb").write(gzip.compress(data) if gz else data)
        out.append((what, p))
    word = sh_level | (fract_bits << 8)
    add("not_gzip", stream, gz=False)
    add("bad_magic", struct.pack("<IIII", 0x12345678, 2, n, word) + stream[16:])
    add("bad_version", struct.pack("<IIII", M, 3, n, word) + stream[16:])
    add("no_points", struct.pack("<IIII", M, 2, 0, word) + stream[16:])
    add("too_many_points", struct.pack("<IIII", M, 2, 10_000_001, word) + stream[16:])
    add("sh_level_4", struct.pack("<IIII", M, 2, n, 4 | (fract_bits << 8)) + stream[16:])
    add("fract_bits_25", struct.pack("<IIII", M, 2, n, sh_level | (25 << 8)) + stream[16:])
    add("shorter_than_its_arrays", struct.pack("<IIII", M, 2, n + 1, word) + stream[16:])
    add("one_byte_short", stream[:-1])
    add("short_header", stream[:12])
    add("empty_stream", b"")
    out.append(("missing", str(tmp / "missing.spz")))
    return out


# ---- the two routes -------------------------------------------------------------------------------------------------------------------------------
def reader_result(path):
    """(return code, error text or None, splat count) of the reader for the path's extension; the handle is closed again"""
    l = _lib.lib()
    h, n = C.c_void_p(), C.c_uint32()
    rc = (l.gs_ply_open if path.lower().endswith(".ply") else l.gs_spz_open)(path.encode(), C.byref(h), C.byref(n))
    text = l.gs_last_error_string() if rc != 0 else None
    if rc == 0:
        l.gs_ply_close(h)
    return rc, text, n.value


def open_result(path):
    """(return code, error text or None, gs_splat_file_info) of gs_splat_file_open; the handle is closed again"""
    l = _lib.lib()
    h, info = C.c_void_p(0x1234), _abi.gs_splat_file_info()
    rc = l.gs_splat_file_open(path.encode(), C.byref(h), C.byref(info))
    text = l.gs_last_error_string() if rc != 0 else None
    if rc == 0:
        assert l.gs_splat_file_close(h) == 0
    else:
        assert not h
    return rc, text, info


def read_native(path):
    """(the reader's arrays, whether they want LinearizeData)"""
    ply = path.lower().endswith(".ply")
    return (creator.ReadPLYNative(path) if ply else creator.ReadSPZNative(path)), ply


def assert_premises(raw, linearize) -> None:
    """the importer suites' premises: finite values, no -0 among the extremes, already-linear rotations inside their fields"""
    BM.assert_no_negative_zero(creator.LinearizeData(raw) if linearize else raw)
    for a in (raw.pos, raw.dc0, raw.sh, raw.opacity, raw.scale, raw.rot):
        assert np.isfinite(np.asarray(a)).all()
    if not linearize:
        assert (np.asarray(raw.rot) >= 0).all() and (np.asarray(raw.rot) <= 1).all()


def host_route(path, morton=True, **fmt):
    """the yardstick: the host reader's arrays of the file through the host importer"""
    raw, linearize = read_native(path)
    assert_premises(raw, linearize)
    return creator.CreateAssetFromSplatsNative(raw, linearize=linearize, morton=morton, **fmt)


def check_file(ctx, path, what, morton=True, slice_bytes=0, want=None, **fmt):
    """the file straight into a GPU asset, held to the host route's asset of the same file: the five blobs and the bounds, bit for bit"""
    want = host_route(path, morton, **fmt) if want is None else want
    g = creator.CreateGpuAssetFromFile(path, morton=morton, slice_bytes=slice_bytes, context=ctx, **fmt)
    try:
        got = g.Download()
        assert g.splatCount == want.splatCount, what
        BM.assert_same_asset(got, want, what)
        for name, a, b in zip(("pos", "other", "color", "sh", "chunk"), BM.blobs_of(got), BM.blobs_of(want)):
            assert (a is None and b is None) or same_bits(a, b, None), (what, name)
        assert same_bits(got.boundsMin, want.boundsMin) and same_bits(got.boundsMax, want.boundsMax), what
    finally:
        g.Dispose()
    return want
