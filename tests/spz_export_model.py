"""The yardstick of the SPZ export (helper, not a test): a numpy twin of the packer, written from its specification and not
from the C++.  The body of an SPZ version 2 stream for n splats is a 16-byte header -- "NGSP", version 2, n, sh_level | fract_bits << 8 -- and six
columns in file order: positions n x 9, alpha n, colour n x 3, scale n x 3, rotation n x 3, SH n x 3k with k = 0, 3, 8, 15.

Inputs are the [n, 62] export records (tests/export_model.py: pos, nor, f_dc, 45 f_rest channel-major, opacity logit, log scale, rot wxyz) and,
for alpha, the decoded LINEAR opacity of the same splats.  All arithmetic is float32, every product and every sum rounded on its own; rounding to
an integer is to nearest, ties to even.
    code8(t)  = 0 if not t >= 0 (NaN, -inf), 255 if t > 255, else rint(t)
    position  q = rint(p * 2^f), clamped to [-2^23, 2^23 - 1], NaN -> 0; three bytes little-endian per coordinate
    alpha     code8(v * 255)
    colour    code8(((dc0 * 0.15) + 0.5) * 255)
    scale     code8((s + 10) * 16)
    rotation  l2 = ((x x + y y) + z z) + w w;  q * (1 / sqrt(l2));  all four negated if w < 0;  code8((c * 127.5) + 127.5) for x, y, z
    SH        code8((c * 128) + 128), laid out [splat][coefficient][r, g, b]
Automatic fract_bits: the largest f <= 12 with rint(m * 2^f) <= 2^23 - 1, m the largest |coordinate|; 0 if none.

The second half restates what the project's readers do with a code (creator.ReadSPZ) and what the export does with the reader's value on its way
back into a record: the round trip the fixed-point tests of tests/test_spz_export_model.py walk."""
from __future__ import annotations

import struct

import numpy as np

from unitygaussiansplatting_amd import creator

f32 = np.float32
SH_COEFFS = {0: 0, 1: 3, 2: 8, 3: 15}
MAX_SPLATS = 10_000_000
FRACT_AUTO = None


def code8(t) -> np.ndarray:
    t = np.asarray(t, f32)
    with np.errstate(all="ignore"):
        inside = (t >= f32(0.0)) & ~(t > f32(255.0))               # NaN compares false: code 0
        r = np.rint(np.where(inside, t, f32(0.0))).astype(np.uint8)
        return np.where(t > f32(255.0), np.uint8(255), np.where(inside, r, np.uint8(0))).astype(np.uint8)


def pack_coordinates(p, fract_bits: int) -> np.ndarray:
    """the 24-bit two's complement codes, as uint32"""
    p = np.asarray(p, f32)
    with np.errstate(all="ignore"):
        q = np.rint((p * f32(2.0 ** fract_bits)).astype(f32))
        q = np.where(np.isnan(q), f32(0.0), np.clip(q, f32(-(2.0 ** 23)), f32(2.0 ** 23 - 1)))
    return (q.astype(np.int64) & 0xffffff).astype(np.uint32)


def position_bytes(pos, fract_bits: int) -> np.ndarray:
    q = pack_coordinates(pos, fract_bits).reshape(-1, 3)
    return np.stack([(q >> s) & 0xff for s in (0, 8, 16)], axis=-1).astype(np.uint8).reshape(len(q), 9)


def pack_alpha(v) -> np.ndarray:
    with np.errstate(all="ignore"):
        return code8((np.asarray(v, f32) * f32(255.0)).astype(f32))


def pack_colour(dc0) -> np.ndarray:
    with np.errstate(all="ignore"):
        t = (np.asarray(dc0, f32) * f32(0.15)).astype(f32)
        t = (t + f32(0.5)).astype(f32)
        return code8((t * f32(255.0)).astype(f32))


def pack_scale(s) -> np.ndarray:
    with np.errstate(all="ignore"):
        t = (np.asarray(s, f32) + f32(10.0)).astype(f32)
        return code8((t * f32(16.0)).astype(f32))


def pack_sh(c) -> np.ndarray:
    with np.errstate(all="ignore"):
        t = (np.asarray(c, f32) * f32(128.0)).astype(f32)
        return code8((t + f32(128.0)).astype(f32))


def pack_rotation(wxyz) -> np.ndarray:
    """[n, 4] (w, x, y, z) -> [n, 3] bytes of x, y, z"""
    q = np.asarray(wxyz, f32).reshape(-1, 4)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    with np.errstate(all="ignore"):
        l2 = (((x * x).astype(f32) + (y * y).astype(f32)).astype(f32) + (z * z).astype(f32)).astype(f32)
        l2 = (l2 + (w * w).astype(f32)).astype(f32)
        inv = (f32(1.0) / np.sqrt(l2).astype(f32)).astype(f32)
        c = (q[:, 1:4] * inv[:, None]).astype(f32)
        c = np.where((w < f32(0.0))[:, None], -c, c)
        return code8(((c * f32(127.5)).astype(f32) + f32(127.5)).astype(f32))


def auto_fract_bits(pos) -> int:
    pos = np.asarray(pos, f32).reshape(-1, 3)
    lo = np.fmin.reduce(pos, axis=0, initial=f32(np.inf))           # what a min / max reduction leaves: a NaN never wins, nothing = +-inf
    hi = np.fmax.reduce(pos, axis=0, initial=f32(-np.inf))
    return auto_fract_bits_of_bounds(np.concatenate([lo, hi]))


def auto_fract_bits_of_bounds(bounds) -> int:
    m = np.fmax.reduce(np.abs(np.asarray(bounds, f32)), initial=f32(0.0))
    with np.errstate(all="ignore"):
        for f in range(12, 0, -1):
            if np.rint(f32(m) * f32(2.0 ** f)) <= f32(2.0 ** 23 - 1):
                return f
    return 0


def header(n: int, sh_level: int, fract_bits: int) -> bytes:
    return struct.pack("<IIII", 0x5053474e, 2, n, sh_level | (fract_bits << 8))


def body(rows, opacity, sh_level: int = 3, fract_bits=FRACT_AUTO):
    """(the gunzipped stream as a uint8 array, fract_bits used) for [n, 62] export records and their n linear opacities"""
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 62)
    n, k = len(rows), SH_COEFFS[sh_level]
    f = auto_fract_bits(rows[:, 0:3]) if fract_bits is None else int(fract_bits)
    sh = rows[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1)[:, :k, :]      # channel-major in the record -> [coefficient][r, g, b]
    parts = [np.frombuffer(header(n, sh_level, f), np.uint8), position_bytes(rows[:, 0:3], f).reshape(-1), pack_alpha(opacity).reshape(-1),
             pack_colour(rows[:, 6:9]).reshape(-1), pack_scale(rows[:, 55:58]).reshape(-1), pack_rotation(rows[:, 58:62]).reshape(-1),
             pack_sh(sh).reshape(-1)]
    out = np.concatenate(parts).astype(np.uint8)
    assert len(out) == 16 + n * (19 + 3 * k)
    return out, f


def split(body_bytes, n: int, sh_level: int):
    """the six columns of a body, as [n, width] uint8 views"""
    k = SH_COEFFS[sh_level]
    out, at = [], 16
    for w in (9, 1, 3, 3, 3, 3 * k):
        out.append(np.asarray(body_bytes[at:at + n * w], np.uint8).reshape(n, w))
        at += n * w
    assert at == len(body_bytes)
    return out


# ---- what a reader makes of a code, and the export of that value (creator.ReadSPZ; CSExportData through tests/export_model.py) ------------------
def unpack_coordinates(codes, fract_bits: int) -> np.ndarray:
    fx = np.asarray(codes, np.int64)
    fx = np.where(fx & 0x800000, fx - (1 << 24), fx)
    return (fx.astype(f32) * f32(1.0 / (1 << fract_bits))).astype(f32)


def unpack_alpha(b) -> np.ndarray:
    """the reader's linear opacity: the value the writer's alpha is taken of"""
    return (np.asarray(b, np.uint8).astype(f32) / f32(255.0)).astype(f32)


def unpack_colour(b) -> np.ndarray:
    """the reader's linear colour SH0ToColor((b / 255 - 0.5) / 0.15), then the record's f_dc = ColorToSH0 of it"""
    col = ((np.asarray(b, np.uint8).astype(f32) / f32(255.0) - f32(0.5)) / f32(0.15)).astype(f32)
    lin = creator.SH0ToColor(col)
    return ((lin - f32(0.5)) / f32(0.2820948)).astype(f32)


def unpack_scale(b) -> np.ndarray:
    """the reader's linear scale |ExpDet(b / 16 - 10)|, then the record's LogDet of it"""
    lin = np.abs(creator.ExpDet((np.asarray(b, np.uint8).astype(f32) / f32(16.0) - f32(10.0)).astype(f32))).astype(f32)
    return creator.LogDet(lin)


def unpack_sh(b) -> np.ndarray:
    return ((np.asarray(b, np.uint8).astype(f32) - f32(128.0)) / f32(128.0)).astype(f32)


def unpack_rotation(b):
    """([n, 4] (w, x, y, z) normalised as the reader does, the reader's x x + y y + z z before it takes w) for [n, 3] bytes"""
    xyz = (np.asarray(b, np.uint8).reshape(-1, 3).astype(f32) * f32(1.0 / 127.5) - f32(1.0)).astype(f32)
    sq = ((xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2]).astype(f32)
    w = np.sqrt(np.maximum(f32(0.0), f32(1.0) - sq)).astype(f32)
    l2 = (sq + w * w).astype(f32)
    inv = (f32(1.0) / np.sqrt(l2).astype(f32)).astype(f32)
    return np.concatenate([(w * inv)[:, None], xyz * inv[:, None]], axis=1).astype(f32), sq


def write_gzip(path: str, body_bytes) -> None:
    """a body as a file the readers open (the bytes of gzip are nobody's concern)"""
    import gzip
    with open(path, "wb") as f:
        f.write(gzip.compress(np.asarray(body_bytes, np.uint8).tobytes(), compresslevel=1))


def read_gzip(path: str) -> np.ndarray:
    import gzip
    with open(path, "rb") as f:
        return np.frombuffer(gzip.decompress(f.read()), np.uint8)
