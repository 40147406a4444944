"""The SPZ export on the CPU box: the packer's host build (tests/spz_export_host_harness.cpp: gsm::SpzPack* of csrc/gs_device_math.h) against its numpy
twin (tests/spz_export_model.py) byte for byte; every code of every column a fixed point of reader-then-writer; the automatic fract_bits at its
boundaries; the argument checks that need no device; the harness under the host sanitizers."""
import ctypes as C

import numpy as np
import pytest

import spz_export_model as SM
from common import _p
from harness import build_harness, run_under_sanitizers
from unitygaussiansplatting_amd import _abi, _lib, creator
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

f32 = np.float32
u8 = np.uint8


@pytest.fixture(scope="module")
def sxh(tmp_path_factory):
    L = C.CDLL(build_harness(tmp_path_factory.mktemp("sxh"), "spz_export_host_harness.cpp"))
    L.sxh_auto_fract_bits.restype = C.c_uint32
    L.sxh_body_bytes.restype = C.c_uint64
    L.sxh_body_bytes.argtypes = [C.c_uint64, C.c_uint32]
    L.sxh_alive_refused.argtypes = [C.c_uint64]
    return L


def host_code8(sxh, t):
    t = np.ascontiguousarray(t, f32).reshape(-1)
    out = np.zeros(len(t), u8)
    sxh.sxh_code8(_p(t), C.c_uint64(len(t)), _p(out))
    return out


def host_coordinates(sxh, p, f):
    p = np.ascontiguousarray(p, f32).reshape(-1)
    out = np.zeros(len(p), np.uint32)
    sxh.sxh_coordinates(_p(p), C.c_uint64(len(p)), C.c_uint32(f), _p(out))
    return out


def host_rotations(sxh, wxyz):
    q = np.ascontiguousarray(wxyz, f32).reshape(-1, 4)
    out = np.zeros((len(q), 3), u8)
    sxh.sxh_rotations(_p(q), C.c_uint64(len(q)), _p(out))
    return out


def host_body(sxh, rows, opacity, sh_level, fract_bits):
    rows, opacity = np.ascontiguousarray(rows, f32).reshape(-1, 62), np.ascontiguousarray(opacity, f32)
    out = np.zeros(sxh.sxh_body_bytes(len(rows), sh_level), u8)
    sxh.sxh_body(_p(rows), _p(opacity), C.c_uint32(len(rows)), C.c_uint32(sh_level), C.c_uint32(fract_bits), _p(out))
    return out


def around(x):
    """x, and the floats just either side of it"""
    x = np.asarray(x, f32).reshape(-1)
    return np.concatenate([x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))]).astype(f32)


SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 3.4028235e38, -3.4028235e38, 1.0, -1.0], f32)
HALVES = (np.arange(-2, 258, dtype=f32) + f32(0.5)).astype(f32)   # every half-way value of an 8-bit column, and the clamps beyond both ends


def invert(fn, t):
    """the float32 inputs x at which the column's expression fn(x) comes out at (or next to) the targets t: found by bisection on the monotone fn"""
    t = np.asarray(t, f32)
    lo, hi = np.full(t.shape, -1.0e6, f32), np.full(t.shape, 1.0e6, f32)
    for _ in range(80):
        mid = ((lo.astype(np.float64) + hi.astype(np.float64)) / 2).astype(f32)
        below = fn(mid) < t
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    out = np.concatenate([lo, hi])
    for _ in range(3):                                             # a few floats either side: the tie itself, if a float hits it, is among them
        out = np.concatenate([out, np.nextafter(out, f32(np.inf)), np.nextafter(out, f32(-np.inf))])
    return np.unique(out.astype(f32))


# ---- 1. model == host build ----------------------------------------------------------------------------------------------------------------------
def test_code8_at_every_tie_and_clamp(sxh):
    t = np.concatenate([around(HALVES), around(np.arange(-2, 259, dtype=f32)), SPECIAL, around([255.0, 255.5, 256.0, 1e30, -1e30])])
    got, want = host_code8(sxh, t), SM.code8(t)
    assert np.array_equal(got, want), t[got != want][:8]
    assert SM.code8(f32(0.5)) == 0 and SM.code8(f32(1.5)) == 2 and SM.code8(f32(2.5)) == 2 and SM.code8(f32(254.5)) == 254      # ties to even
    assert SM.code8(f32(255.5)) == 255 and SM.code8(f32(np.nan)) == 0 and SM.code8(f32(-np.inf)) == 0 and SM.code8(f32(np.inf)) == 255


def test_positions_model_equals_host(sxh):
    rng = np.random.default_rng(3)
    for f in (0, 1, 11, 12, 13, 23, 24):
        s = 2.0 ** -f
        ties = (np.concatenate([np.arange(-40, 40), rng.integers(-(1 << 23), 1 << 23, 2000)]).astype(np.float64) + 0.5) * s
        edges = np.array([2.0 ** 23, 2.0 ** 23 - 1, 2.0 ** 23 - 0.5, -(2.0 ** 23), -(2.0 ** 23) - 0.5, -(2.0 ** 23) - 1, 2.0 ** 24, -(2.0 ** 24)]) * s
        p = np.concatenate([around(ties.astype(f32)), around(edges.astype(f32)), SPECIAL, rng.normal(0, 3.0, 4000).astype(f32),
                            (rng.normal(0, 1.0, 2000) * (2.0 ** (24 - f))).astype(f32)])
        got, want = host_coordinates(sxh, p, f), SM.pack_coordinates(p, f)
        assert np.array_equal(got, want), (f, p[got != want][:8])
        assert want.max() <= 0xffffff
    # ties to even, the two clamps and NaN, spelled out at fract_bits 0
    assert SM.pack_coordinates(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e9, -1e9, np.nan, np.inf, -np.inf], f32), 0).tolist() == \
        [0, 2, 2, 0, 0xfffffe, 0x7fffff, 0x800000, 0, 0x7fffff, 0x800000]
    assert SM.position_bytes(np.array([[1.0, -1.0, 258.0]], f32), 0).tolist() == [[1, 0, 0, 255, 255, 255, 2, 1, 0]]     # little-endian, x y z


def test_every_column_model_equals_host_in_whole_bodies(sxh):
    """records whose fields sweep every half-way value of their column (found by inverting the column's own expression), values either side, the
    clamps and the special values; every SH level, several fract_bits"""
    with np.errstate(all="ignore"):
        alpha = invert(lambda v: (v * f32(255.0)).astype(f32), HALVES)
        colour = invert(lambda d: (((d * f32(0.15)).astype(f32) + f32(0.5)).astype(f32) * f32(255.0)).astype(f32), HALVES)
        scale = invert(lambda s: ((s + f32(10.0)).astype(f32) * f32(16.0)).astype(f32), HALVES)
        sh = invert(lambda c: ((c * f32(128.0)).astype(f32) + f32(128.0)).astype(f32), HALVES)
    rng = np.random.default_rng(9)
    n = max(len(alpha), len(colour), len(scale), len(sh)) + len(SPECIAL)
    fill = lambda v, shape: np.resize(np.concatenate([SPECIAL, v]), shape).astype(f32)
    rows = np.zeros((n, 62), f32)
    rows[:, 0:3] = fill((np.arange(-300, 300, dtype=f32) + f32(0.5)) * f32(2.0 ** -12), (n, 3))
    rows[:, 6:9] = fill(colour, (n, 3))
    rows[:, 9:54] = fill(sh, (n, 45))
    rows[:, 55:58] = fill(scale, (n, 3))
    rows[:, 58:62] = rng.normal(0, 1, (n, 4)).astype(f32)
    opacity = fill(alpha, (n,))
    for sh_level in range(4):
        for f in (0, 12, 24):
            got, (want, used) = host_body(sxh, rows, opacity, sh_level, f), SM.body(rows, opacity, sh_level, f)
            assert used == f and np.array_equal(got, want), (sh_level, f, np.flatnonzero(got != want)[:8])
    cols = SM.split(SM.body(rows, opacity, 3, 12)[0], n, 3)
    for c in (1, 2, 3, 5):
        assert len(np.unique(cols[c])) == 256                      # the sweep reaches every code of every 8-bit column
    # the SH column is [splat][coefficient][r, g, b] of a channel-major record, cut at k coefficients
    one = np.zeros((1, 62), f32)
    one[0, 9:54] = (np.arange(45, dtype=f32) - f32(22.0)) / f32(128.0)
    one[0, 58] = 1.0
    for level, k in SM.SH_COEFFS.items():
        shc = SM.split(SM.body(one, np.zeros(1, f32), level, 0)[0], 1, level)[5].reshape(k, 3)
        assert np.array_equal(shc, np.array([[106 + j, 121 + j, 136 + j] for j in range(k)], u8).reshape(k, 3))


def test_rotations_model_equals_host(sxh):
    rng = np.random.default_rng(5)
    q = rng.normal(0, 1, (20000, 4)).astype(f32)
    q[:4000] *= rng.uniform(1e-3, 1e3, (4000, 1)).astype(f32)      # non-unit length
    q[4000:5000, 0] = 0.0                                          # w = 0
    q[5000:5500, 0] = -0.0
    q[5500:9000, 0] = -np.abs(q[5500:9000, 0])                     # w < 0
    odd = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0], [-0.0, 1, 0, 0], [np.nan, 1, 0, 0], [1, np.nan, 0, 0], [np.inf, 1, 1, 1], [1, np.inf, 0, 0],
                    [-1, -np.inf, 0, 0], [1e-30, 1e-30, 0, 0], [-1e-30, 1e-30, 0, 0], [1e30, 1e30, 1e30, 1e30], [-1e30, 1e30, 0, 0], [1e-45, 0, 0, 1e-45]], f32)
    q = np.concatenate([q, odd])
    got, want = host_rotations(sxh, q), SM.pack_rotation(q)
    assert np.array_equal(got, want), q[(got != want).any(axis=1)][:8]
    assert SM.pack_rotation(np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0], [-2, 0, 0, 2], [0, 0, 0, 0]], f32)).tolist() == \
        [[128, 128, 128], [128, 128, 128], [255, 128, 128], [128, 0, 128], [128, 128, 37], [0, 0, 0]]


# ---- 2. codes are fixed points: writer(reader(code)) == code ----------------------------------------------------------------------------------------
ALL = np.arange(256, dtype=u8)


def test_the_restated_reader_is_the_reader(tmp_path):
    """the unpack_* functions of the model against creator.ReadSPZ on a file of 256 splats that holds every code of every 8-bit column"""
    rng = np.random.default_rng(1)
    pos = rng.integers(0, 256, (256, 9)).astype(u8)
    rot = np.full((256, 3), 128, u8)
    sh = np.stack([np.roll(ALL, j) for j in range(45)], axis=1)
    body = np.concatenate([np.frombuffer(SM.header(256, 3, 12), u8), pos.reshape(-1), ALL, np.repeat(ALL, 3), np.repeat(ALL, 3), rot.reshape(-1), sh.reshape(-1)])
    path = str(tmp_path / "codes.spz")
    SM.write_gzip(path, body)
    back = creator.ReadSPZ(path)
    codes = pos.reshape(256, 3, 3).astype(np.int64)
    assert np.array_equal(back.pos, SM.unpack_coordinates(codes[..., 0] | (codes[..., 1] << 8) | (codes[..., 2] << 16), 12))
    assert np.array_equal(back.opacity, SM.unpack_alpha(ALL))
    assert np.array_equal(back.sh.reshape(256, 45), SM.unpack_sh(sh))
    assert np.array_equal(back.scale[:, 0], np.abs(creator.ExpDet((ALL.astype(f32) / f32(16.0) - f32(10.0)).astype(f32))))
    assert np.array_equal(creator.LogDet(back.scale[:, 1]), SM.unpack_scale(ALL))
    assert np.array_equal(((back.dc0[:, 2] - f32(0.5)) / f32(0.2820948)).astype(f32), SM.unpack_colour(ALL))


def test_all_256_codes_of_the_byte_columns_are_fixed_points():
    assert np.array_equal(SM.pack_alpha(SM.unpack_alpha(ALL)), ALL)
    assert np.array_equal(SM.pack_colour(SM.unpack_colour(ALL)), ALL)
    assert np.array_equal(SM.pack_scale(SM.unpack_scale(ALL)), ALL)
    assert np.array_equal(SM.pack_sh(SM.unpack_sh(ALL)), ALL)


def test_position_codes_are_fixed_points(sxh):
    rng = np.random.default_rng(2)
    codes = np.concatenate([rng.integers(0, 1 << 24, 100_000), [0, 1, 0x7fffff, 0x800000, 0xffffff]]).astype(np.uint32)
    for f in (0, 1, 12, 23, 24):
        p = SM.unpack_coordinates(codes, f)
        assert np.array_equal(SM.pack_coordinates(p, f), codes), f
        assert np.array_equal(host_coordinates(sxh, p, f), codes), f


def test_every_rotation_code_inside_the_unit_ball_is_a_fixed_point(sxh):
    """all 256^3 (x, y, z) byte triples whose decoded x x + y y + z z <= 1, as the reader computes it: 8,680,336 of them.  Beyond the unit ball the
    reader's w is 0 and its normalisation moves the code, so those are not the writer's to return."""
    g = np.arange(256, dtype=u8)
    total = 0
    for x0 in range(0, 256, 32):                                   # in slabs, to bound the memory
        b = np.stack(np.meshgrid(g[x0:x0 + 32], g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        q, sq = SM.unpack_rotation(b)
        keep = sq <= f32(1.0)
        b, q = b[keep], q[keep]
        total += len(b)
        back = SM.pack_rotation(q)
        assert np.array_equal(back, b), b[(back != b).any(axis=1)][:8]
        assert np.array_equal(host_rotations(sxh, q), b)
    assert total == 8_680_336


# ---- 3. automatic fract_bits -------------------------------------------------------------------------------------------------------------------------
def test_automatic_fract_bits_at_its_boundaries(sxh):
    def both(m, sign=1.0):
        bounds = np.array([-1.0, -0.5, -0.25, 1.0, 0.5, 0.25], f32)
        bounds[1 if sign < 0 else 4] = f32(sign * m)
        got = sxh.sxh_auto_fract_bits(_p(bounds))
        assert got == SM.auto_fract_bits_of_bounds(bounds) == SM.auto_fract_bits(bounds.reshape(2, 3)), (m, sign)
        return got

    for f in range(0, 13):
        edge = f32(2.0 ** (23 - f) - 2.0 ** (-f - 1))               # m 2^f = 2^23 - 1/2: the tie rounds to the even 2^23, which no longer fits
        assert float(edge) == 2.0 ** (23 - f) - 2.0 ** (-f - 1)
        below = np.nextafter(edge, f32(0.0))
        for sign in (1.0, -1.0):
            assert both(below, sign) == f, (f, sign)
            assert both(edge, sign) == max(f - 1, 0), (f, sign)
    assert both(f32(0.0)) == 12 == sxh.sxh_auto_fract_bits(_p(np.zeros(6, f32)))
    assert both(f32(2047.0)) == 12 and both(f32(2048.0)) == 11
    assert both(f32(2.0 ** 24)) == 0 and both(f32(1e30)) == 0 and both(f32(np.inf)) == 0
    nothing = np.array([np.inf] * 3 + [-np.inf] * 3, f32)         # a reduction over no finite position
    assert sxh.sxh_auto_fract_bits(_p(nothing)) == SM.auto_fract_bits_of_bounds(nothing) == 0 == SM.auto_fract_bits(np.full((4, 3), np.nan, f32))
    rows = np.zeros((3, 62), f32)
    rows[:, 0:3] = [[1.0, 2.0, -3000.0], [np.nan, 0.0, 0.0], [5.0, 5.0, 5.0]]
    rows[:, 58] = 1.0
    assert SM.body(rows, np.ones(3, f32), 0)[1] == 11


# ---- 4. the ABI and the checks that need no device ---------------------------------------------------------------------------------------------------
def test_spz_entry_points_validate_their_arguments(sxh):
    lib, bad = _lib.lib(), _abi.GS_ERR_INVALID_ARGUMENT
    assert C.sizeof(_abi.gs_spz_params) == 16 and _abi.GS_SPZ_FRACT_AUTO == 0xffffffff
    p, s = _abi.gs_export_params(), GaussianSplatRenderer.SpzParams()
    assert (s.sh_level, s.fract_bits, s.compression_level, s.slice_bytes) == (3, _abi.GS_SPZ_FRACT_AUTO, -1, 0)
    size, alive, fract = C.c_uint64(7), C.c_uint32(7), C.c_uint32(7)
    some = C.create_string_buffer(64)                              # never dereferenced: the NULL checks come first
    assert lib.gs_renderer_edit_export_spz_body(None, C.byref(p), C.byref(s), None, 0, C.byref(size), C.byref(alive), C.byref(fract)) == bad
    assert lib.gs_renderer_edit_export_spz_body(some, None, C.byref(s), None, 0, C.byref(size), C.byref(alive), C.byref(fract)) == bad
    assert lib.gs_renderer_edit_export_spz_body(some, C.byref(p), None, None, 0, C.byref(size), C.byref(alive), C.byref(fract)) == bad
    assert lib.gs_renderer_edit_export_spz(None, C.byref(p), C.byref(s), b"/nonexistent/x.spz", C.byref(alive)) == bad
    assert lib.gs_renderer_edit_export_spz(some, None, C.byref(s), b"/nonexistent/x.spz", C.byref(alive)) == bad
    assert lib.gs_renderer_edit_export_spz(some, C.byref(p), None, b"/nonexistent/x.spz", C.byref(alive)) == bad
    assert lib.gs_renderer_edit_export_spz(some, C.byref(p), C.byref(s), None, C.byref(alive)) == bad
    assert (size.value, alive.value, fract.value) == (7, 7, 7) and lib.gs_abi_version() == 9
    for name in ("ExportSpzFile", "ExportSpzBody", "SpzParams"):
        assert callable(getattr(GaussianSplatRenderer, name)), name


def test_parameter_and_alive_count_checks_of_the_host_code(sxh):
    ok = lambda **kw: sxh.sxh_params_refused(C.byref(GaussianSplatRenderer.SpzParams(**kw))) == 0
    assert ok() and ok(shLevel=0, fractBits=0, level=0, sliceBytes=4096) and ok(shLevel=3, fractBits=24, level=9, sliceBytes=0xffffffff)
    assert not ok(shLevel=4) and not ok(fractBits=25) and not ok(fractBits=0xfffffffe) and not ok(level=-2) and not ok(level=10)
    assert not ok(sliceBytes=1) and not ok(sliceBytes=4095)
    # the readers open 1 .. 10,000,000 splats (creator.ReadSPZ): nothing else is written
    assert sxh.sxh_alive_refused(0) == 1 and sxh.sxh_alive_refused(1) == 0
    assert sxh.sxh_alive_refused(SM.MAX_SPLATS) == 0 and sxh.sxh_alive_refused(SM.MAX_SPLATS + 1) == 1 and sxh.sxh_alive_refused(1 << 32) == 1
    for level, k in SM.SH_COEFFS.items():
        assert sxh.sxh_body_bytes(1000, level) == 16 + 1000 * (19 + 3 * k)
    assert sxh.sxh_body_bytes(SM.MAX_SPLATS, 3) == 16 + 64 * SM.MAX_SPLATS


# ---- 5. the harness under the host sanitizers ----------------------------------------------------------------------------------------------------------
def test_harness_runs_clean_under_the_host_sanitizers(tmp_path):
    r = run_under_sanitizers(tmp_path, "spz_export_host_harness.cpp", "SPZ_EXPORT_HARNESS_MAIN")
    assert r.returncode == 0 and "spz export harness ok" in r.stdout, (r.stdout, r.stderr[-2000:])
