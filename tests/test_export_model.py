"""The export on the CPU box: the C-ABI surface of the gs_renderer_edit_export_* calls, LogDet (host build = numpy twin bit for bit, and within its
documented bound of the exact logarithm), the decode premise (the reference's own LoadSplatData under the model = the host build of ExportSplat, bit
for bit), the SH rotation (host build = model in float32; model in float64 = the defining property of a rotation) and the premises of the GPU cases."""
import ctypes as C

import numpy as np
import pytest

import edit_model as EM
import export_model as XM
import ref_lib
from common import PRESETS, _p, same_bits, small_asset
from harness import build_harness
from unitygaussiansplatting_amd import _abi, _lib, camera, creator
from unitygaussiansplatting_amd.cutout import shader_data_array
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

f32 = np.float32


@pytest.fixture(scope="module")
def xh(tmp_path_factory):
    L = C.CDLL(build_harness(tmp_path_factory.mktemp("xh"), "export_host_harness.cpp"))
    L.xh_sizes.restype = C.c_uint32
    return L


def export_params(tr, bake) -> _abi.gs_export_params:
    r = GaussianSplatRenderer.__new__(GaussianSplatRenderer)      # no context: ExportParams reads the transform only
    r.transform = tr
    return r.ExportParams(bake)


def host_records(xh, asset, tr=None, bake=False, cuts=None) -> np.ndarray:
    keep = []
    desc = _abi.make_asset_desc(asset, keep)
    tr = tr or camera.Transform()
    p = export_params(tr, bake)
    arr, cnt = shader_data_array(cuts, tr.localToWorldMatrix)
    out = np.zeros((asset.splatCount, 62), f32)
    xh.xh_export(C.byref(desc), C.byref(p), arr, C.c_uint32(cnt), _p(out))
    return out


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_export_entry_points_validate_their_arguments(xh):
    lib = _lib.lib()
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    assert C.sizeof(_abi.gs_export_params) == 16 * 4 + 4 * 4 + 3 * 4 + 4 == 96 == xh.xh_sizes(1)
    assert _abi.GS_EXPORT_RECORD_BYTES == 248 == 4 * len(creator.PLY_ATTRS)
    assert xh.xh_sizes(0) == 83 * 4                               # the band matrices the kernel receives by value
    p = _abi.gs_export_params()
    buf = (C.c_float * 62)()
    alive = C.c_uint32(7)
    # a NULL renderer
    assert lib.gs_renderer_edit_export_data(None, C.byref(p), buf, C.sizeof(buf), 0) == bad
    assert lib.gs_renderer_edit_export_alive(None, C.byref(p), buf, 1, C.byref(alive)) == bad
    assert lib.gs_renderer_edit_export_ply(None, C.byref(p), b"/nonexistent/x.ply", C.byref(alive)) == bad
    # NULL params, and a buffer too small for one record: both are refused before the renderer is looked at (`some` is never dereferenced)
    some = C.create_string_buffer(64)
    assert lib.gs_renderer_edit_export_data(some, None, buf, C.sizeof(buf), 0) == bad
    assert lib.gs_renderer_edit_export_alive(some, None, buf, 1, C.byref(alive)) == bad
    assert lib.gs_renderer_edit_export_ply(some, None, b"/nonexistent/x.ply", C.byref(alive)) == bad
    assert lib.gs_renderer_edit_export_ply(some, C.byref(p), None, C.byref(alive)) == bad
    assert lib.gs_renderer_edit_export_data(some, C.byref(p), buf, 247, 0) == bad
    assert lib.gs_renderer_edit_export_data(some, C.byref(p), buf, 0, 1) == bad
    assert lib.gs_renderer_edit_export_data(some, C.byref(p), buf, C.sizeof(buf), 2) == bad      # memory_kind
    assert alive.value == 7
    assert lib.gs_abi_version() == 9                             # additions to ABI 9


def test_renderer_mirrors_the_export_methods():
    for name in ("EditExportData", "ExportAlive", "ExportPlyFile", "ExportParams"):
        assert callable(getattr(GaussianSplatRenderer, name)), name
    tr = camera.Transform(**XM.BAKE_TRANSFORM)
    p = export_params(tr, True)
    assert p.bake_transform == 1 and export_params(tr, False).bake_transform == 0
    assert np.array_equal(np.array(p.matrix_object_to_world[:], f32).reshape(4, 4), np.asarray(tr.localToWorldMatrix, f32))
    assert list(p.rotation) == [float(f32(v)) for v in tr.rotation] and list(p.scale) == [float(f32(v)) for v in tr.scale]


# ---- 2. LogDet ----------------------------------------------------------------------------------------------------------------------------
def logdet_inputs() -> np.ndarray:
    norm8 = (np.arange(256, dtype=f32) * (f32(1.0) / f32(255.0))).astype(f32)                    # every Norm8 value
    half = np.arange(65536, dtype=np.uint16).view(np.float16).astype(f32)                        # every fp16 value, NaNs and negatives included
    rng = np.random.default_rng(11)
    sweep = ((np.repeat(np.arange(256, dtype=np.uint32), 2048) << np.uint32(23)) | rng.integers(0, 1 << 23, 256 * 2048, dtype=np.uint32)).view(f32)
    edges = ((np.arange(256, dtype=np.uint32)[:, None] << np.uint32(23)) | np.array([0, 1, 0x3504f3, 0x3504f4, 0x7fffff], np.uint32)[None, :]).reshape(-1).view(f32)
    den = np.concatenate([rng.integers(1, 1 << 23, 4096, dtype=np.uint32), np.array([1, 2, 3, 0x7fffff, 0x400000], np.uint32)]).view(f32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -1e-45, 1.0, 3.4028235e38, 1.17549435e-38], f32)
    near1 = (f32(1.0) + np.arange(-4096, 4097, dtype=f32) * f32(2.0 ** -24)).astype(f32)
    return np.concatenate([norm8, half, sweep, edges, den, special, near1, -sweep[::97]])


def test_logdet_host_build_equals_the_numpy_twin(xh):
    x = logdet_inputs()
    got = np.zeros_like(x)
    xh.xh_logdet(_p(x), _p(got), C.c_uint64(len(x)))
    want = creator.LogDet(x)
    assert same_bits(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8]
    v = creator.LogDet(np.array([0.0, -0.0, np.inf, -3.0, np.nan, -np.inf], f32))
    assert v[0] == -np.inf and v[1] == -np.inf and v[2] == np.inf and np.isnan(v[3:]).all()
    assert creator.LogDet(f32(1.0)) == 0.0 and creator.LogDet(np.ones((2, 3), f32)).shape == (2, 3)


def test_logdet_stays_within_its_documented_bound():
    x = logdet_inputs()
    x = x[np.isfinite(x) & (x > 0)]
    assert (x < f32(1.1754944e-38)).sum() > 4000                  # denormals are in
    exact = np.log(x.astype(np.float64))
    err = np.abs(creator.LogDet(x).astype(np.float64) - exact)
    bound = creator.LOGDET_REL * np.abs(exact) + creator.LOGDET_ABS
    k = int(np.argmax(err / bound))
    print(f"LogDet: max |error| {err.max():.3e} (at x = {x[int(np.argmax(err))]!r}); max error / bound {err[k] / bound[k]:.3f} at x = {x[k]!r}; "
          f"max |error| on [0.5, 2] {err[(x >= 0.5) & (x <= 2)].max():.3e}")
    assert (err <= bound).all(), (x[k], err[k], bound[k])


# ---- 3. the decode premise: the reference's own LoadSplatData under the model = the host build -------------------------------------------------
@pytest.mark.parametrize("quality", PRESETS)
def test_host_build_of_the_record_equals_the_model_on_the_reference_decode(xh, quality):
    asset = small_asset(20000, 5, quality)                        # (Cluster16k needs more than 16,384 splats; the asset of the GPU cases)
    dec = ref_lib.Ref(asset, "fused").decode_all()                # skips when oracle/_ref is not built
    if not ref_lib.fused_is_pinned():
        # oracle/_ref was built by another compiler: its fused build is another member of the family (ref_lib.PINNED_COMPILER), which the host build
        # cannot equal bit for bit.  The premise then rests on the oracle's own decode, which tests/test_ref_parity.py holds to that build's bounds.
        dec = None
    m = XM.ExportModel(asset, decoded=dec)
    for name, cuts in EM.cutout_lists().items():
        m.edit.set_cutouts(cuts, camera.Transform().localToWorldMatrix)
        want = m.export_data()
        got = host_records(xh, asset, cuts=cuts)
        assert same_bits(got, want), (quality, name, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:6])
        assert int(want[:, 3].sum()) == int(m.edit.cut.sum()) and np.array_equal(want[:, 3], want[:, 5])
    assert np.isfinite(want[:, 54:58]).all() and want[:, 9:54].any()


# ---- 4. the SH rotation -----------------------------------------------------------------------------------------------------------------------
def random_rotation(rng) -> np.ndarray:
    q = rng.standard_normal(4)
    return np.asarray(camera.quat_to_mat3(q / np.linalg.norm(q)), np.float64)


def matrix4(m3, scale=(1.0, 1.0, 1.0), dtype=np.float64) -> np.ndarray:
    M = np.eye(4)
    M[:3, :3] = np.asarray(m3, np.float64) @ np.diag(scale)
    return M.astype(dtype)


PI = np.pi
# ShadeSH's constants (GaussianSplatting.hlsl:130-179) in closed form; the reference's seven-digit decimals are their roundings
C1 = np.sqrt(3.0 / (4.0 * PI))
C2 = [0.5 * np.sqrt(15.0 / PI), -0.5 * np.sqrt(15.0 / PI), 0.25 * np.sqrt(5.0 / PI), -0.5 * np.sqrt(15.0 / PI), 0.25 * np.sqrt(15.0 / PI)]
C3 = [-0.25 * np.sqrt(35.0 / (2.0 * PI)), 0.5 * np.sqrt(105.0 / PI), -0.25 * np.sqrt(21.0 / (2.0 * PI)), 0.25 * np.sqrt(7.0 / PI),
      -0.25 * np.sqrt(21.0 / (2.0 * PI)), 0.25 * np.sqrt(105.0 / PI), -0.25 * np.sqrt(35.0 / (2.0 * PI))]


def shade_basis(d) -> np.ndarray:
    """the 15 weights ShadeSH gives sh1..sh15 for direction d ([M, 3] -> [M, 15]), its basis and its signs"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([-C1 * y, C1 * z, -C1 * x,
                     C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
                     C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                     C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)], axis=1)


def test_shade_constants_are_the_references():
    ref = [0.4886025, 1.0925484, -1.0925484, 0.3153916, -1.0925484, 0.5462742, -0.5900436, 2.8906114, -0.4570458, 0.3731763, -0.4570458, 1.4453057, -0.5900436]
    assert np.allclose([C1] + C2 + C3, ref, rtol=0, atol=6e-8)


def assert_rotation_property(R, rng, what):
    """the rotated coefficients evaluated at d = the originals evaluated at R^-1 d, band by band, in float64.  Every number on either side comes out
    of fewer than 128 float64 roundings (normalisation 6, a band-2 entry <= 15, a band-3 entry <= 15 more, Dot7 13, a basis function <= 12, the sum
    over a band 13) of values bounded by sum |coefficient| x max |basis|; no basis function exceeds 0.75 on the unit sphere (the zonal ones at the
    pole are the largest: 0.4886, 0.6308, 0.7464).  The bound asserted is 128 x 2^-53 x 0.75 x sum |coefficient|."""
    bands = XM.sh_bands(matrix4(R), np.float64)
    sh = rng.standard_normal((64, 15, 3))
    out = XM.rotate_sh(sh, bands, np.float64)
    d = rng.standard_normal((64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    B, Bi = shade_basis(d), shade_basis(d @ R)                    # R^-1 d = R^T d, as rows: d R
    for lo, hi in ((0, 3), (3, 8), (8, 15)):
        got = np.einsum("nkc,nk->nc", out[:, lo:hi], B[:, lo:hi])
        want = np.einsum("nkc,nk->nc", sh[:, lo:hi], Bi[:, lo:hi])
        mag = np.abs(sh[:, lo:hi]).sum(axis=1) * 0.75
        assert np.abs(B).max() <= 0.75
        assert (np.abs(got - want) <= 128 * 2.0 ** -53 * mag).all(), (what, lo, float(np.abs(got - want).max()))


def test_sh_rotation_has_the_defining_property_in_float64():
    rng = np.random.default_rng(5)
    for k in range(40):
        assert_rotation_property(random_rotation(rng), rng, f"random {k}")
    for k in range(8):                                             # a non-uniformly scaled matrix: CalcSHRotMatrix normalises the rows
        R = random_rotation(rng)
        s = rng.uniform(0.3, 3.0, 3)
        bands = XM.sh_bands(matrix4(np.diag(s) @ R), np.float64)
        want = XM.sh_bands(matrix4(R), np.float64)
        assert all(np.abs(a - b).max() <= 64 * 2.0 ** -53 for a, b in zip(bands, want))


def quarter_turn(axis: int) -> np.ndarray:
    R = np.zeros((3, 3))
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    R[axis, axis] = 1.0
    R[b, a], R[a, b] = 1.0, -1.0
    return R


def test_sh_rotation_known_answers():
    rng = np.random.default_rng(6)
    for dtype in (np.float32, np.float64):
        for m, n in zip(XM.sh_bands(np.eye(4, dtype=dtype), dtype), (3, 5, 7)):
            assert np.array_equal(m, np.eye(n, dtype=dtype))      # identity: exactly
    sh = rng.standard_normal((5, 15, 3)).astype(f32)
    assert same_bits(XM.rotate_sh(sh, XM.sh_bands(np.eye(4, dtype=f32), f32), f32), sh)
    for axis in range(3):
        R = quarter_turn(axis)
        assert np.isclose(np.linalg.det(R), 1.0)
        assert_rotation_property(R, rng, f"quarter turn about axis {axis}")
        b1 = XM.sh_bands(matrix4(R), np.float64)[0]
        assert set(np.abs(b1).reshape(-1).tolist()) == {0.0, 1.0} and (np.abs(b1).sum(axis=0) == 1).all()      # band 1 permutes (with signs)
        four = np.linalg.matrix_power                              # four quarter turns are the identity, band by band
        for m in XM.sh_bands(matrix4(R), np.float64):
            assert np.abs(four(m, 4) - np.eye(len(m))).max() <= 64 * 2.0 ** -53
    for axis in range(3):                                          # a negative scale on one axis: a mirror; the bands are diagonal signs
        s = [1.0, 1.0, 1.0]
        s[axis] = -1.0
        bands = XM.sh_bands(matrix4(np.eye(3), s), np.float64)
        for m in bands:
            assert np.array_equal(np.abs(m), np.eye(len(m))), (axis, m)
        assert_rotation_property(np.diag(s), rng, f"mirror of axis {axis}")      # (an improper R: the property holds for it all the same)
        # ... and the quaternion's axis-flip branch: the two OTHER components change sign before QuatMul with the identity rotation
        dec = np.zeros((1, 59), f32)
        dec[0, 3:7] = (0.1, 0.2, 0.3, 0.9)
        dec[0, 7:10] = (1.0, 2.0, 3.0)
        dec[0, 10] = 0.5
        rec = XM.export_records(dec, [False], (matrix4(np.eye(3), s, f32), (0.0, 0.0, 0.0, 1.0), s))
        want = np.array([0.1, 0.2, 0.3], f32)
        want[[k for k in range(3) if k != axis]] *= f32(-1.0)
        assert rec[0, 58] == f32(0.9) and np.array_equal(rec[0, 59:62], want)
        assert same_bits(rec[0, 55:58], creator.LogDet(np.array([1.0, 2.0, 3.0], f32)))      # scale *= |bakeScale|


def test_sh_rotation_host_build_equals_the_model_in_float32(xh):
    rng = np.random.default_rng(7)
    mats = [np.eye(4, dtype=f32)] + [matrix4(quarter_turn(a), dtype=f32) for a in range(3)]
    mats += [matrix4(np.eye(3), s, f32) for s in ((-1, 1, 1), (1, -1, 1), (1, 1, -1))]
    mats += [matrix4(random_rotation(rng), rng.uniform(0.2, 4.0, 3) * rng.choice([-1.0, 1.0], 3), f32) for _ in range(200)]
    mats.append(np.asarray(camera.Transform(**XM.BAKE_TRANSFORM).localToWorldMatrix, f32))
    for i, M in enumerate(mats):
        M = np.ascontiguousarray(M, f32)
        M[:3, 3] = rng.standard_normal(3).astype(f32)             # the translation does not enter
        got = np.zeros(83, f32)
        xh.xh_bands(_p(M), _p(got))
        want = np.concatenate([b.reshape(-1) for b in XM.sh_bands(M, f32)])
        assert same_bits(got, want), (i, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])


@pytest.mark.parametrize("quality", ["Medium", "VeryHigh"])
def test_host_build_of_the_baked_record_equals_the_model(xh, quality):
    asset = small_asset(5003, 5, quality)
    m = XM.ExportModel(asset)
    transforms = [camera.Transform(**XM.BAKE_TRANSFORM), camera.Transform(position=(0.1, 0.2, 0.3), rotation=(0.0, 0.0, 0.0, 1.0), scale=(1.0, -2.0, 1.0)),
                  camera.Transform(rotation=(0.5, 0.5, 0.5, 0.5), scale=(1.0, 1.0, -0.5))]
    cuts = EM.cutout_lists()["ellipsoid+inverted box"]
    for tr in transforms:
        m.edit.set_cutouts(cuts, tr.localToWorldMatrix)
        want = m.export_data(tr, True)
        got = host_records(xh, asset, tr, True, cuts)
        assert same_bits(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:6]
        assert not same_bits(want[:, 9:54], m.export_data()[:, 9:54])      # the bake did something to the SH
        assert 0 < int(want[:, 3].sum()) < m.n                    # cut on the OBJECT-space position, whatever was baked


# ---- 5. premises of the GPU cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", PRESETS)
def test_every_pattern_leaves_the_stated_number_alive(quality):
    m = XM.ExportModel(small_asset(20000, 5, quality))
    assert m.n == 20000 == 78 * 256 + 32
    for name in XM.PATTERNS:
        XM.apply_pattern(m, name, camera.Transform().localToWorldMatrix)
        alive = int(m.alive().sum())
        print(quality, name, "alive", alive, "deleted", int(m.deleted().sum()), "cut", int(m.edit.cut.sum()))
        if name in XM.ALIVE_20000:
            assert alive == XM.ALIVE_20000[name], (name, alive)
        else:                                                      # the random half under the two cutouts: all three of deleted, cut and alive matter
            assert alive == XM.ALIVE_HALF_20000[quality] and int(m.deleted().sum()) == 10088 and int(m.edit.cut.sum()) == 15183
            assert 1000 <= int((m.deleted() & m.edit.cut).sum())
        assert len(m.export_alive()) == alive
    assert np.flatnonzero(m.alive()).tolist() == [19999]


def test_the_tail_bits_of_33_splats_export_nothing():
    m = XM.ExportModel(EM.point_asset(33))
    m.edit.select_all()
    m.edit.delete_selected()
    assert m.edit.bits()[2].tolist() == [0xFFFFFFFF, 0xFFFFFFFF]  # the deleted bits beyond N are set
    assert m.edit.info()[1] == 64                                  # ... and counted by the edit info: 31 phantoms
    assert int(m.alive().sum()) == 0 and len(m.export_alive()) == 0 and len(m.export_data()) == 33


def test_ply_of_the_model_reads_back(tmp_path):
    m = XM.ExportModel(small_asset(5003, 5, "Medium"))
    XM.apply_pattern(m, "half deleted under cutouts", camera.Transform().localToWorldMatrix)
    rows = m.export_alive()
    path = str(tmp_path / "m.ply")
    creator.WritePLY(path, XM.columns(rows))
    back = creator.ReadPLY(path)
    assert same_bits(back.pos, rows[:, 0:3]) and same_bits(back.sh.transpose(0, 2, 1).reshape(len(rows), 45), rows[:, 9:54])
    assert same_bits(back.rot, rows[:, 58:62]) and same_bits(back.opacity, rows[:, 54])
