"""CPU: gsm::Mask* (csrc/gs_device_math.h) compiled for the host with tests/harness.py's line and run by tests/mask_host_harness.cpp the way the kernels of
gs_mask.hip run them -- boundary counts, one XOR per crossing and a suffix parity for the polygon; the conservative box of each segment for the stroke --
held to the brute-force twin of tests/mask_model.py bit for bit on the cases the GPU suite uses; the boundary count against the per-pixel comparison for
crossing values around every half-integer; and gsm::EditSelectionMaskHit against the selection twin."""
import ctypes as C

import numpy as np
import pytest

import edit_model as EM
import mask_model as MM
from common import default_camera
from harness import build_harness
from unitygaussiansplatting_amd import camera
from unitygaussiansplatting_amd._abi import gs_frame_params

f32 = np.float32
_FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def mh(tmp_path_factory):
    lib = C.CDLL(build_harness(tmp_path_factory.mktemp("mask"), "mask_host_harness.cpp"))
    lib.mh_boundary_count.restype = C.c_uint32
    lib.mh_boundary_count.argtypes = [C.c_float, C.c_uint32]
    lib.mh_fill_polygon.restype = None
    lib.mh_fill_polygon.argtypes = [C.c_uint32, C.c_uint32, _FP, C.c_uint32, C.c_int32, C.c_void_p]
    lib.mh_stroke.restype = C.c_uint64
    lib.mh_stroke.argtypes = [C.c_uint32, C.c_uint32, _FP, C.c_uint32, C.c_float, C.c_int32, C.c_void_p]
    lib.mh_selection_hits.restype = None
    lib.mh_selection_hits.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(gs_frame_params), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.mh_coord_ok.restype = C.c_int32
    lib.mh_coord_ok.argtypes = [C.c_float]
    return lib


def host_polygon(mh, w, h, pts, start=None, subtract=False):
    p = np.ascontiguousarray(pts, f32).reshape(-1, 2)
    wd = np.zeros((h, MM.row_words(w)), np.uint32) if start is None else MM.words(start)
    mh.mh_fill_polygon(w, h, p.ctypes.data_as(_FP), len(p), int(subtract), wd.ctypes.data)
    return wd


def host_stroke(mh, w, h, pts, radius, start=None, subtract=False):
    p = np.ascontiguousarray(pts, f32).reshape(-1, 2)
    wd = np.zeros((h, MM.row_words(w)), np.uint32) if start is None else MM.words(start)
    tests = mh.mh_stroke(w, h, p.ctypes.data_as(_FP), len(p), radius, int(subtract), wd.ctypes.data)
    return wd, tests


@pytest.mark.parametrize("size", MM.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_polygons_equal_the_twin(mh, size):
    w, h = size
    for name, pts in MM.polygon_cases(w, h):
        got = host_polygon(mh, w, h, pts)
        assert np.array_equal(got, MM.words(MM.polygon_coverage(w, h, pts))), (name, size)
        assert MM.padding_bits(got, w) == 0, name


@pytest.mark.parametrize("size", MM.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_strokes_equal_the_twin(mh, size):
    w, h = size
    for name, pts, radius in MM.stroke_cases(w, h) + [("seeded 1000 segments", MM.random_stroke(w, h, 1001, 31), 2.4)]:
        got, _ = host_stroke(mh, w, h, pts, radius)
        assert np.array_equal(got, MM.words(MM.stroke_coverage(w, h, pts, radius))), (name, size)
        assert MM.padding_bits(got, w) == 0, name


def test_host_set_then_subtract_and_the_work_of_a_stroke(mh):
    w, h = 257, 65
    rng = np.random.default_rng(2)
    start = rng.random((h, w)) < 0.5
    lasso, inner = MM.radial_lasso(w, h, 300, 5), MM.scaled(MM.PENTAGRAM, w, h)
    a = MM.apply(start, MM.polygon_coverage(w, h, lasso), False)
    b = MM.apply(a, MM.polygon_coverage(w, h, inner), True)
    got = host_polygon(mh, w, h, inner, start=MM.from_words(host_polygon(mh, w, h, lasso, start=start), w), subtract=True)
    assert np.array_equal(got, MM.words(b)) and not np.array_equal(MM.words(a), MM.words(b))
    pts = MM.random_stroke(w, h, 200, 8)
    got, tests = host_stroke(mh, w, h, pts, 2.0, start=start, subtract=True)
    assert np.array_equal(got, MM.words(MM.apply(start, MM.stroke_coverage(w, h, pts, 2.0), True)))
    assert tests < 0.2 * w * h * 199, "the stroke tests the pixels of the boxes, not every pixel for every segment"


def test_boundary_count_equals_the_per_pixel_comparison(mh):
    """k = #{x in [0, W): x + 0.5 < xs}, for crossing values at, just below and just above every half-integer and integer, below 0, above W, and the specials"""
    for w in (1, 31, 32, 33, 257, 65535):
        xc = MM.centres(w)
        base = np.concatenate([np.arange(-3, min(w, 300) + 4), np.arange(max(0, w - 300), w + 4)]).astype(np.float64)
        vals = np.concatenate([base, base + 0.5]).astype(f32)
        vals = np.concatenate([vals, np.nextafter(vals, f32(np.inf)), np.nextafter(vals, f32(-np.inf)), np.nextafter(np.nextafter(vals, f32(np.inf)), f32(np.inf))])
        vals = np.concatenate([vals, np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 3.0e38, -3.0e38, 65536.0, 131072.0, 8388608.5, 16777216.0], f32)])
        for xs in vals:
            with np.errstate(invalid="ignore"):
                want = int((xc < xs).sum())
            assert mh.mh_boundary_count(float(xs), w) == want, (w, float(xs))


def test_coordinate_limit(mh):
    for v, ok in ((0.0, 1), (65536.0, 1), (-65536.0, 1), (np.nextafter(f32(65536.0), f32(np.inf)), 0), (np.nan, 0), (np.inf, 0), (-np.inf, 0)):
        assert mh.mh_coord_ok(float(v)) == ok, v


@pytest.mark.parametrize("cuts", ["none", "ellipsoid+inverted box"])
def test_host_selection_hits_equal_the_twin(mh, cuts):
    n, k = 2000, 77
    asset = EM.point_asset(n, nan_at=k)
    model = EM.EditModel(asset)
    tr = camera.Transform()
    model.set_cutouts(EM.cutout_lists()[cuts], tr.localToWorldMatrix)
    for cam in (default_camera(W=64, H=40), EM.inside_camera()):
        W, H = cam.pixelWidth, cam.pixelHeight
        P = camera.frame_params(cam, tr)
        for mask in (MM.polygon_coverage(W, H, MM.scaled(MM.PENTAGRAM, W, H)), np.ones((H, W), bool), np.zeros((H, W), bool)):
            want = MM.mask_hit_flags(model.clip_positions(P), model.cut, mask)
            got = np.zeros(n, np.uint8)
            wd = MM.words(mask)
            pos = np.ascontiguousarray(asset.posData).view(f32)
            cptr = C.cast(model.cutouts, C.c_void_p) if model.cutout_count else None
            mh.mh_selection_hits(pos.ctypes.data, n, C.byref(P), cptr, model.cutout_count, wd.ctypes.data, W, H, got.ctypes.data)
            assert np.array_equal(got.astype(bool), want), (cuts, W, H)
            assert not got[k], "a NaN position hits nothing"
            if mask.all():
                assert 0 < want.sum() < n
