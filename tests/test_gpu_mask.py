"""-m gpu: the screen mask drawn on the GPU (gs_mask_*; csrc/gs_mask.hip) against the brute-force float32 twin of
tests/mask_model.py: the downloaded words are the twin's words, every bit -- polygons by the even-odd rule, round-capped strokes, set and subtract -- the
bits beyond W stay zero after every call, and every refusal leaves the mask as it was."""
import ctypes as C
import functools

import numpy as np
import pytest

import mask_model as MM
from gpu_rig import BAD
from unitygaussiansplatting_amd import _lib
from unitygaussiansplatting_amd._lib import GsError
from unitygaussiansplatting_amd.renderer import ScreenMask

pytestmark = pytest.mark.gpu
f32 = np.float32
_FP = C.POINTER(C.c_float)
IDS = lambda s: f"{s[0]}x{s[1]}"


def assert_words(mask: ScreenMask, want: np.ndarray, what):
    got = mask.DownloadWords()
    assert MM.padding_bits(got, mask.width) == 0, (what, "a bit beyond W is set")
    ww = MM.words(want)
    assert np.array_equal(got, ww), (what, int((MM.from_words(got, mask.width) != want).sum()), np.argwhere(got != ww)[:6].tolist())


@pytest.mark.parametrize("size", MM.SIZES, ids=IDS)
def test_polygons_equal_the_twin(gpu_ctx, size):
    w, h = size
    m = gpu_ctx.CreateScreenMask(w, h)
    assert not m.DownloadWords().any(), "a new mask is zeroed"
    for name, pts in MM.polygon_cases(w, h):
        m.Clear()
        m.FillPolygon(pts)
        assert_words(m, MM.polygon_coverage(w, h, pts), (name, size))
    m.Dispose()


@pytest.mark.parametrize("size", MM.SIZES, ids=IDS)
def test_strokes_equal_the_twin(gpu_ctx, size):
    w, h = size
    m = gpu_ctx.CreateScreenMask(w, h)
    for name, pts, radius in MM.stroke_cases(w, h) + [("seeded 1000 segments", MM.random_stroke(w, h, 1001, 31), 2.4)]:
        m.Clear()
        m.Stroke(pts, radius)
        want = MM.stroke_coverage(w, h, pts, radius)
        assert_words(m, want, (name, size))
        if name == "one point, radius 0.5":
            assert want.sum() == 1 and want[h // 2, w // 2]
    m.Dispose()


@functools.lru_cache(maxsize=None)
def big_expected():
    """the twin's masks of the 1200 x 797 case, computed once"""
    w, h = MM.BIG
    lasso, star, brush = MM.radial_lasso(w, h, 4097, 77), MM.scaled(MM.PENTAGRAM, w, h), MM.random_stroke(w, h, 13, 5)
    a = MM.polygon_coverage(w, h, lasso)
    b = MM.apply(a, MM.polygon_coverage(w, h, star), True)
    c = MM.apply(b, MM.stroke_coverage(w, h, brush, 20.0), False)
    d = MM.apply(c, MM.stroke_coverage(w, h, brush[3:9], 7.5), True)
    return (lasso, star, brush), (a, b, c, d)


def test_the_1200x797_case_set_then_subtract(gpu_ctx):
    w, h = MM.BIG
    (lasso, star, brush), (a, b, c, d) = big_expected()
    assert 0.05 < a.mean() < 0.95 and (a & ~b).any() and (c & ~b).any() and (c & ~d).any()
    m = gpu_ctx.CreateScreenMask(w, h)
    m.FillPolygon(lasso)
    assert_words(m, a, "lasso of 4097 vertices")
    m.FillPolygon(star, subtract=True)
    assert_words(m, b, "minus a pentagram")
    m.Stroke(brush, 20.0)
    assert_words(m, c, "plus a stroke of radius 20")
    m.Stroke(brush[3:9], 7.5, subtract=True)
    assert_words(m, d, "minus a thinner stroke")
    m.Dispose()


@pytest.mark.parametrize("size", [(33, 2), (257, 65)], ids=IDS)
def test_set_then_subtract_on_a_random_start(gpu_ctx, size):
    w, h = size
    rng = np.random.default_rng(w)
    start = rng.random((h, w)) < 0.5
    m = gpu_ctx.CreateScreenMask(w, h)
    m.Upload(start)
    assert_words(m, start, "upload")
    lasso, inner, pts = MM.radial_lasso(w, h, 300, 5), MM.scaled(MM.BOW_TIE, w, h), MM.random_stroke(w, h, 60, 8)
    want = MM.apply(start, MM.polygon_coverage(w, h, lasso), False)
    m.FillPolygon(lasso)
    assert_words(m, want, "set")
    want = MM.apply(want, MM.polygon_coverage(w, h, inner), True)
    m.FillPolygon(inner, subtract=True)
    assert_words(m, want, "subtract")
    want = MM.apply(want, MM.stroke_coverage(w, h, pts, 1.7), True)
    m.Stroke(pts, 1.7, subtract=True)
    assert_words(m, want, "stroke subtract")
    want = MM.apply(want, MM.stroke_coverage(w, h, pts[::-1], 0.9), False)
    m.Stroke(pts[::-1], 0.9)
    assert_words(m, want, "stroke set")
    assert np.array_equal(m.Download(), want)
    m.Dispose()


@pytest.mark.parametrize("size", [(1, 1), (31, 3), (33, 2), (257, 65)], ids=IDS)
def test_padding_bits_after_an_upload_of_all_ones(gpu_ctx, size):
    w, h = size
    m = gpu_ctx.CreateScreenMask(w, h)
    m.UploadWords(np.full((h, MM.row_words(w)), 0xFFFFFFFF, np.uint32))
    assert_words(m, np.ones((h, w), bool), "all ones")
    m.Stroke([(w / 2, h / 2)], 65536.0, subtract=True)
    assert_words(m, np.zeros((h, w), bool), "the largest brush clears everything")
    m.FillPolygon([(-10, -10), (w + 10, -10), (w + 10, h + 10), (-10, h + 10)])
    assert_words(m, np.ones((h, w), bool), "a polygon around the screen")
    m.Clear()
    assert not m.DownloadWords().any()
    m.Dispose()


def test_refusals_leave_the_mask_unchanged(gpu_ctx):
    w, h = 70, 9
    lib = _lib.lib()
    m = gpu_ctx.CreateScreenMask(w, h)
    start = np.random.default_rng(3).random((h, w)) < 0.5
    m.Upload(start)
    ok = np.array([(1.0, 1.0), (60.0, 2.0), (30.0, 8.0)], f32)

    def poly(p, count=None, sub=0):
        p = np.ascontiguousarray(p, f32)
        return lib.gs_mask_fill_polygon(m._h, p.ctypes.data_as(_FP), len(p) if count is None else count, sub)

    def stroke(p, radius, count=None, sub=0):
        p = np.ascontiguousarray(p, f32)
        return lib.gs_mask_stroke(m._h, p.ctypes.data_as(_FP), len(p) if count is None else count, C.c_float(radius), sub)

    for bad in (np.nan, np.inf, -np.inf, 65537.0, -70000.0, float(np.nextafter(f32(65536.0), f32(np.inf)))):
        for k in range(3):
            for c in range(2):
                p = ok.copy()
                p[k, c] = bad
                assert MM.refused(p, 3) and MM.refused(p, 1, 2.0)
                assert poly(p) == BAD and poly(p, sub=1) == BAD and stroke(p, 2.0) == BAD and stroke(p, 2.0, sub=1) == BAD, (bad, k, c)
    assert poly(ok, count=2) == BAD and poly(ok, count=0) == BAD and poly(ok, count=65537) == BAD         # V = 2
    assert stroke(ok, 2.0, count=0) == BAD and stroke(ok, 2.0, count=65537) == BAD                           # P = 0
    for r in (0.0, -1.0, np.nan, np.inf, 65536.5):
        assert MM.refused(ok, 1, r) and stroke(ok, r) == BAD and stroke(ok, r, sub=1) == BAD, r
    assert lib.gs_mask_fill_polygon(m._h, None, 3, 0) == BAD and lib.gs_mask_stroke(m._h, None, 1, C.c_float(1.0), 0) == BAD
    buf = np.full(h * MM.row_words(w) + 1, 0xFFFFFFFF, np.uint32)
    for count in (0, h * MM.row_words(w) - 1, h * MM.row_words(w) + 1):
        assert lib.gs_mask_upload(m._h, buf.ctypes.data, count) == BAD and lib.gs_mask_download(m._h, buf.ctypes.data, count) == BAD, count
    assert (buf == 0xFFFFFFFF).all(), "a refused download wrote"
    with pytest.raises(GsError):
        m.Upload(np.zeros((h, w + 1), bool))
    with pytest.raises(GsError):
        m.FillPolygon(np.zeros((4, 3), f32))
    assert_words(m, start, "after the refusals")
    for bad_size in ((0, 4), (4, 0), (65536, 4), (4, 65536)):
        hnd = C.c_void_p()
        assert lib.gs_mask_create(gpu_ctx._h, bad_size[0], bad_size[1], C.byref(hnd)) == BAD and not hnd
    # the limits themselves are accepted
    m.Stroke(ok, 65536.0)
    assert_words(m, np.ones((h, w), bool), "radius 65536")
    m.Dispose()


def test_the_largest_vertex_count(gpu_ctx):
    """65,536 vertices on a screen of two rows (the twin walks every edge): the outline's device copy grows past every earlier call's"""
    w, h = 33, 2
    m = gpu_ctx.CreateScreenMask(w, h)
    m.FillPolygon(MM.scaled(MM.TRIANGLE, w, h))
    lasso = MM.radial_lasso(w, h, 65536, 11)
    m.FillPolygon(lasso, subtract=True)
    want = MM.apply(MM.polygon_coverage(w, h, MM.scaled(MM.TRIANGLE, w, h)), MM.polygon_coverage(w, h, lasso), True)
    assert_words(m, want, "65536 vertices")
    m.Dispose()
