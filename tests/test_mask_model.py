"""CPU: the premises of tests/mask_model.py, the numpy twin the GPU's screen mask and the two selecting calls are held to -- the even-odd rule leaves the
holes it should, the <= rule decides vertices on pixel centres, a horizontal edge on a row's centre line never crosses, a disc of radius 0.5 on a pixel
centre is that pixel -- and the new entry points refuse their arguments without a device."""
import ctypes as C

import numpy as np

import edit_model as EM
import mask_model as MM
import pick_model as PM
from unitygaussiansplatting_amd import _abi, _lib

f32 = np.float32
BAD = _abi.GS_ERR_INVALID_ARGUMENT


def test_words_round_trip_and_padding():
    rng = np.random.default_rng(1)
    for w, h in MM.SIZES:
        m = rng.random((h, w)) < 0.5
        wd = MM.words(m)
        assert wd.shape == (h, MM.row_words(w)) and MM.padding_bits(wd, w) == 0
        assert np.array_equal(MM.from_words(wd, w), m)
    wd = MM.words(np.array([[True] + [False] * 31 + [True]]))
    assert wd.tolist() == [[1, 1]]                                 # bit x & 31 of word x >> 5


def test_bow_tie_and_pentagram_have_even_odd_holes():
    w = h = 101
    bow = MM.polygon_coverage(w, h, np.array(MM.BOW_TIE, f32) * 100 + f32(0.25))
    assert bow[50, 10] and bow[50, 90] and not bow[10, 50] and not bow[90, 50]      # the side triangles are inside, the top and bottom ones outside
    star = MM.polygon_coverage(w, h, np.array(MM.PENTAGRAM, f32) * 100 + f32(0.25))
    assert not star[52, 50], "the pentagon in the middle is wound twice: a hole under the even-odd rule"
    assert star[8, 50] and star[40, 85] and star[40, 15] and star[80, 25] and star[80, 75]      # the five points
    assert 0 < star.sum() < w * h


def test_a_vertex_on_a_pixel_centre_is_decided_by_the_less_or_equal_rule():
    cov = MM.polygon_coverage(7, 7, [(1.5, 1.5), (4.5, 1.5), (4.5, 4.5), (1.5, 4.5)])
    want = np.zeros((7, 7), bool)
    want[1:4, 1:4] = True                                          # rows and columns 1 .. 3: the centres at 1.5 are in, those at 4.5 are out
    assert np.array_equal(cov, want)


def test_a_horizontal_edge_on_a_row_centre_never_crosses():
    # the outline runs along yc = 2.5 from x = 1 to x = 5, and back along y = 5.  On row 2 the top edge has both ends at yc (<=: no crossing) and the two
    # vertical edges, each with one end at yc and the other below, cross: rows 2 .. 4 between them, and nothing else
    cov = MM.polygon_coverage(8, 8, [(1.0, 2.5), (5.0, 2.5), (5.0, 5.0), (1.0, 5.0)])
    want = np.zeros((8, 8), bool)
    want[2:5, 1:5] = True
    assert np.array_equal(cov, want)
    flat = MM.polygon_coverage(8, 8, [(1.0, 2.5), (5.0, 2.5), (7.0, 2.5)])
    assert not flat.any()


def test_stroke_premises():
    one = MM.stroke_coverage(9, 7, [(4.5, 3.5)], 0.5)
    assert one.sum() == 1 and one[3, 4], "a disc of radius 0.5 on a pixel centre is that pixel"
    assert not MM.stroke_coverage(9, 7, [(-40.0, -40.0)], 7.0).any()
    line = MM.stroke_coverage(9, 7, [(1.5, 3.5), (1.5, 3.5), (6.5, 3.5)], 1.0)                  # a zero-length segment inside a polyline
    want = np.zeros((7, 9), bool)
    want[3, 0:8] = True
    want[2, 1:7] = want[4, 1:7] = True
    assert np.array_equal(line, want)
    assert MM.stroke_coverage(9, 7, [(3.0, 3.0), (4.0, 4.0)], 100.0).all()
    assert np.array_equal(MM.apply(want, line, True), np.zeros((7, 9), bool)) and np.array_equal(MM.apply(~want, line, False), np.ones((7, 9), bool))


def test_refusal_twin():
    ok = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]
    assert not MM.refused(ok, 3) and MM.refused(ok[:2], 3) and not MM.refused(ok[:1], 1, 2.0) and MM.refused(np.zeros((0, 2)), 1, 2.0)
    for bad in (np.nan, np.inf, -np.inf, 65537.0, -65536.01):
        assert MM.refused(ok[:2] + [(bad, 0.0)], 3), bad
    assert not MM.refused(ok[:2] + [(65536.0, -65536.0)], 3)
    for r in (0.0, -1.0, np.nan, np.inf, 65536.01):
        assert MM.refused(ok, 1, r), r
    assert not MM.refused(ok, 1, 65536.0)


def test_selection_twin_against_the_rectangle_twin():
    """on finite pixel positions a mask holding one pixel rectangle hits exactly what the rectangle twin hits with rect_of_mask_box's rectangle; a NaN
    position, a splat behind the camera and centres just outside each screen edge hit nothing"""
    W, H = 40, 30
    rng = np.random.default_rng(4)
    n = 4000
    clip = np.ones((n, 4), f32)
    clip[:, 0] = rng.random(n) * 2.4 - 1.2
    clip[:, 1] = rng.random(n) * 2.4 - 1.2
    clip[:, 3] = np.where(rng.random(n) < 0.2, -1.0, 1.0)
    cut = rng.random(n) < 0.1
    box = (5, 3, 33, 21)
    mask = np.zeros((H, W), bool)
    mask[box[1]:box[3] + 1, box[0]:box[2] + 1] = True
    got = MM.mask_hit_flags(clip, cut, mask)
    want = EM.hit_flags(clip, cut, W, H, MM.rect_of_mask_box(*box, H))
    assert np.array_equal(got, want) and 100 < got.sum() < n
    full = np.ones((H, W), bool)
    edge = np.ones((6, 4), f32)
    edge[:, :2] = [(-1.0 - 2.0 ** -20, 0.0), (1.0, 0.0), (0.0, -1.0 - 2.0 ** -20), (0.0, 1.0), (np.nan, 0.0), (0.0, 0.0)]
    px, py = EM.pixel_positions(edge, W, H)
    assert px[0] < 0 and px[1] == W and py[2] < 0 and py[3] == H and np.isnan(px[4])
    assert MM.mask_hit_flags(edge, np.zeros(6, bool), full).tolist() == [False, False, False, False, False, True]
    assert EM.hit_flags(edge, np.zeros(6, bool), W, H, (0, 0, W, H))[4], "the rectangle tool's quirk: a NaN pixel position is inside every rectangle"
    behind = np.array([[0.0, 0.0, 0.0, -1.0], [0.0, 0.0, 0.0, 0.0]], f32)
    assert not MM.mask_hit_flags(behind, np.zeros(2, bool), full).any()
    # y: py counts up from the bottom edge, the mask's rows down from the top
    top = np.zeros((H, W), bool)
    top[0, :] = True
    up = np.array([[0.0, 1.0 - 2.0 ** -10, 0.0, 1.0], [0.0, -1.0, 0.0, 1.0]], f32)     # py just below H; py = 0
    assert MM.mask_hit_flags(up, np.zeros(2, bool), top).tolist() == [True, False]


def test_select_surface_mask_twin_against_the_rectangle_twin():
    rng = np.random.default_rng(9)
    H, W, n = 12, 20, 300
    rec = PM.none_records(H, W)
    named = rng.random((H, W)) < 0.7
    rec["splat"][named] = rng.integers(0, n + 20, named.sum())
    rec["tag"][named] = rng.integers(6, 8, named.sum())
    deleted = EM.pack_bits(rng.random(n) < 0.2, (n + 31) // 32)
    cut = rng.random(n) < 0.2
    start = rng.integers(0, 2 ** 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    box = (3, 2, 15, 9)
    mask = np.zeros((H, W), bool)
    mask[box[1]:box[3] + 1, box[0]:box[2] + 1] = True
    for subtract in (False, True):
        got = MM.select_surface_mask(rec, start, mask, 7, n, deleted, cut, subtract)
        assert np.array_equal(got, PM.select_surface(rec, start, box, 7, n, deleted, cut, subtract))
        assert not np.array_equal(got, start)
    assert np.array_equal(MM.select_surface_mask(rec, start, np.zeros((H, W), bool), 7, n), start)


def test_entry_points_refuse_null_without_a_device():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.gs_mask_create(None, 16, 16, C.byref(h)) == BAD and not h
    assert lib.gs_mask_destroy(None) == 0
    assert lib.gs_mask_clear(None) == BAD
    assert lib.gs_mask_upload(None, None, 0) == BAD and lib.gs_mask_download(None, None, 0) == BAD
    assert lib.gs_mask_fill_polygon(None, None, 3, 0) == BAD
    assert lib.gs_mask_stroke(None, None, 1, C.c_float(1.0), 0) == BAD
    assert lib.gs_renderer_edit_update_selection_mask(None, None, None, 0) == BAD
    assert lib.gs_renderer_edit_select_surface_mask(None, None, None, 0) == BAD
