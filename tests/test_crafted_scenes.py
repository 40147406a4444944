"""CPU only: every scene of tests/crafted.py IS what tests/test_gpu_compositor_edges.py takes it for, stated on the oracle alone.

  premise         the designed list lengths occur exactly, in the designed tiles; the boundary grids have pairs in tile 0 and in the last tile id; the
                  early quadrants reach A == 1.0 (fp16 0x3c00) within the first staging batch while the late quadrant is still 0; the screen-covering
                  splats are on every tile's list, the needles on hundreds
  observability   every record a case is about -- the first and the last of each staging batch, the last of the list, the late quadrant's splats, the grids' corner
                  splats, the screen-covering layers, off-screen needles whose band reaches in -- is
                  visible on its own: the frame with that ONE splat deleted (the oracle's deleted bits) differs from the full frame, in some pixel, by at
                  least 8 x RT_TOL in rt_diff's metric.  A compositor that drops or doubles such a record therefore cannot stay within RT_TOL."""
import numpy as np
import pytest

import crafted as K
from common import RT_TOL, rt_diff

OBSERVABLE = 8.0 * RT_TOL
A_ONE = 0x3c00


def _alpha(frame):
    return frame[..., 3]


@pytest.mark.parametrize("tile", K.TILE_SHAPES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_list_length_scene_has_the_designed_lists_and_every_batch_edge_is_visible(tile):
    sc = K.list_length_scene(tile)
    nt = tile[0] * tile[1]
    orc, P, rects, lengths, per_splat = K.checked_tile_lists(sc, tile)
    want = np.zeros_like(lengths)
    for (tx, ty), L in sc.meta["designed"].items():
        want[ty, tx] = L
    assert sorted(sc.meta["designed"].values()) == sorted(K.list_lengths_for(tile))
    assert np.array_equal(lengths, want), "a designed list has another length, or a tile between them is touched"
    assert (per_splat == 1).all() and orc.visible == sc.asset.splatCount            # every dot is drawn, on one tile
    full = orc.draw(P, 0)
    assert _alpha(full).view(np.float16).max() < 0.03                                # nothing near saturation: every record of every list is walked
    about = []
    for (tx, ty), L in sc.meta["designed"].items():
        lst = K.tile_list(rects, orc.order, tile, tx, ty)
        assert len(lst) == L
        edges = sorted({p for k in range(0, L, nt) for p in (k, min(k + nt, L) - 1)} | {L - 1})      # first and last record of each batch, the last of the list
        about += [int(lst[p]) for p in edges]
    seen = K.observable(sc, about, full)
    assert (seen >= OBSERVABLE).all(), f"records that could be dropped within the tolerance: {[(s, v) for s, v in zip(about, seen) if v < OBSERVABLE]}"


@pytest.mark.parametrize("tile", K.TILE_SHAPES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_early_termination_scene_saturates_the_early_quadrants_in_batch_one_and_the_late_one_comes_in_batch_three(tile):
    sc = K.early_termination_scene(tile)
    tw, th = tile
    nt = tw * th
    assert sc.W % 8 and sc.H % 8
    orc, P, rects, lengths, _ = K.checked_tile_lists(sc, tile)
    full = orc.draw(P, 0)
    for which, d in sc.meta["tiles"].items():
        tx, ty = d["tile"]
        x0, y0 = tx * tw, ty * th
        lst = K.tile_list(rects, orc.order, tile, tx, ty)
        assert len(lst) == lengths[ty, tx] == 2 * nt + 5 + 3, (which, len(lst))
        assert np.array_equal(np.sort(lst[:len(d["squares"])]), d["squares"]) and np.array_equal(lst[-3:], d["lates"])
        assert (np.searchsorted(np.arange(0, 4 * nt, nt), [len(lst) - 3], side="right") - 1)[0] == d["batch"] == 2      # the late splats: third batch
        if which == "edge":
            assert (tx + 1) * tw - sc.W == 11 and (ty + 1) * th - sc.H == 3 and tx == lengths.shape[1] - 1 and ty == lengths.shape[0] - 1
        # after the first batch (the frame of the list's first NT records alone): early quadrants at A == 1.0 on every inside pixel, the late quadrant 0
        first = K.oracle_frame(sc, deleted=np.setdiff1d(np.arange(sc.asset.splatCount), lst[:nt]))[2]
        for qx, qy in d["early"]:
            a = first[y0 + 8 * qy:min(y0 + 8 * qy + 8, sc.H), x0 + 8 * qx:min(x0 + 8 * qx + 8, sc.W), 3]
            assert a.size and (a == A_ONE).all(), (which, qx, qy)
        lx, ly = x0 + 8 * d["late"][0], y0 + 8 * d["late"][1]
        assert not first[ly:ly + 8, lx:lx + 8].any(), which
        # ... and in the whole frame the late quadrant holds something, but is not saturated (an accumulating second draw still changes it)
        late = full[ly:min(ly + 8, sc.H), lx:min(lx + 8, sc.W)]
        assert late.any() and (late[..., 3] != A_ONE).any()
        seen = K.observable(sc, list(d["lates"]) + list(d["squares"]), full)
        assert (seen >= OBSERVABLE).all(), (which, seen)
    # an accumulating draw onto the finished frame differs from it (where A < 1), and only there
    twice = K.oracle_frame(sc, rt=full.copy())[2]
    changed = (twice != full).any(axis=-1)
    assert changed.any() and not changed[_alpha(full) == A_ONE].any()


@pytest.mark.parametrize("num_tiles", sorted(K.GRID_CLASSES))
def test_grid_scenes_have_the_tile_count_of_their_class_and_pairs_in_the_first_and_the_last_tile(num_tiles):
    tile = (16, 16)
    tiles_x, tiles_y = K.GRID_CLASSES[num_tiles]
    W, H = K.grid_size(tiles_x, tiles_y)
    assert -(-W // 16) == tiles_x and -(-H // 16) == tiles_y and tiles_x * tiles_y == num_tiles and W <= 65535 and H <= 65535
    sc = K.grid_scene(W, H, K.grid_splats(num_tiles))
    orc, P, rects, lengths, per_splat = K.checked_tile_lists(sc, tile)
    assert lengths.shape == (tiles_y, tiles_x) and lengths[0, 0] > 0 and lengths[-1, -1] > 0
    assert (per_splat[sc.meta["corners"]] > 0).all() and (per_splat > 1).sum() >= 50          # (splats over several tiles, too)
    if num_tiles > 65536:
        # tile ids that need more than 16 bits have pairs
        ty = np.repeat(np.arange(tiles_y), tiles_x).reshape(tiles_y, tiles_x)
        ids = ty * tiles_x + np.arange(tiles_x)[None, :]
        high = int(lengths[ids >= 65536].sum())
        assert high > 0
        if num_tiles == 131072:
            assert 4 * high >= int(lengths.sum()), "the three-pass scene: at least a quarter of the pairs beyond tile id 65,535"
    # the corner splats -- the records behind "pairs in tile 0 and in the last tile id" -- are visible on their own (a window of 24 pixels around each corner)
    for s, (cx, cy) in zip(sc.meta["corners"], ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1))):
        win = (max(cx - 23, 0), max(cy - 23, 0), min(cx + 23, W - 1), min(cy + 23, H - 1))
        seen = K.observable(sc, [s], window=win)
        assert (seen >= OBSERVABLE).all(), (s, win, seen)


@pytest.mark.parametrize("W,H", [(65535, 8), (8, 65535)])
def test_extreme_targets_have_rectangles_whose_16_bit_far_corner_is_65535(W, H):
    sc = K.grid_scene(W, H)
    orc, P, rects, lengths, per_splat = K.checked_tile_lists(sc, (16, 16))
    far = (rects[:, 1] & 0xffff) if W == 65535 else (rects[:, 1] >> 16)
    assert far.max() == 65535 and lengths[-1, -1] > 0 and lengths[0, 0] > 0
    assert (K.observable(sc, sc.meta["corners"]) >= OBSERVABLE).all()
    assert np.count_nonzero(per_splat) >= 0.9 * sc.asset.splatCount


def test_heavy_tail_scene_has_screen_covering_splats_needles_and_small_ones():
    sc = K.heavy_tail_scene()
    m = sc.meta
    for tile in K.TILE_SHAPES:
        orc, P, rects, lengths, per_splat = K.checked_tile_lists(sc, tile)
        assert (per_splat[m["full"]] == lengths.size).all(), "a screen-covering splat is on every tile's list"
        assert lengths.min() >= len(m["full"])
        assert np.median(per_splat[m["small"]]) == 1 and per_splat[m["small"]].max() <= 9
        assert np.median(per_splat[m["needle"]]) >= 3200 // (tile[0] * tile[1] // 16), np.median(per_splat[m["needle"]])
        assert np.count_nonzero(per_splat[m["offscreen"]]) >= 40, "needles centred off screen reach in"
        assert per_splat.sum() > 4 * per_splat[m["small"]].sum()                     # the few huge ones are most of the pairs
    # the emitters of the tail are individually visible: every screen-covering layer, off-screen needles
    orc, P, full = K.oracle_frame(sc)
    assert float(_alpha(full).view(np.float16).max()) <= 1.0
    seen = K.observable(sc, [int(v) for v in m["full"]], full)
    assert (seen >= OBSERVABLE).all(), seen
    # (a needle's rectangle may overlap the target while its two-pixel band misses it: those whose long axis passes at least 4 pixels inside the target
    # within one axis length of the centre -- geometry of the raster records alone -- are visible on their own, every one of the first twelve)
    recs = orc.raster_records(P)[0]
    reaching = K.needles_reaching_in(sc, recs, m["offscreen"])
    assert len(reaching) >= 30, len(reaching)
    seen = K.observable(sc, reaching[:12], full)
    assert (seen >= OBSERVABLE).all(), seen


def test_values_scene_holds_the_values_it_names():
    sc = K.values_scene()
    m = sc.meta
    orc, P, rects, lengths, per_splat = K.checked_tile_lists(sc, (16, 16))
    assert m["lo"] < 1.0 / 255.0 < m["hi"] and np.float16(m["lo"]) == np.float32(m["lo"]) and np.nextafter(np.float16(m["lo"]), np.float16(1)) == np.float16(m["hi"])
    opac = orc.view["color"][:, 1] & 0xffff                                          # f16 opacity of the 40-byte record
    assert (opac[m["below"]] == np.float16(m["lo"]).view(np.uint16)).all() and (opac[m["above"]] == np.float16(m["hi"]).view(np.uint16)).all()
    assert (opac[np.concatenate([m["black"], m["under"], m["bright"]])] == A_ONE).all()
    assert (per_splat[m["below"]] == 0).all(), "opacity below 1/255: never drawn"
    assert (per_splat[m["above"]] == 1).all(), "opacity just above 1/255: drawn"
    full = orc.draw(P, 0)
    f = full.view(np.float16).astype(np.float32)
    assert np.isfinite(f).all() and f[..., :3].max() > 100.0 and (f[..., 3] == 1.0).any()
    about = np.concatenate([m[k] for k in ("above", "black", "under", "veil", "bright")])
    seen = K.observable(sc, about, full)
    assert (seen >= OBSERVABLE).all(), seen
    # one live fragment each for the splats barely above the threshold: deleting one changes exactly one pixel
    one = K.oracle_frame(sc, deleted=[int(m["above"][0])])[2]
    assert np.count_nonzero((rt_diff(one, full) > 0).any(axis=-1)) == 1
