"""-m gpu: the compositor's edges on the crafted scenes of tests/crafted.py (tests/test_crafted_scenes.py shows on the CPU that each scene is what it is taken
for here, and that the records a case is about cannot be dropped or doubled within the tolerance).  Every case goes through GaussianSplatRenderer in
SortMode.Full and SortMode.Visible (bin_emit / vis_count + vis_offsets + vis_emit) and is held to the oracle as tests/test_gpu_random_parity.py holds its cases:

    order buffer, 40-byte SplatViewData      bit-exact
    (tile, splat) pairs, visible count       equal
    RGBA16F target                           <= 2^-9 relative to max(1, |c|), EVERY pixel (rt_err, no rare allowance); blend mode 1 <= 4e-3
    the same case at several tile shapes     downloads bit-identical to each other (and between the two sort modes)

  grids              every class of the pair sort's dispatch, on both sides of its boundary, pinned 16x16: 64/65, 128/129, 256/257 (one pass: 6, 7, 8 bits),
                     2,048/2,049 (per-tile counters), 4,096/4,097, 16,384/16,385, 65,536 (two passes: 6, 7, 8 bits) and 65,538, 131,072 tiles (three
                     passes; 65,537 is prime, no target has it); 65,535 x 8 and 8 x 65,535 (the 16-bit rectangle fields); each asserts the pass count the
                     draw took (gs_stage_times.onesweep_pair_launches) and the tile shape it reports, and draws a second time (the tile schedule then comes
                     from the extra workgroup of the emission kernel instead of tile_order_kernel): the same bits
  list lengths       per tile shape: lists of 1, 63, 64, 65, NT-1, NT, NT+1, 2NT-1, 2NT, 2NT+1, 3NT+1 one-fragment records (NT = the blend's staging batch)
  early termination  per tile shape: quadrants saturated by the first batch, the late quadrant's only splats in the third; an interior tile and the
                     bottom-right partial tile (a column of quadrants wholly outside the target); onto a cleared target, then once more without clearing;
                     both blend modes
  heavy tail         40 screen-covering splats among 20,000 small ones and 300 needles (60 centred off screen)
  values             opacity 1.0, the fp16 neighbours of 1/255, colours 0 and 300 .. 1000"""
import numpy as np
import pytest

import crafted as K
from common import RT_TOL, rt_err, views_equal
from unitygaussiansplatting_amd._lib import GsError
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget, SortMode

pytestmark = pytest.mark.gpu

MODES = (SortMode.Full, SortMode.Visible)
TOL = {0: RT_TOL, 1: 4e-3}               # exact mode, fast mode


def _err(img, ref):
    """rt_err(img, ref), a band of rows at a time (a 4,096 x 8,192 target is 134 M channel values: the float32 temporaries of one call would be 2 GB)."""
    step = max(1, (1 << 22) // img.shape[1])
    return max(rt_err(img[y:y + step], ref[y:y + step]) for y in range(0, img.shape[0], step))


_last_reference = {}


def _reference(sc, blend):
    """The oracle's side of a case, kept for the case's other sort mode and tile shapes (one at a time: the largest frame is 268 MB)."""
    key = (sc.name, blend)
    if key not in _last_reference:
        _last_reference.clear()
        _last_reference[key] = K.oracle_frame(sc, blend=blend)
    return _last_reference[key]


def _stats(r, cam, rt, clear):
    try:
        return r.FrameStats()
    except GsError as ex:                                       # the documented protocol (gsplat_c.h: GS_ERR_PAIR_OVERFLOW): the pair buffer has been grown,
        assert ex.code == -6 and clear, ex                      # the host draws the frame again
        rt.Clear(); r.Draw(cam, rt)
        return r.FrameStats()


def _run(gpu_ctx, sc, mode, tile, blend=0, accumulate=False, redraw=False, passes=None):
    """One case in one sort mode at one pinned tile shape against the oracle; returns the downloads (cleared draw[, the accumulating second draw])."""
    what = f"{sc.name} {mode.name} tile {tile} blend {blend}"
    orc, P, ref = _reference(sc, blend)
    r = GaussianSplatRenderer(gpu_ctx, sc.asset)
    r.sortMode = mode
    r.OnEnable()
    r.SetTileShape(*tile)
    r.blendMode = blend
    if passes is not None:
        r.SetProfiling(4)                                       # gs_renderer_stage_times needs a profiling ring
    cam = sc.cam
    rt = RenderTarget(gpu_ctx, sc.W, sc.H)
    out = []
    try:
        r.SortPoints(cam); r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
        st = _stats(r, cam, rt, True)
        assert views_equal(r.DownloadView(), orc.view), f"{what}: view records differ"
        pairs = orc.pairs(r.FrameParams(cam), st)
        assert (st.tile_w, st.tile_h) == tuple(tile) and st.sort_error == 0, f"{what}: drawn with {st.tile_w}x{st.tile_h}, sort error {st.sort_error}"
        assert st.visible_splats == orc.visible, f"{what}: visible {st.visible_splats} vs {orc.visible}"
        assert st.tile_pairs == pairs, f"{what}: pairs {st.tile_pairs} vs {pairs}"
        if passes is not None:
            got = r.StageTimes().onesweep_pair_launches
            assert got == passes, f"{what}: {st.tiles_x} x {st.tiles_y} tiles sorted in {got} passes, not {passes}"
        img = rt.Download()
        e = _err(img, ref)
        print(f"{what}: P={pairs} visible={orc.visible} err={e:.3e}")
        assert e <= TOL[blend], f"{what}: target off by {e}"
        out.append(img)
        if redraw:                                              # the same frame again: this time the draw has the previous one's tile costs
            rt.Clear(); r.Draw(cam, rt)
            assert _stats(r, cam, rt, True).tile_pairs == pairs
            assert np.array_equal(rt.Download(), img), f"{what}: the second draw of the same frame differs from the first"
        if accumulate:                                          # once more WITHOUT clearing: the blend starts from the frame it has just made
            ref2 = orc.draw(P, blend, rt=ref.copy())
            r.Draw(cam, rt)
            assert _stats(r, cam, rt, False).tile_pairs == pairs
            img2 = rt.Download()
            e2 = _err(img2, ref2)
            print(f"{what}: accumulated err={e2:.3e}")
            assert e2 <= TOL[blend], f"{what}: accumulating draw off by {e2}"
            assert not np.array_equal(img2, img)
            out.append(img2)
        assert np.array_equal(r.DownloadOrder(), orc.order), f"{what}: order differs"
    finally:
        r.OnDisable()
        rt.Dispose()
    return out


def _same(frames, what):
    for k, f in enumerate(frames[1:]):
        for a, b in zip(frames[0], f):
            assert np.array_equal(a, b), f"{what}: variant {k + 1} is not bit-identical to variant 0"


@pytest.mark.parametrize("num_tiles", sorted(K.GRID_CLASSES))
def test_grid_classes_of_the_pair_sort(gpu_ctx, num_tiles):
    W, H = K.grid_size(*K.GRID_CLASSES[num_tiles])
    sc = K.grid_scene(W, H, K.grid_splats(num_tiles))
    frames = [_run(gpu_ctx, sc, mode, (16, 16), redraw=True, passes=K.pair_sort_passes(num_tiles)) for mode in MODES]
    _same(frames, sc.name)


@pytest.mark.parametrize("W,H", [(65535, 8), (8, 65535)])
def test_targets_of_65535_pixels(gpu_ctx, W, H):
    sc = K.grid_scene(W, H)
    frames = [_run(gpu_ctx, sc, mode, (16, 16), redraw=True, passes=2) for mode in MODES]            # 4,096 tiles
    frames += [_run(gpu_ctx, sc, SortMode.Visible, (32, 32), passes=2)]                               # 2,048
    _same(frames, sc.name)


@pytest.mark.parametrize("tile", K.TILE_SHAPES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_list_lengths_around_the_staging_batch(gpu_ctx, tile):
    sc = K.list_length_scene(tile)
    frames = [_run(gpu_ctx, sc, mode, tile) for mode in MODES]
    frames += [_run(gpu_ctx, sc, SortMode.Full, other) for other in K.TILE_SHAPES if other != tile]
    _same(frames, sc.name)


@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("tile", K.TILE_SHAPES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_early_termination_with_a_late_quadrant(gpu_ctx, tile, blend):
    sc = K.early_termination_scene(tile)
    frames = [_run(gpu_ctx, sc, mode, tile, blend=blend, accumulate=True) for mode in MODES]
    frames += [_run(gpu_ctx, sc, SortMode.Visible, other, blend=blend, accumulate=True) for other in K.TILE_SHAPES if other != tile]
    _same(frames, sc.name)                                      # (both blend modes: a pixel's early stop depends on neither the tile nor the sort mode)


def test_heavy_tailed_emission(gpu_ctx):
    sc = K.heavy_tail_scene()
    frames = [_run(gpu_ctx, sc, mode, tile, redraw=(tile == (16, 16))) for tile in K.TILE_SHAPES for mode in MODES]
    _same(frames, sc.name)


def test_extreme_values(gpu_ctx):
    sc = K.values_scene()
    frames = [_run(gpu_ctx, sc, mode, tile) for tile in K.TILE_SHAPES for mode in MODES]
    _same(frames, sc.name)
