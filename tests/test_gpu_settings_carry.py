"""What a host set on a renderer stays set: through SetFramesInFlight (the lanes draw with the owner's settings, whether they were made before or after the
lanes) and through EditSetSplatCount (the resize builds a new renderer state and the lanes again).  The frames of a renderer with lanes are compared bit
for bit with those of a fresh one-at-a-time renderer that was given the same settings; new lanes draw with their owner's deleted bits."""
import numpy as np
import pytest

import edit_model as EM
from common import default_camera, small_asset
from builders import DST_TR
from gpu_rig import download, draw_frame, pinned_renderer as make_renderer
from unitygaussiansplatting_amd.renderer import RenderTarget, SortMode

pytestmark = pytest.mark.gpu
W, H = 320, 200
CAMS = [default_camera(az=25.0), default_camera(az=110.0, elev=-20.0), default_camera(az=250.0, elev=35.0, radius=7.0), default_camera(az=300.0, elev=5.0)]


def apply_settings(r, history=None, view_every_frame=False):
    r.blendMode = 1                                                # Draw hands it to gs_renderer_set_blend_mode
    r.SetTileShape(16, 16)
    if view_every_frame:
        r.SetViewBufferMode(True)
    if history is not None:
        r.SetSortHistoryLimit(history)


def frame(r, ctx, cam):
    """one SortPoints / CalcViewData / Draw: (view records, pixels, visible order)"""
    rt = RenderTarget(ctx, cam.pixelWidth, cam.pixelHeight)
    draw_frame(r, cam, rt)
    out = (r.DownloadView(), rt.Download(), r.DownloadVisibleOrder(), r.FrameStats())
    rt.Dispose()
    return out


def assert_same_frame(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, "view")
    assert np.array_equal(got[1], want[1]), (what, "frame", int((got[1] != want[1]).sum()))
    assert np.array_equal(got[2], want[2]), (what, "visible order")
    assert (got[3].tile_w, got[3].tile_h) == (want[3].tile_w, want[3].tile_h) == (16, 16), (what, "tile shape of the draw")


def test_settings_survive_lanes_and_a_resize(gpu_ctx):
    """blend mode 1, 16x16 tiles, the view buffer written every frame and a history of 3, THEN two lanes, THEN a shrink to 130 splats (a partial last word)"""
    r = make_renderer(gpu_ctx, small_asset(300, 5, "VeryHigh"), DST_TR, SortMode.Visible)
    apply_settings(r, history=3, view_every_frame=True)
    r.SetFramesInFlight(2)
    r.EditSetSplatCount(130)
    assert r.TileShape(W, H) == (16, 16)
    assert r.SortHistory()[1] == 3
    assert r.FramesInFlight() == (2, True)
    got = download(r)
    fresh = make_renderer(gpu_ctx, got.asset(), DST_TR, SortMode.Visible)
    fresh.SetDeletedBits(got.deleted)
    apply_settings(fresh, history=3, view_every_frame=True)
    assert fresh.FramesInFlight() == (1, False)
    for k, cam in enumerate(CAMS[:2]):
        mine, theirs = frame(r, gpu_ctx, cam), frame(fresh, gpu_ctx, cam)
        assert_same_frame(mine, theirs, ("resized", k))
        assert mine[1].any() and len(mine[2]) > 0
    assert r.SortHistory()[1] == 3 and r.TileShape(W, H) == (16, 16)
    fresh.DisposeResourcesForAsset(); r.DisposeResourcesForAsset()


def test_settings_made_after_the_lanes_reach_them(gpu_ctx):
    """33 of 300 splats deleted, two lanes, THEN blend mode and tile shape: four consecutive frames visit both lanes twice"""
    asset = small_asset(300, 5, "VeryHigh")
    flags = np.zeros(300, bool)
    edges = [0, 31, 32, 299]                                       # both sides of a word boundary, and the last splat (the last word is partial)
    flags[edges] = True
    flags[np.random.default_rng(33).permutation(np.setdiff1d(np.arange(300), edges))[:29]] = True
    assert int(flags.sum()) == 33
    words = EM.pack_bits(flags, (300 + 31) // 32)
    r = make_renderer(gpu_ctx, asset, DST_TR, SortMode.Visible)
    r.SetDeletedBits(words)
    r.SetFramesInFlight(2)
    assert r.FramesInFlight() == (2, True)
    apply_settings(r)
    one = make_renderer(gpu_ctx, asset, DST_TR, SortMode.Visible)
    one.SetDeletedBits(words)
    apply_settings(one)
    whole = make_renderer(gpu_ctx, asset, DST_TR, SortMode.Visible)          # nothing deleted: what the frames must NOT be
    apply_settings(whole)
    deleted = np.flatnonzero(flags)
    seen_deleted_elsewhere = False
    for k, cam in enumerate(CAMS):
        mine, theirs, full = frame(r, gpu_ctx, cam), frame(one, gpu_ctx, cam), frame(whole, gpu_ctx, cam)
        assert_same_frame(mine, theirs, ("lanes first", k))
        assert mine[1].any() and len(mine[2]) > 0
        assert not np.isin(mine[2], deleted).any(), ("a deleted splat was drawn", k)
        seen_deleted_elsewhere |= bool(np.isin(full[2], deleted).any())
        assert np.array_equal(mine[2], full[2][~np.isin(full[2], deleted)]), ("the drawn splats are the undeleted ones, in the same order", k)
    assert seen_deleted_elsewhere                                  # premise: without the bits some of the 33 are visible
    assert r.TileShape(W, H) == (16, 16)
    for x in (whole, one, r):
        x.DisposeResourcesForAsset()
