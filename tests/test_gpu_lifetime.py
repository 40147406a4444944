"""Lifetime of everything the host layer owns on the GPU: five times over, make a context, an asset, a renderer and a target, render a frame, touch every
buffer and event that is made lazily or regrown (csrc/gs_handles.h owns them; gs_common.h says who holds what), set everything back, render the frame
again and destroy the lot.  Every call must succeed and the frame must be the same bytes every time.  The ownership rules themselves are proved on the
CPU (tests/test_handles.py); this is the check that the library built on them still creates, regrows and releases in an order the GPU agrees with."""

import numpy as np
import pytest

from common import default_camera, small_asset
from unitygaussiansplatting_amd import _lib
from unitygaussiansplatting_amd.camera import Transform
from unitygaussiansplatting_amd.cutout import GaussianCutout, Type
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext, GpuSorting, RenderMode, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
W, H = 96, 64                   # 24 tiles of 16x16
N = 5000                        # > two 2,048-position bin partitions, > one 256-splat chunk
CYCLES = 5


def draw(r, rt, cam):
    r.SortPoints(cam)
    r.CalcViewData(cam)
    rt.Clear()
    r.Draw(cam, rt)


def frame(r, rt, cam) -> bytes:
    draw(r, rt, cam)
    r.FrameStats()              # (raises on a sort time-out or a pair overflow)
    return rt.Download().tobytes()


def one_cycle(asset, cam):
    lib = _lib.lib()
    ctx = GpuContext(0)
    r = GaussianSplatRenderer(ctx, asset)
    r.sortMode, r.framesInFlight = SortMode.Full, 1                 # whatever the environment asks the host layer to default to
    r.CreateResourcesForAsset()
    rt = RenderTarget(ctx, W, H)
    first = frame(r, rt, cam)

    # the visible-only sort's buffers; then two lanes: their contexts, renderers and events, the target's second pixel buffer and last-use events
    r.SetSortMode(SortMode.Visible)
    draw(r, rt, cam)
    r.SetFramesInFlight(2)
    assert r.FramesInFlight() == (2, True)
    draw(r, rt, cam)
    draw(r, rt, cam)
    ctx.Synchronize()
    # cutouts set, changed, cleared (device buffer, pinned shadow, copy event; the lanes' too)
    r.m_Cutouts = [GaussianCutout(Type.Box, False, Transform(position=(0.5, 0.0, 0.0)))]
    draw(r, rt, cam)
    r.m_Cutouts = [GaussianCutout(Type.Ellipsoid, True, Transform(scale=(2.0, 1.0, 1.0))), None]
    draw(r, rt, cam)
    r.m_Cutouts = None
    draw(r, rt, cam)
    # deleted bits set, cleared, set again
    bits = np.zeros((N + 31) // 32, np.uint32)
    bits[::3] = 0x0F0F0F0F
    r.SetDeletedBits(bits)
    draw(r, rt, cam)
    r.SetDeletedBits(None)
    r.SetDeletedBits(bits)
    draw(r, rt, cam)
    # edit: select all, delete (with lanes: the delete events and the lanes' copies), info, release; select all again re-makes the buffers
    r.EditSelectAll()
    r.EditDeleteSelected()                                          # (ends with gs_renderer_edit_info)
    assert r.editDeletedSplats > 0
    _lib.check(lib.gs_renderer_edit_release(r._r_h), "gs_renderer_edit_release")
    r.EditSelectAll()
    r.SetDeletedBits(bits)                                          # (the delete removed everything: draw something again)
    draw(r, rt, cam)
    # the renderer's profiling ring, regrown; the target's
    r.SetProfiling(2)
    draw(r, rt, cam)
    r.SetProfiling(4)
    draw(r, rt, cam)
    draw(r, rt, cam)
    r.StageTimes()
    r.SetProfiling(0)
    rt.SetProfiling(True)
    rt.Resolve((0.0, 0.0, 0.0, 1.0), want8=False)
    rt.ResolveTime()
    rt.SetProfiling(False)
    # the pair buffers and their sort state, regrown
    _, cap = r.PollPairs()
    r.ReservePairs(cap + 1)
    assert r.PollPairs()[1] == cap + 1
    draw(r, rt, cam)
    # a host scene depth (the target's copy, the per-splat depths)
    rt.SetSceneDepth(np.full((H, W), 6.0, np.float32))
    draw(r, rt, cam)
    # the debug modes: depth buffer of the points, box records, chunk order
    for mode in (RenderMode.DebugPoints, RenderMode.DebugPointIndices, RenderMode.DebugBoxes, RenderMode.DebugChunkBounds):
        r.m_RenderMode = mode
        draw(r, rt, cam)
    r.m_RenderMode = RenderMode.Splats
    o32, o8 = rt.Resolve((0.0, 0.0, 0.0, 1.0), want8=True)
    assert o8 is not None and o8.shape == (H, W, 4)
    # a stand-alone sorter through its host round trip (its temporary device buffers)
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    s = GpuSorting(ctx, 1000)
    k, v = s.DispatchHost(keys, np.arange(1000, dtype=np.uint32))
    assert np.array_equal(k, np.sort(keys)) and np.array_equal(keys[v], k)

    # everything back, the first frame again
    r.SetSortMode(SortMode.Full)
    r.SetFramesInFlight(1)
    r.SetDeletedBits(None)
    rt.SetSceneDepth(None)
    again = frame(r, rt, cam)
    s.Dispose()
    rt.Dispose()
    r.Dispose()
    ctx.Dispose()
    return first, again


def test_create_touch_everything_destroy_five_times():
    asset = small_asset(N, 7, "Medium")
    assert asset.chunkData is not None                              # (DebugChunkBounds draws something)
    cam = default_camera(W=W, H=H)
    frames = [one_cycle(asset, cam) for _ in range(CYCLES)]
    assert np.frombuffer(frames[0][0], np.uint16).any(), "the frame is empty"
    for c, (first, again) in enumerate(frames):
        assert again == first, f"cycle {c}: the frame after the tour differs from the frame before it"
        assert first == frames[0][0], f"cycle {c}: the first frame differs from cycle 0's"
