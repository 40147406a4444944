"""-m gpu: frames in flight drawing into a target whose memory the host was given -- its device pointers handed out (gs_target_device_ptr) or a depth
buffer lent by the host (gs_target_set_scene_depth, memory_kind 1).  A lane's blend then waits for everything the context's stream holds, not only for
the target's last use (enqueue_draw, gs_raster.hip), and the context's stream waits for the blend.  Every frame's pixels and visible order equal, bit
for bit, those of a fresh one-at-a-time renderer drawing into an ordinary target."""
import ctypes as C

import numpy as np
import pytest

from common import default_camera, small_asset
from unitygaussiansplatting_amd import _lib
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
W, H = 320, 200
# four cameras: each of the two lanes draws twice
CAMS = [default_camera(az=25.0), default_camera(az=110.0, elev=-20.0), default_camera(az=250.0, elev=35.0, radius=7.0), default_camera(az=300.0, elev=5.0)]
# the cameras orbit the scene's centre at 6 to 7 units: a wall at view depth 6 hides the splats behind the centre and leaves those in front of it
WALL = 6.0
_reference = {}


def visible_renderer(ctx, frames):
    r = GaussianSplatRenderer(ctx, small_asset(300, 5, "VeryHigh"))
    r.sortMode = SortMode.Visible
    r.OnEnable()
    if frames > 1:
        r.SetFramesInFlight(frames)
        assert r.FramesInFlight() == (frames, True)
    return r


def draw_frames(r, rt):
    """SortPoints / CalcViewData / clear / Draw of every camera into rt: [(pixels, visible order)]"""
    out = []
    for cam in CAMS:
        r.SortPoints(cam); r.CalcViewData(cam); rt.Clear(); r.Draw(cam, rt)
        out.append((rt.Download(), r.DownloadVisibleOrder()))
    return out


def reference_frames(ctx, wall):
    """the frames of a fresh one-at-a-time renderer into an ordinary target (wall: the constant scene depth, given from the host, or None); drawn once"""
    if wall not in _reference:
        r = visible_renderer(ctx, 1)
        rt = RenderTarget(ctx, W, H)
        if wall is not None:
            rt.SetSceneDepth(np.full((H, W), wall, np.float32))
        _reference[wall] = draw_frames(r, rt)
        for px, order in _reference[wall]:
            px.setflags(write=False); order.setflags(write=False)
        r.OnDisable(); rt.Dispose()
    return _reference[wall]


def assert_same_frames(got, want, what):
    assert len(got) == len(want) == len(CAMS)
    for k, ((gp, go), (wp, wo)) in enumerate(zip(got, want)):
        assert np.array_equal(go, wo), (what, k, "visible order")
        assert np.array_equal(gp, wp), (what, k, "pixels", int((gp != wp).sum()))


def test_lanes_draw_into_an_exposed_target(gpu_ctx):
    want = reference_frames(gpu_ctx, None)
    assert any(px.any() for px, _ in want)                         # premise: something is drawn
    r = visible_renderer(gpu_ctx, 2)
    rt = RenderTarget(gpu_ctx, W, H)
    px, res = C.c_void_p(), C.c_void_p()
    _lib.check(_lib.lib().gs_target_device_ptr(rt._h, C.byref(px), C.byref(res)), "gs_target_device_ptr")
    assert px.value
    got = draw_frames(r, rt)
    assert_same_frames(got, want, "exposed")
    again = C.c_void_p()
    _lib.check(_lib.lib().gs_target_device_ptr(rt._h, C.byref(again), None), "gs_target_device_ptr")
    assert again.value == px.value                                 # the pointer the host holds stays the target's
    r.OnDisable(); rt.Dispose()


def test_lanes_draw_against_a_borrowed_depth_buffer(gpu_ctx):
    want = reference_frames(gpu_ctx, WALL)
    plain = reference_frames(gpu_ctx, None)
    assert any(px.any() for px, _ in want)                         # premise: some splats are in front of the wall ...
    assert any(not np.array_equal(w[0], p[0]) for w, p in zip(want, plain))   # ... and some behind it
    hip = C.CDLL("libamdhip64.so")                                 # (the runtime the library itself is linked against)
    host = np.full((H, W), WALL, np.float32)
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(host.nbytes)) == 0
    try:
        assert hip.hipMemcpy(dev, C.c_void_p(host.ctypes.data), C.c_size_t(host.nbytes), 1) == 0      # hipMemcpyHostToDevice; blocks
        r = visible_renderer(gpu_ctx, 2)
        rt = RenderTarget(gpu_ctx, W, H)
        _lib.check(_lib.lib().gs_target_set_scene_depth(rt._h, dev, 1), "gs_target_set_scene_depth")
        got = draw_frames(r, rt)
        assert_same_frames(got, want, "borrowed depth")
        r.OnDisable(); rt.Dispose()                                # (both wait for their streams: nothing reads the buffer any more)
    finally:
        hip.hipFree(dev)
