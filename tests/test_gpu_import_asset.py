"""The import on the GPU (csrc/gs_bake.hip through gs_import_encode_to_asset and creator.CreateGpuAssetFromSplats) against the native host importer:
after every import the five blobs of GpuAsset.Download() over gs_import_blob_sizes bytes each, byte for byte, and the bounds, bit for bit, against
creator.CreateAssetFromSplatsNative of the same input -- every preset, BC7 colour and the Cluster* palettes included, linearize and morton on and off.
The premises (finite input, no -0 among the extremes) are asserted on every input.  The coplanar case builds its yardstick the way
tests/test_gpu_bake.py's does: the input ordered by the model's key with the degenerate component forced to 0, imported with morton = 0."""
import ctypes as C
import functools

import numpy as np
import pytest

import bake_model as BM
from common import same_bits, small_asset
from gpu_rig import BAD, frame_of, pinned_renderer as make_renderer, same_frame
from unitygaussiansplatting_amd import _abi, _lib, asset as A, creator, scenes
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

pytestmark = pytest.mark.gpu
f32 = np.float32
VF, CF, SF = A.VectorFormat, A.ColorFormat, A.SHFormat
MEDIUM = dict(quality="Medium")
BC7 = dict(quality="Medium", formatColor=CF.BC7)                   # Medium with BC7 colour (formatSH = Norm6)


@functools.lru_cache(maxsize=None)
def splats(n, linearize=True, seed=None):
    raw = scenes.make_splats(n, 400 + n if seed is None else seed, 3.0)
    return raw if linearize else creator.LinearizeData(raw)


def assert_premises(raw, linearize):
    lin = creator.LinearizeData(raw) if linearize else raw
    BM.assert_no_negative_zero(lin)
    for a in (raw.pos, raw.dc0, raw.sh, raw.opacity, raw.scale, raw.rot):
        assert np.isfinite(np.asarray(a)).all()
    if not linearize:
        assert (np.asarray(raw.rot) >= 0).all() and (np.asarray(raw.rot) <= 1).all()


def check_import(ctx, raw, what, linearize=True, morton=True, want=None, source=None, **fmt):
    """import `source` (default: raw) on the GPU and hold the download to the host importer's asset of raw; returns the host asset"""
    assert_premises(raw, linearize)
    if want is None:
        want = creator.CreateAssetFromSplatsNative(raw, linearize=linearize, morton=morton, **fmt)
    g = creator.CreateGpuAssetFromSplats(raw if source is None else source, linearize=linearize, morton=morton, context=ctx, **fmt)
    try:
        got = g.Download()
        assert g.splatCount == len(raw.pos)
        BM.assert_same_asset(got, want, what)
        for name, a, b in zip(("pos", "other", "color", "sh", "chunk"), BM.blobs_of(got), BM.blobs_of(want)):
            assert (a is None and b is None) or same_bits(a, b, None), (what, name)
        assert same_bits(got.boundsMin, want.boundsMin) and same_bits(got.boundsMax, want.boundsMax), what
    finally:
        g.Dispose()
    return want


# ---- 1. every preset ----------------------------------------------------------------------------------------------------------------------------
PRESET_CASES = {
    "VeryHigh": (700, dict(quality="VeryHigh")),
    "High": (700, dict(quality="High")),
    "Medium": (700, MEDIUM),
    "CLUSTER4K": (4500, dict(quality="Medium", formatSH=SF.Cluster4k)),
    "VeryLow": (4500, dict(quality="VeryLow")),
    "LowCluster4k": (4500, dict(quality="Low", formatSH=SF.Cluster4k)),
}


@pytest.mark.parametrize("linearize,morton", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("preset", list(PRESET_CASES))
def test_every_preset(gpu_ctx, preset, linearize, morton):
    n, fmt = PRESET_CASES[preset]
    check_import(gpu_ctx, splats(n, linearize), (preset, linearize, morton), linearize, morton, **fmt)


# ---- 2. sizes around every boundary ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 32768, 32769])
def test_sizes(gpu_ctx, n):
    """a lone splat; one short of a BC7 block, a full block, one into the next; one short of a chunk, a full chunk, one into the next; 32,768 fills the
    first row of 128 texture tiles and 32,769 starts the second, whose 127 other tiles get the constant BC7 block"""
    raw = splats(n)
    check_import(gpu_ctx, raw, (n, "Medium"), **MEDIUM)
    want = check_import(gpu_ctx, raw, (n, "BC7"), **BC7)
    rows = len(want.colorData) // (512 * 16) // 4                  # the blocks lie row-major over the texture: regroup them [tile, block, byte]
    tiles = want.colorData.reshape(rows, 4, 128, 4, 16).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 16)
    assert len(tiles) == (256 if n > 32768 else 128)
    empty = tiles[(n + 255) // 256:]
    assert (empty == np.array([0x40] + [0] * 15, np.uint8)).all()


# ---- 3. the cluster rule -------------------------------------------------------------------------------------------------------------------------------
def test_cluster_rule(gpu_ctx):
    fmt = dict(quality="Medium", formatSH=SF.Cluster4k)
    raw = splats(4097)
    arrs = [np.ascontiguousarray(a, f32) for a in (raw.pos[:4096], raw.dc0[:4096], raw.sh[:4096].reshape(4096, 45), raw.opacity[:4096], raw.scale[:4096], raw.rot[:4096])]
    inp = _abi.gs_import_input(4096, *[a.ctypes.data for a in arrs])
    f = _abi.gs_import_formats(2, 2, 2, int(SF.Cluster4k), 1, 1)
    out = C.c_void_p(0x1234)
    assert _lib.lib().gs_import_encode_to_asset(gpu_ctx._h, C.byref(inp), 0, C.byref(f), C.byref(out), None, None) == BAD and not out
    text = _lib.lib().gs_last_error_string()
    sizes = (C.c_uint64 * 5)()
    assert _lib.lib().gs_import_blob_sizes(4096, C.byref(f), sizes) == BAD
    assert text and text == _lib.lib().gs_last_error_string() and b"Cluster" in text
    check_import(gpu_ctx, raw, "4097 to Cluster4k", **fmt)


# ---- 4. crafted colour blocks, input order = texel order ----------------------------------------------------------------------------------------------------
def test_crafted_blocks(gpu_ctx):
    """morton = 0, BC7 colour, two chunks + a last block of 3 splats: chunk 0 of one colour (every block has den = 0) but for one block that holds the
    chunk's extremes; in chunk 1 a block whose first splat is the chunk's brightest (the anchor flip) and one whose first is the darkest"""
    n = 256 + 240 + 3
    raw = creator.LinearizeData(scenes.make_splats(n, 77, 3.0))
    raw.dc0[:256] = f32(0.4); raw.opacity[:256] = f32(0.6)
    raw.dc0[16] = f32(0.1); raw.dc0[17] = f32(0.9)                 # one block with the chunk's two extremes
    raw.dc0[256 + 32] = f32(0.99); raw.opacity[256 + 32] = f32(0.99)
    raw.dc0[256 + 33:256 + 48] = f32(0.2); raw.opacity[256 + 33:256 + 48] = f32(0.3)
    raw.dc0[256 + 64] = f32(0.01); raw.opacity[256 + 64] = f32(0.01)
    raw.dc0[256 + 65:256 + 80] = f32(0.8); raw.opacity[256 + 65:256 + 80] = f32(0.7)
    check_import(gpu_ctx, raw, "crafted", linearize=False, morton=False, **BC7)


# ---- 5. duplicate positions -----------------------------------------------------------------------------------------------------------------------------
def test_duplicate_positions(gpu_ctx):
    """600 splats on 40 distinct points: equal codes come out in input order, as the importer's stable sort has them"""
    raw = splats(600, True, 91)
    raw = creator.InputSplatData(raw.pos[np.arange(600) % 40].copy(), raw.dc0, raw.sh, raw.opacity, raw.scale, raw.rot)
    check_import(gpu_ctx, raw, "duplicates", **MEDIUM)
    check_import(gpu_ctx, raw, "duplicates BC7", **BC7)


def test_coplanar(gpu_ctx):
    """one axis constant: max == min, the Morton component is 0 x inf = NaN, which the GPU defines as 0 and the host's conversion leaves undefined: the
    yardstick is the importer, morton = 0, of the input ordered by the model's key"""
    raw = splats(600, True, 92)
    pos = raw.pos.copy()
    pos[:, 1] = f32(0.75)
    pos[300:] = pos[:300]                                          # and duplicates among them
    raw = creator.InputSplatData(pos, raw.dc0, raw.sh, raw.opacity, raw.scale, raw.rot)
    order = np.argsort(BM.morton_codes(pos, pos.min(axis=0), pos.max(axis=0)), kind="stable")
    want = creator.CreateAssetFromSplatsNative(raw.take(order), "Medium", morton=False)
    check_import(gpu_ctx, raw, "coplanar", want=want, **MEDIUM)


# ---- 6. device arrays ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["Medium", "VeryLow"])
def test_device_arrays(gpu_ctx, preset):
    """the same arrays as torch tensors on the GPU (memory_kind = 1) give the asset of the host arrays and are left as they were.  Whichever test of a
    run touches torch's GPU side first pays for its initialisation: seconds that are not this case's"""
    import torch
    n, fmt = PRESET_CASES[preset]
    raw = splats(n)
    host = [np.ascontiguousarray(a, f32) for a in (raw.pos, raw.dc0, raw.sh.reshape(n, 45), raw.opacity, raw.scale, raw.rot)]
    dev = [torch.from_numpy(a).to("cuda:0") for a in host]
    torch.cuda.synchronize()
    before = [t.clone() for t in dev]
    check_import(gpu_ctx, raw, (preset, "device arrays"), source=creator.InputSplatData(*dev), **fmt)
    torch.cuda.synchronize()
    for t, b, a in zip(dev, before, host):
        assert torch.equal(t, b) and same_bits(t.cpu().numpy(), a)


class HipArray:
    """a float32 array in device memory of the HIP runtime the library itself runs on, with the four members CreateGpuAssetFromSplats asks of a device
    array: the memory_kind = 1 route without another framework's runtime in the process"""
    hip = None

    def __init__(self, host: np.ndarray):
        if HipArray.hip is None:
            HipArray.hip = C.CDLL("libamdhip64.so.7")              # already loaded: the library links it
        self.host = np.ascontiguousarray(host, f32)
        self.ptr = C.c_void_p()
        assert HipArray.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.host.nbytes)) == 0
        assert HipArray.hip.hipMemcpy(self.ptr, C.c_void_p(self.host.ctypes.data), C.c_size_t(self.host.nbytes), C.c_int(1)) == 0      # hipMemcpyHostToDevice

    def __len__(self): return len(self.host)
    def data_ptr(self): return self.ptr.value
    def element_size(self): return 4
    def is_floating_point(self): return True
    def is_contiguous(self): return True
    def numel(self): return self.host.size

    def download(self) -> np.ndarray:
        out = np.zeros_like(self.host)
        assert HipArray.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(out.nbytes), C.c_int(2)) == 0                  # hipMemcpyDeviceToHost
        return out

    def free(self):
        HipArray.hip.hipFree(self.ptr)


@pytest.mark.parametrize("preset", ["Medium", "VeryLow"])
def test_device_arrays_of_the_librarys_own_runtime(gpu_ctx, preset):
    n, fmt = PRESET_CASES[preset]
    raw = splats(n)
    dev = [HipArray(a) for a in (raw.pos, raw.dc0, raw.sh.reshape(n, 45), raw.opacity, raw.scale, raw.rot)]
    try:
        check_import(gpu_ctx, raw, (preset, "hip arrays"), source=creator.InputSplatData(*dev), **fmt)
        for d in dev:
            assert same_bits(d.download(), d.host)
    finally:
        for d in dev:
            d.free()


# ---- 7. a renderer over the imported asset ---------------------------------------------------------------------------------------------------------------------
def test_renderer_over_a_gpu_imported_very_low_asset(gpu_ctx):
    raw = splats(4500)
    host = creator.CreateAssetFromSplatsNative(raw, "VeryLow")
    g = creator.CreateGpuAssetFromSplats(raw, "VeryLow", context=gpu_ctx)
    r0 = make_renderer(gpu_ctx, host)
    r1 = GaussianSplatRenderer(gpu_ctx)
    try:
        r1.sortMode, r1.framesInFlight = r0.sortMode, r0.framesInFlight
        r1.CreateResourcesForGpuAsset(g)
        assert r1.splatCount == r0.splatCount == 4500
        info = (C.c_uint32 * 6)()
        _lib.check(_lib.lib().gs_asset_info(g.handle, info), "gs_asset_info")
        assert info[0] == 4500 and int(CF.BC7) in list(info)
        a, b = frame_of(r1, gpu_ctx), frame_of(r0, gpu_ctx)
        assert same_frame(a, b) and a[2].any()
    finally:
        r1.DisposeResourcesForAsset(); r0.DisposeResourcesForAsset(); g.Dispose()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(gpu_ctx):
    lib = _lib.lib()
    raw = splats(700)
    arrs = [np.ascontiguousarray(a, f32) for a in (raw.pos, raw.dc0, raw.sh.reshape(700, 45), raw.opacity, raw.scale, raw.rot)]
    ptrs = [a.ctypes.data for a in arrs]
    inp = _abi.gs_import_input(700, *ptrs)
    ok = _abi.gs_import_formats(2, 2, 2, 3, 1, 1)
    other = make_renderer(gpu_ctx, small_asset(700, 5, "Medium"))
    try:
        before = frame_of(other, gpu_ctx)
        h = gpu_ctx._h
        cases = [(None, inp, 0, ok), (h, None, 0, ok), (h, inp, 0, None), (h, _abi.gs_import_input(0, *ptrs), 0, ok), (h, inp, 2, ok),
                 (h, inp, 0, _abi.gs_import_formats(4, 2, 2, 3, 1, 1)), (h, inp, 0, _abi.gs_import_formats(2, 4, 2, 3, 1, 1)),
                 (h, inp, 0, _abi.gs_import_formats(2, 2, 4, 3, 1, 1)), (h, inp, 0, _abi.gs_import_formats(2, 2, 2, 9, 1, 1)),
                 (h, inp, 0, _abi.gs_import_formats(2, 2, 2, 3, 2, 1)), (h, inp, 0, _abi.gs_import_formats(2, 2, 2, 3, 1, 2)),
                 (h, inp, 0, _abi.gs_import_formats(2, 2, 2, int(SF.Cluster4k), 1, 1))]
        for k in range(6):
            p = list(ptrs)
            p[k] = None
            cases.append((h, _abi.gs_import_input(700, *p), 0, ok))
        for ctx_h, i, kind, f in cases:
            out = C.c_void_p(0x1234)
            rc = lib.gs_import_encode_to_asset(ctx_h, C.byref(i) if i is not None else None, kind, C.byref(f) if f is not None else None, C.byref(out), None, None)
            assert rc == BAD and not out, (kind, rc)
        assert lib.gs_import_encode_to_asset(h, C.byref(inp), 0, C.byref(ok), None, None, None) == BAD
        check_import(gpu_ctx, raw, "after the refusals", **MEDIUM)
        assert same_frame(frame_of(other, gpu_ctx), before)
    finally:
        other.DisposeResourcesForAsset()


# ---- 9. PLY to GPU asset ------------------------------------------------------------------------------------------------------------------------------------------
def test_ply_to_gpu_asset(gpu_ctx, tmp_path):
    path = str(tmp_path / "in.ply")
    creator.WritePLY(path, scenes.make_splats(3001, 21, 2.0))
    raw = creator.ReadPLY(path)
    check_import(gpu_ctx, raw, "ply", **MEDIUM)
    check_import(gpu_ctx, raw, "ply BC7", **BC7)
