"""The import on the GPU (csrc/gs_bake.hip through creator.CreateGpuAssetFromSplats) at its edges, against the native host importer of the same input
(creator.CreateAssetFromSplatsNative): the five blobs over gs_import_blob_sizes bytes byte for byte, the bounds bit for bit, the splat count -- no
tolerance anywhere.  tests/test_gpu_import_asset.py holds the presets on friendly input; here the device compile of gs_device_math.h meets arguments at
and beyond the edges of exp / sigmoid / normalize / BakeQ / BakeNorm, a chunk constant in every column, more than 262,144 splats (the second round of
bounds_fold_kernel's fold, three look-back groups in both Onesweep sorts, for the import and for the bake), Morton codes with one word constant, the
whole BC7 block set through the DPP row reductions, and device arrays that are views into larger allocations.  Every input meets the premises of
DESIGN.md section 4.11 by construction, and they are asserted on every input; the host pipeline is held to the same inputs on the CPU by
tests/test_import_gpu_model.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import bake_model as BM
import copy_model as CM
import edit_model as EM
from builders import (BC7_TARGET, EDGE_FORMATS, EDGE_SEEDS, adversarial_splats, assert_import_premises, block_set, block_set_asset, block_set_input, blocks_at,
                      edge_case, linear_input, without_negative_zero)
from common import same_bits
from gpu_rig import check_bake, pinned_renderer as make_renderer
from unitygaussiansplatting_amd import asset as A, creator, scenes

pytestmark = pytest.mark.gpu
f32 = np.float32
VF, CF, SF = A.VectorFormat, A.ColorFormat, A.SHFormat
MEDIUM = creator.QUALITY["Medium"]
VERY_LOW = creator.QUALITY["VeryLow"]
BIG = 262144 + 3 * 256 + 77                                         # 1,028 blocks of 256, the last one partial: the bounds fold's second round


def fmt_of(formats) -> dict:
    fp, fs, fc, fsh = formats
    return dict(formatPos=fp, formatScale=fs, formatColor=fc, formatSH=fsh)


def check_import(ctx, raw, formats, what, linearize=True, morton=True, want=None, source=None):
    """import `source` (default: raw) on the GPU and hold the download to the host importer's asset of raw; returns (the host asset, the download)"""
    assert_import_premises(raw, linearize)
    if want is None:
        want = creator.CreateAssetFromSplatsNative(raw, linearize=linearize, morton=morton, **fmt_of(formats))
    g = creator.CreateGpuAssetFromSplats(raw if source is None else source, linearize=linearize, morton=morton, context=ctx, **fmt_of(formats))
    try:
        got = g.Download()
        assert g.splatCount == len(raw.pos) == want.splatCount, what
        BM.assert_same_asset(got, want, what)
        for name, a, b in zip(("pos", "other", "color", "sh", "chunk"), BM.blobs_of(got), BM.blobs_of(want)):
            assert (a is None and b is None) or same_bits(a, b, None), (what, name)
        assert same_bits(got.boundsMin, want.boundsMin) and same_bits(got.boundsMax, want.boundsMax), what
        assert same_bits(g.boundsMin, want.boundsMin) and same_bits(g.boundsMax, want.boundsMax), what
    finally:
        g.Dispose()
    return want, got


# ---- a. the adversarial walk ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", EDGE_SEEDS)
def test_adversarial_walk(gpu_ctx, seed):
    """the twelve inputs of tests/test_import_gpu_model.py's walk: both linearize, both morton, eight format tuples"""
    raw = edge_case(seed)
    for linearize in (True, False):
        src = raw if linearize else linear_input(raw)
        for morton in (True, False):
            for formats in EDGE_FORMATS:
                check_import(gpu_ctx, src, formats, (seed, len(raw), formats, linearize, morton), linearize, morton)


def test_adversarial_very_low(gpu_ctx):
    """BC7 colour and a Cluster4k palette over adversarial (finite) SH rows: the palette's byte contract applies"""
    rng = np.random.default_rng(52_100)
    raw = without_negative_zero(adversarial_splats(without_negative_zero(scenes.make_splats(4500, 61, 1.0)), rng, negative_zero=False))
    check_import(gpu_ctx, raw, VERY_LOW, "adversarial VeryLow")


# ---- b. a chunk that is constant in every column ------------------------------------------------------------------------------------------------------------
def halves(words) -> np.ndarray:
    """[..., 2] float32: the (low, high) fp16 halves of uint32 words"""
    w = np.ascontiguousarray(words, np.uint32)
    return np.stack([(w & 0xffff).astype(np.uint16).view(np.float16), (w >> 16).astype(np.uint16).view(np.float16)], -1).astype(f32)


def test_constant_chunk(gpu_ctx):
    """splats 256..511 are copies of splat 256, whose fifteen SH coefficients are one rgb (an SH column spans them all): chunk 1 widens all 13
    columns by 1e-5 and normalises everything to 0; with BC7 its sixteen blocks have den = 0"""
    raw = without_negative_zero(scenes.make_splats(600, 71, 3.0))
    raw.sh[256] = raw.sh[256, 0]
    for x in (raw.pos, raw.dc0, raw.sh, raw.opacity, raw.scale, raw.rot):
        x[256:512] = x[256]
    stride = {VF.Norm11: 4, VF.Norm16: 6}
    for formats in (MEDIUM, BC7_TARGET, BM.FORMAT_TARGETS[0]):
        want, _ = check_import(gpu_ctx, raw, formats, ("constant chunk", formats), morton=False)
        rec = want.chunkData.view(np.uint32).reshape(-1, 16)
        assert len(rec) == 3
        for c in range(3):                                         # ChunkInfo: 4 colour pairs, pos min / max x 3 as fp32, 3 scale pairs, 3 SH pairs
            pos = rec[c, 4:10].view(f32).reshape(3, 2)
            pairs = halves(rec[c, [0, 1, 2, 3, 10, 11, 12, 13, 14, 15]])
            if c == 1:                                             # max = min + 1e-5 in all 13 columns (the fp16 pairs: to within their rounding)
                assert same_bits(pos[:, 1], (pos[:, 0] + f32(1.0e-5)).astype(f32)) and same_bits(pos[:, 0], raw.pos[256])
                ulp = np.abs(np.spacing(pairs[:, 0].astype(np.float16))).astype(f32)
                assert (pairs[:, 1] >= pairs[:, 0]).all() and (pairs[:, 1] - pairs[:, 0] <= f32(1.0e-5) + ulp).all()
            else:
                assert (pos[:, 1] - pos[:, 0] > 0.5).all() and (pairs[:, 1] - pairs[:, 0] > 0.01).all()
        sz = stride[formats[0]]
        assert not want.posData[256 * sz:512 * sz].any()           # the positions of chunk 1 normalise to 0


# ---- c. / d. past 262,144 splats --------------------------------------------------------------------------------------------------------------------------------
PLANTED = {"xmin": (1024 * 256 + 5, 0, -3.25), "zmin": (262143, 2, -3.5), "ymin": (BIG - 1, 1, -3.75),
           "xmax": (1025 * 256 + 17, 0, 3.25), "ymax": (BIG - 40, 1, 3.5), "zmax": (3, 2, 3.75)}


@functools.lru_cache(maxsize=None)
def big_input() -> creator.InputSplatData:
    """262,989 splats whose six global position extremes sit where the strided fold of the 1,028 partials can lose them: x-min in block 1,024 (the
    first of the fold's second round), z-min at the last index of the first round, y-min at n - 1 and y-max at n - 40 (the partial block), x-max in
    block 1,025, z-max at index 3.  make_splats clips to [-3, 3]: the planted values lie outside"""
    raw = without_negative_zero(scenes.make_splats(BIG, 81, 3.0))
    assert np.abs(raw.pos).max() <= 3.0
    for at, axis, v in PLANTED.values():
        raw.pos[at, axis] = f32(v)
    for x in (raw.pos, raw.dc0, raw.sh, raw.opacity, raw.scale, raw.rot):
        x.setflags(write=False)
    return raw


def assert_planted_bounds(asset):
    assert tuple(asset.boundsMin) == (PLANTED["xmin"][2], PLANTED["ymin"][2], PLANTED["zmin"][2])
    assert tuple(asset.boundsMax) == (PLANTED["xmax"][2], PLANTED["ymax"][2], PLANTED["zmax"][2])


@pytest.mark.parametrize("formats,morton", [(MEDIUM, True), (MEDIUM, False), (BC7_TARGET, True)], ids=["Medium", "Medium-unordered", "BC7"])
def test_past_262144_splats(gpu_ctx, formats, morton):
    """1,028 bounds partials; both sorts over 65 partitions of 4,096 keys = three look-back groups of 32"""
    raw = big_input()
    assert len(raw) == BIG and (BIG + 255) // 256 == 1028 and (BIG + 4095) // 4096 == 65
    want, _ = check_import(gpu_ctx, raw, formats, ("262,989", formats, morton), morton=morton)
    assert_planted_bounds(want)


def test_bake_past_262144_source_splats(gpu_ctx):
    """alive_list_kernel over 1,028 source chunks and the same fold: a VeryHigh renderer over the big input, every third splat deleted but for the six
    planted extremes, baked to Medium"""
    raw = big_input()
    asset = creator.CreateAssetFromSplatsNative(raw, "VeryHigh", morton=False)
    alive = np.arange(BIG) % 3 != 0
    alive[[at for at, _, _ in PLANTED.values()]] = True
    dec = CM.decode(asset)[alive]
    assert 175_000 < alive.sum() < BIG and same_bits(dec[:, 0:3], raw.pos[alive])
    r = make_renderer(gpu_ctx, asset)
    try:
        r.SetDeletedBits(EM.pack_bits(~alive, (BIG + 31) // 32))
        want = check_bake(r, dec, BM.MEDIUM, "bake of 262,989 source splats")
        assert_planted_bounds(want)
    finally:
        r.DisposeResourcesForAsset()


# ---- e. degenerate Morton words -------------------------------------------------------------------------------------------------------------------------------
def morton_words(pos):
    codes = BM.morton_codes(pos, pos.min(axis=0), pos.max(axis=0))
    return (codes & np.uint64(0xffffffff)).astype(np.uint32), (codes >> np.uint64(32)).astype(np.uint32)


def with_positions(raw, pos) -> creator.InputSplatData:
    return creator.InputSplatData(np.ascontiguousarray(pos, f32), raw.dc0, raw.sh, raw.opacity, raw.scale, raw.rot)


def test_morton_high_word_constant(gpu_ctx):
    """the cloud shrunk by 2^-13 about its mean, the mean first moved to the middle of its cell of 1,024 steps of the 21-bit grid so that no seed can
    straddle a cell, between two corner splats that keep the bounds: every other splat varies in the low 10 bits of its components only, so the order
    rests on the first sort and the second is a stable pass of single-bucket digits over five partitions"""
    n = 20000
    raw = without_negative_zero(scenes.make_splats(n, 91, 3.0))
    lo_corner, hi_corner = raw.pos.min(axis=0).astype(np.float64), raw.pos.max(axis=0).astype(np.float64)
    mean = raw.pos.mean(axis=0, dtype=np.float64)
    cell = np.floor((mean - lo_corner) / (hi_corner - lo_corner) * 2097151.0 / 1024.0)
    centre = lo_corner + (cell * 1024.0 + 512.0) / 2097151.0 * (hi_corner - lo_corner)
    pos = (centre + (raw.pos.astype(np.float64) - mean) * 2.0 ** -13).astype(f32)
    pos[0], pos[n - 1] = lo_corner, hi_corner
    pos[pos == 0] = 0
    pos[5000:5040] = pos[100:140]                                  # equal codes, far apart in the input: the stable order through both sorts
    lo, hi = morton_words(pos)
    assert len(np.unique(hi[1:n - 1])) == 1 and len(np.unique(lo[1:n - 1])) > 15000 and len(np.unique(lo[1:n - 1])) < n - 2
    check_import(gpu_ctx, with_positions(raw, pos), MEDIUM, "one high word")


def test_morton_low_word_constant(gpu_ctx):
    """every component a multiple of 2,048 steps of the 21-bit grid: the low word is 0 (all ones for the far corner), the order rests on the second
    sort, and equal codes keep the input order through both"""
    n = 20000
    raw = without_negative_zero(scenes.make_splats(n, 92, 3.0))
    k = np.random.default_rng(93).integers(0, 1024, (n, 3))
    pos = ((k * 2048 + 0.5) / 2097151.0).astype(f32)
    pos[0], pos[n - 1] = f32(0.0), f32(1.0)
    pos[5000:5040] = pos[100:140]                                  # equal codes, far apart in the input
    lo, hi = morton_words(pos)
    assert len(np.unique(lo)) <= 2 and 15000 < len(np.unique(hi)) < n
    check_import(gpu_ctx, with_positions(raw, pos), MEDIUM, "one low word")


# ---- f. the whole BC7 block set on the device ----------------------------------------------------------------------------------------------------------------------
def test_bc7_block_set(gpu_ctx):
    """the 26,000-odd blocks of tests/test_import_gpu_model.py (p-bit ties, anchor flips, den = 0, low contrast) through bake_store_bc7's row
    reductions: about 1,740 chunks, which also crosses the 1,024-partial fold with BC7 compiled in"""
    raw, offs = block_set_input()
    want = block_set_asset()
    assert len(offs) == len(block_set()) > 26000 and len(raw) > 262144 * 1.5
    assert_import_premises(raw, False)
    g = creator.CreateGpuAssetFromSplats(raw, linearize=False, morton=False, context=gpu_ctx, **fmt_of(BC7_TARGET))
    try:
        got = g.Download()
    finally:
        g.Dispose()
    bad = np.flatnonzero((blocks_at(got, offs) != blocks_at(want, offs)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:8], blocks_at(got, offs[bad[:2]]), blocks_at(want, offs[bad[:2]]))
    BM.assert_same_asset(got, want, "block set")


# ---- g. device arrays that are views --------------------------------------------------------------------------------------------------------------------------------
class HipView:
    """a float32 array one float into a larger allocation of the HIP runtime the library itself runs on: its base pointer is 4-byte but not
    16-byte aligned, and guard words (NaNs as floats) lie before and after it.  The four members CreateGpuAssetFromSplats asks of a device array"""
    hip = None
    BEFORE, AFTER, GUARD = 1, 7, 0x7fc0de00

    def __init__(self, host: np.ndarray):
        if HipView.hip is None:
            HipView.hip = C.CDLL("libamdhip64.so.7")               # already loaded: the library links it
        self.host = np.ascontiguousarray(host, f32)
        self.whole = np.full(self.BEFORE + self.host.size + self.AFTER, self.GUARD, np.uint32) + np.arange(self.BEFORE + self.host.size + self.AFTER, dtype=np.uint32) % 251
        self.whole[self.BEFORE:self.BEFORE + self.host.size] = self.host.reshape(-1).view(np.uint32)
        self.base = C.c_void_p()
        assert HipView.hip.hipMalloc(C.byref(self.base), C.c_size_t(self.whole.nbytes)) == 0
        assert HipView.hip.hipMemcpy(self.base, C.c_void_p(self.whole.ctypes.data), C.c_size_t(self.whole.nbytes), C.c_int(1)) == 0      # hipMemcpyHostToDevice
        assert self.base.value % 16 == 0 and self.data_ptr() % 16 == 4

    def __len__(self): return len(self.host)
    def data_ptr(self): return self.base.value + 4 * self.BEFORE
    def element_size(self): return 4
    def is_floating_point(self): return True
    def is_contiguous(self): return True
    def numel(self): return self.host.size

    def download(self) -> np.ndarray:
        out = np.zeros_like(self.whole)
        assert HipView.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.base, C.c_size_t(out.nbytes), C.c_int(2)) == 0                  # hipMemcpyDeviceToHost
        return out

    def free(self):
        HipView.hip.hipFree(self.base)


@pytest.mark.parametrize("preset,n", [("Medium", 700), ("VeryLow", 4500)])
def test_device_arrays_that_are_views(gpu_ctx, preset, n):
    raw = without_negative_zero(scenes.make_splats(n, 400 + n, 3.0))
    dev = [HipView(a) for a in (raw.pos, raw.dc0, raw.sh.reshape(n, 45), raw.opacity, raw.scale, raw.rot)]
    try:
        check_import(gpu_ctx, raw, creator.QUALITY[preset], (preset, "views"), source=creator.InputSplatData(*dev))
        for d in dev:
            assert np.array_equal(d.download(), d.whole)            # the arrays and the guards hold their bits
    finally:
        for d in dev:
            d.free()
