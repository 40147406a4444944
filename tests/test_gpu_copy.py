"""The merge on the GPU (csrc/gs_copy.hip through gs_renderer_edit_set_splat_count / _copy_splats_into / _download_splat_data and
GaussianSplatRenderer.EditSetSplatCount / EditCopySplatsInto / MergeSplatObjects) against the numpy model of CSCopySplats and of the resize
(tests/copy_model.py; its premises are asserted on the CPU by tests/test_copy_model.py): after every call all four blobs byte for byte -- the SH pad
and the texels at indices >= N included --, the three bit buffers, the splat count and the order; a resized renderer against a fresh renderer over
the downloaded blobs, bit for bit, and against the oracle within the suite's bar.

Two of the issue's cases are stated as they can be built: the Cluster presets need more than 4,096 / 16,384 splats, so "every preset at 513 splats"
copies the first 513 splats of a 20,000-splat source of each preset; and a lane is an object the C ABI never hands out, so its refusal cannot be
provoked from outside the library."""
import ctypes as C
import functools

import numpy as np
import pytest

import copy_model as CM
import edit_model as EM
import export_model as XM
from builders import CAMS, DST_TR, SRC_TR, decode_of
from common import PRESETS, small_asset
from gpu_rig import BAD, assert_same_frames, asset_tails, check_state, download, frames_of, native_count, oracle_frames, pinned_renderer as make_renderer
from unitygaussiansplatting_amd import _lib, asset as A, camera
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext, MergeSplatObjects, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
f32 = np.float32


def boundary_bits(n: int) -> np.ndarray:
    """deleted words with bits on both sides of every word boundary the source has"""
    flags = np.zeros(n, bool)
    flags[[k for k in (0, 31, 32, 63, 64, 255, 256, n - 1) if k < n]] = True
    return EM.pack_bits(flags, (n + 31) // 32)


# ---- 1. counts and offsets ------------------------------------------------------------------------------------------------------------------
SOURCES = [(1, "VeryHigh", False), (63, "VeryHigh", False), (64, "VeryHigh", False), (65, "VeryHigh", True), (257, "Medium", True), (513, "High", True)]


@pytest.mark.parametrize("dst_n", [33, 255, 256, 257, 300])
def test_counts_and_offsets(gpu_ctx, dst_n):
    """Every source size into every offset of one destination, the model following call by call.  dst_start 33 and 95 make two waves (33: lanes 31 / 32
    of a source wave) and, from 257 splats on, two workgroups share a destination deleted word; the two largest sources live on a context of their own."""
    dst_asset = small_asset(dst_n, 5, "VeryHigh")
    dst = make_renderer(gpu_ctx, dst_asset, DST_TR)
    want, tails = CM.blobs_of(dst_asset), asset_tails(dst_asset)
    other_ctx = GpuContext(gpu_ctx.device)
    ident = np.arange(dst_n, dtype=np.uint32)
    check_state(dst, want, "before", tails, order=ident)
    try:
        for n, quality, with_bits in SOURCES:
            tr = SRC_TR if n in (65, 513) else camera.Transform()
            src = make_renderer(other_ctx if n >= 257 else gpu_ctx, small_asset(n, 5, quality), tr)
            words = boundary_bits(n) if with_bits else None
            src.SetDeletedBits(words)
            dec, xf = decode_of(n, quality), CM.copy_transform(tr, DST_TR)
            for dst_start in (0, 33, 95):
                count = n + 100 if dst_start == 95 else n          # (95: src_start + count runs past the source's end; 0 / 33 with a large source: past the destination's)
                src.EditCopySplatsInto(dst, 0, dst_start, count)
                CM.copy_splats(dec, words, want, xf, 0, dst_start, count)
                check_state(dst, want, (dst_n, n, dst_start), tails, order=ident)
            if n == 513:                                           # the literal index: the data of idx under the deleted bits of src_start + idx; and count = 0
                src.EditCopySplatsInto(dst, 5, 33, 600)
                CM.copy_splats(dec, words, want, xf, 5, 33, 600)
                check_state(dst, want, (dst_n, n, "src_start 5"), tails, order=ident)
                src.EditCopySplatsInto(dst, 0, 0, 0)
                check_state(dst, want, (dst_n, n, "count 0"), tails, order=ident)
            assert dst.editModified
            src.DisposeResourcesForAsset()
    finally:
        dst.DisposeResourcesForAsset()
        other_ctx.Dispose()


# ---- 2. every preset ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", PRESETS)
def test_every_preset_into_a_very_high_destination(gpu_ctx, quality):
    """the first 513 splats of a 20,000-splat source of every preset (Norm11 / Norm6 / fp16 / Cluster SH, BC7 and Norm8 colour, chunked positions);
    VeryLow, Medium and VeryHigh with deleted bits on both sides of the word boundaries, Low and High without a deleted buffer"""
    dst_asset = small_asset(20100, 5, "VeryHigh")
    dst = make_renderer(gpu_ctx, dst_asset, DST_TR)
    want, tails = CM.blobs_of(dst_asset), asset_tails(dst_asset)
    src = make_renderer(gpu_ctx, small_asset(20000, 5, quality), SRC_TR)
    words = boundary_bits(20000) if quality in ("VeryLow", "Medium", "VeryHigh") else None
    src.SetDeletedBits(words)
    before = download(src)
    src.EditCopySplatsInto(dst, 0, 33, 513)
    CM.copy_splats(decode_of(20000, quality), words, want, CM.copy_transform(SRC_TR, DST_TR), 0, 33, 513)
    check_state(dst, want, quality, tails, order=np.arange(20100, dtype=np.uint32))
    assert (want.deleted is None) == (words is None)
    # ... and the whole source with a count past its end: the clamp at the source's end and its partial last chunk (32 splats) in every format
    src.EditCopySplatsInto(dst, 0, 0, 25000)
    CM.copy_splats(decode_of(20000, quality), words, want, CM.copy_transform(SRC_TR, DST_TR), 0, 0, 25000)
    check_state(dst, want, (quality, "count past the source's end"), tails, order=np.arange(20100, dtype=np.uint32))
    assert np.array_equal(want.pos[12 * 20000:], CM.blobs_of(dst_asset).pos[12 * 20000:])      # the destination's last 100 splats are its own
    after = download(src)                                          # the source renderer of a copy is unchanged
    assert all(np.array_equal(getattr(before, f), getattr(after, f)) for f in ("pos", "other", "color", "sh", "deleted"))
    src.DisposeResourcesForAsset(); dst.DisposeResourcesForAsset()


# ---- 3. resize ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resize_reference(n0: int, n1: int):
    """the model of one resize and the oracle's frames of its result: computed once, shared by the three modes"""
    words = EM.pack_bits(np.random.default_rng(n0 + n1).random(n0) < 0.3, (n0 + 31) // 32)
    want = CM.set_splat_count(decode_of(n0, "VeryHigh"), words, n1)
    return words, want, oracle_frames(want.asset(), want.deleted, DST_TR)


@pytest.mark.parametrize("mode", ["full", "visible", "lanes"])
@pytest.mark.parametrize("n0,n1", [(300, 1000), (300, 130), (32700, 32800)])
def test_resize(gpu_ctx, n0, n1, mode):
    """grow, shrink (a partial last word: no bit or record at an index >= N) and grow across 32,768, where the colour texture gains its second
    16-row Morton band.  "lanes": SetFramesInFlight(2) BEFORE the resize; the lanes are made again and the frames are the one-at-a-time renderer's."""
    words, want, oracle = resize_reference(n0, n1)
    sort_mode = SortMode.Full if mode == "full" else SortMode.Visible
    r = make_renderer(gpu_ctx, small_asset(n0, 5, "VeryHigh"), DST_TR, sort_mode, 2 if mode == "lanes" else 1)
    r.SetDeletedBits(words)
    r.SetSortHistoryLimit(3)
    r.EditSelectAll(); r.EditStoreSelectionMouseDown(); r.EditStorePosMouseDown(); r.EditStoreOtherMouseDown()
    assert r.DownloadEditBits()[0].any()
    rt = RenderTarget(gpu_ctx, 320, 200)
    r.SortPoints(CAMS[1]); r.CalcViewData(CAMS[1]); rt.Clear(); r.Draw(CAMS[1], rt)
    sorted_order = r.DownloadOrder()
    assert not np.array_equal(sorted_order, np.arange(n0, dtype=np.uint32))
    r.EditSetSplatCount(n0)                                        # a count equal to N: nothing happens
    assert _lib.lib().gs_renderer_edit_set_splat_count(r._r_h, n0, None) == 0
    assert np.array_equal(r.DownloadOrder(), sorted_order) and r.DownloadEditBits()[0].any() and native_count(r) == n0
    r.EditSetSplatCount(n1)
    got = check_state(r, want, (n0, n1, mode), order=np.arange(n1, dtype=np.uint32))      # identity order; selection and its copy zero
    assert r.editModified and not r.m_GpuEditPosMouseDown
    if n1 < n0:
        assert not EM.unpack_bits(got.deleted, 32 * want.words)[n1:].any()
    # the pos / other mouse-down copies are gone: a scale is refused like on a fresh renderer
    one, eye = (C.c_float * 3)(1, 1, 1), (C.c_float * 16)(*np.eye(4, dtype=f32).reshape(-1))
    assert _lib.lib().gs_renderer_edit_scale_selection(r._r_h, one, eye, eye, one) == BAD
    assert r.FramesInFlight() == ((2, True) if mode == "lanes" else (1, False)) and r.SortHistory()[:2] == (0, 3)
    # a fresh renderer over the downloaded blobs, the same deleted bits and settings: order, view records and frames bit for bit
    fresh = make_renderer(gpu_ctx, got.asset(), DST_TR, sort_mode)
    fresh.SetDeletedBits(got.deleted)
    fresh.SetSortHistoryLimit(3)
    mine, theirs = frames_of(r, gpu_ctx), frames_of(fresh, gpu_ctx)
    assert_same_frames(mine, theirs, (n0, n1, mode, "fresh"))
    assert_same_frames(mine, oracle, (n0, n1, mode, "oracle"), bits=False)
    assert any(img.any() for _, img in mine[0])
    rt.Dispose(); fresh.DisposeResourcesForAsset(); r.DisposeResourcesForAsset()


def test_resize_away_and_back_to_an_odd_count(gpu_ctx):
    """257 -> 130 -> 257 -> 300 -> 257: back at the asset's own count the blobs are the private ones of the VeryHigh layout -- whole records, where the
    importer pads the asset's pos blob of an odd count by a dword -- and the downloads size themselves accordingly"""
    asset = small_asset(257, 5, "VeryHigh")
    assert len(asset.posData) != 12 * 257                          # premise: the asset's blob is padded
    r = make_renderer(gpu_ctx, asset, DST_TR)
    words = boundary_bits(257)
    r.SetDeletedBits(words)
    want = CM.blobs_of(asset)
    want.deleted = words.copy()
    for n in (130, 257, 300, 257):
        r.EditSetSplatCount(n)
        want = CM.set_splat_count(CM.decode(want), want.deleted, n)
        got = check_state(r, want, ("back and forth", n), order=np.arange(n, dtype=np.uint32))
        pos, other = r.DownloadPosOther()
        assert np.array_equal(pos, got.pos) and np.array_equal(other, got.other) and len(pos) == 12 * n
    assert not want.pos[12 * 130:].any() and want.pos[:12 * 130].any()      # what the shrink cut off came back as zeros
    other = GaussianSplatRenderer(gpu_ctx, asset, DST_TR)
    other.ShareResourcesOf(r)                                      # a renderer over the same asset has the asset's count and blobs, not the resized ones
    r.EditSetSplatCount(300)
    assert other.splatCount == 257 == native_count(other) and len(other.DownloadSplatData()[0]) == len(asset.posData)
    other.DisposeResourcesForAsset(); r.DisposeResourcesForAsset()


# ---- 4. the merge command, and the edit tools on its result -------------------------------------------------------------------------------------
def merged(ctx):
    target = make_renderer(ctx, small_asset(300, 5, "VeryHigh"), DST_TR)
    a = make_renderer(ctx, small_asset(257, 6, "Medium"))
    b = make_renderer(ctx, small_asset(65, 7, "VeryHigh"), SRC_TR)           # mirrored
    MergeSplatObjects(target, [target, a, b])
    want = CM.merge(CM.blobs_of(small_asset(300, 5, "VeryHigh")), DST_TR,
                    [(decode_of(257, "Medium", 6), None, camera.Transform()), (decode_of(65, "VeryHigh", 7), None, SRC_TR)])
    a.DisposeResourcesForAsset(); b.DisposeResourcesForAsset()
    return target, want


def test_merge_splat_objects(gpu_ctx):
    r, want = merged(gpu_ctx)
    assert r.splatCount == 622 == want.n
    got = check_state(r, want, "merge", order=np.arange(622, dtype=np.uint32))
    mine = frames_of(r, gpu_ctx)
    assert_same_frames(mine, oracle_frames(got.asset(), None, DST_TR), "merge vs oracle", bits=False)
    assert all(img.any() for _, img in mine[0])
    r.DisposeResourcesForAsset()


def test_edit_tools_work_on_the_merged_renderer(gpu_ctx, tmp_path):
    r, want = merged(gpu_ctx)
    m = EM.EditModel(want.asset())
    r.EditSelectAll(); m.select_all()
    assert np.array_equal(r.DownloadEditBits()[0], m.bits()[0]) and r.editSelectedSplats == m.info()[0] == 640      # (the tail bits of the last word count)
    r.EditDeselectAll(); m.deselect_all()
    cam = CAMS[0]
    P = r.FrameParams(cam)
    r.EditStoreSelectionMouseDown(); m.store_selection()
    r.EditUpdateSelection((EM.PREMISE_RECT[0], EM.PREMISE_RECT[3]), (EM.PREMISE_RECT[2], EM.PREMISE_RECT[1]), cam, False)
    m.update_selection(P, EM.PREMISE_RECT, False)
    sel = r.DownloadEditBits()[0]
    assert np.array_equal(sel, m.bits()[0]) and EM.popcount(sel) == 134     # (84 of them among the merged splats: tests/test_copy_model.py)
    # translate: the selected positions move by the delta, the others stay
    delta = np.array([0.25, -0.5, 0.125], f32)
    r.EditTranslateSelection(delta)
    moved = download(r)
    flags = EM.unpack_bits(sel, 622)
    pos0, pos1 = want.pos.view(f32).reshape(622, 3), moved.pos.view(f32).reshape(622, 3)
    assert np.array_equal(pos1[flags].view(np.uint32), (pos0[flags] + delta[None, :]).astype(f32).view(np.uint32)) and np.array_equal(pos1[~flags], pos0[~flags])
    assert all(np.array_equal(getattr(moved, f), getattr(want, f)) for f in ("other", "color", "sh"))
    r.EditDeleteSelected()
    deleted = r.DownloadEditBits()[2]
    assert np.array_equal(deleted, sel)
    # ExportPlyFile: the record count is the alive count, the records export_model's over the downloaded blobs
    xm = XM.ExportModel(moved.asset())
    xm.edit.set_deleted_bits(deleted)
    rows = xm.export_alive()
    assert len(rows) == 622 - int(flags.sum())
    path = str(tmp_path / "merged.ply")
    assert r.ExportPlyFile(path) == len(rows)
    alive = r.ExportAlive()
    assert alive.shape == rows.shape and np.array_equal(alive.view(np.uint32), rows.view(np.uint32))
    from unitygaussiansplatting_amd import creator
    back = creator.ReadPLY(path)
    assert np.array_equal(np.ascontiguousarray(back.pos, f32).view(np.uint32), np.ascontiguousarray(rows[:, 0:3]).view(np.uint32))
    r.DisposeResourcesForAsset()


# ---- 5. nothing shared is written ---------------------------------------------------------------------------------------------------------------
def asset_device_bytes(r):
    lib, hip = _lib.lib(), C.CDLL("libamdhip64.so")               # (the runtime the library itself is linked against)
    ptrs, sizes = (C.c_void_p * 5)(), (C.c_uint64 * 5)()
    _lib.check(lib.gs_asset_device_blobs(r._asset_h, ptrs, sizes), "gs_asset_device_blobs")
    out = []
    for k in range(4):
        host = np.zeros(int(sizes[k]), np.uint8)
        assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptrs[k]), C.c_size_t(int(sizes[k])), 2) == 0      # hipMemcpyDeviceToHost
        out.append(host)
    return out


def test_nothing_shared_is_written(gpu_ctx):
    asset = small_asset(300, 5, "VeryHigh")
    first = make_renderer(gpu_ctx, asset, DST_TR)
    ctx2 = GpuContext(gpu_ctx.device)
    second = GaussianSplatRenderer(ctx2, asset, DST_TR)
    second.ShareResourcesOf(first)
    src = make_renderer(gpu_ctx, small_asset(257, 6, "Medium"))
    try:
        before_frames, before_bytes = frames_of(second, ctx2), asset_device_bytes(first)
        first.EditSetSplatCount(600)
        src.EditCopySplatsInto(first, 0, 300, 257)
        first.ctx.Synchronize()
        second.ResetOrder()
        assert native_count(first) == 600 and native_count(second) == 300
        assert_same_frames(frames_of(second, ctx2), before_frames, "the sharing renderer")
        assert all(np.array_equal(x, y) for x, y in zip(asset_device_bytes(first), before_bytes))
        # ... and copy-on-write without a resize: a copy into a renderer over the shared asset leaves the asset alone too
        src.EditCopySplatsInto(second, 0, 10, 100)
        ctx2.Synchronize()
        assert all(np.array_equal(x, y) for x, y in zip(asset_device_bytes(first), before_bytes))
        assert not np.array_equal(download(second).pos[:12 * 300], np.ascontiguousarray(asset.posData, np.uint8)[:12 * 300])
    finally:
        src.DisposeResourcesForAsset(); second.DisposeResourcesForAsset(); first.DisposeResourcesForAsset()
        ctx2.Dispose()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_renderer_unchanged(gpu_ctx):
    lib = _lib.lib()
    vh = small_asset(300, 5, "VeryHigh")
    good = make_renderer(gpu_ctx, vh)
    chunked = make_renderer(gpu_ctx, small_asset(300, 5, "Medium"))
    # chunk-less, but fp16 scales (an other record of 4 + 6 bytes): a descriptor the importer never makes and the C ABI accepts
    half = A.GaussianSplatAsset(splatCount=300, posFormat=A.VectorFormat.Float32, scaleFormat=A.VectorFormat.Norm16, shFormat=A.SHFormat.Float32,
                                colorFormat=A.ColorFormat.Float32x4, posData=np.ascontiguousarray(vh.posData, np.uint8).copy(), otherData=np.zeros(300 * 10 + 4, np.uint8),
                                colorData=np.ascontiguousarray(vh.colorData, np.uint8).copy(), shData=np.ascontiguousarray(vh.shData, np.uint8).copy(), chunkData=None)
    half.dataHash = half.ComputeDataHash()
    fp16 = make_renderer(gpu_ctx, half)
    p = good.CopyParams(good)

    def snapshot(r):
        d = download(r)
        return native_count(r), [d.pos, d.other, d.color, d.sh, d.deleted], r.DownloadOrder()

    def unchanged(r, snap):
        now = snapshot(r)
        return now[0] == snap[0] and all(np.array_equal(x, y) for x, y in zip(now[1], snap[1])) and np.array_equal(now[2], snap[2])

    for r in (chunked, fp16):
        snap = snapshot(r)
        assert lib.gs_renderer_edit_set_splat_count(r._r_h, 400, None) == BAD
        assert lib.gs_renderer_edit_copy_splats_into(good._r_h, r._r_h, C.byref(p), 0, 0, 10) == BAD
        assert unchanged(r, snap)
    chunked.EditSetSplatCount(400)                                 # the Python method returns silently where the C# logs an error
    assert chunked.splatCount == 300 and native_count(chunked) == 300
    snap = snapshot(good)
    assert lib.gs_renderer_edit_copy_splats_into(good._r_h, good._r_h, C.byref(p), 0, 0, 10) == BAD            # src == dst
    assert lib.gs_renderer_edit_set_splat_count(good._r_h, 0, None) == BAD
    assert lib.gs_renderer_edit_set_splat_count(good._r_h, (1 << 30) + 1, None) == BAD                      # above the sort's limit
    good.EditSetSplatCount(0); good.EditSetSplatCount(-3); good.EditSetSplatCount(A.kMaxSplats + 1)
    assert unchanged(good, snap) and good.splatCount == 300
    # a source of any format is fine: chunked into good
    assert lib.gs_renderer_edit_copy_splats_into(chunked._r_h, good._r_h, C.byref(p), 0, 0, 10) == 0
    assert not unchanged(good, snap)
    for r in (good, chunked, fp16):
        r.DisposeResourcesForAsset()
