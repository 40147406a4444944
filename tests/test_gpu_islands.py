"""-m gpu: gs_renderer_edit_components, gs_renderer_edit_select_islands and gs_renderer_edit_grow_selection against the numpy twin of
tests/islands_model.py (brute force up to 5,000 alive splats, the grid model -- held to brute force by tests/test_islands_model.py -- above that).
Labels, sizes and selection words are unique whatever order the GPU links in: exact integers and exact words, all N entries, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import edit_model as EM
import islands_model as IM
import neighbour_model as NM
import neighbour_rig as NR
from builders import decode_of, fp32_point_asset
from common import PRESETS, default_camera, small_asset
from gpu_rig import BAD, edit_info, pinned_renderer
from unitygaussiansplatting_amd import _lib, camera
from unitygaussiansplatting_amd._lib import GsError
from unitygaussiansplatting_amd.cutout import GaussianCutout, Type
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
f32 = np.float32


def point_renderer(ctx, pos):
    return pinned_renderer(ctx, fp32_point_asset(pos))


def words_of(n):
    return (n + 31) // 32


def check_components(r, pos, alive, radius, what):
    """the call against the twin; returns the twin's (labels, sizes)"""
    alive = np.asarray(alive, bool)
    want = IM.components(pos, alive, radius)
    labels, sizes = r.EditComponents(radius)
    bad = np.flatnonzero((labels != want[0]) | (sizes != want[1]))
    assert len(bad) == 0, (what, radius, bad[:8], labels[bad[:8]], want[0][bad[:8]], sizes[bad[:8]], want[1][bad[:8]])
    return want


def check_select(r, pos, labels, sizes, alive, radius, what, ks=(2, 4)):
    """islands added at every k on an empty selection; min_size 2 is select_sparse at 1, word for word; add then subtract; and the selection grown from
    the splat in the middle of the index range"""
    n = len(sizes)
    zero = np.zeros(words_of(n), np.uint32)
    for k in ks:
        r.EditDeselectAll()
        r.EditSelectIslands(radius, k)
        got, want = r.DownloadEditBits()[0], IM.select_islands(zero, sizes, alive, k)
        assert np.array_equal(got, want), (what, "add", k, np.flatnonzero(got != want)[:8])
    r.EditDeselectAll()
    r.EditSelectSparse(radius, 1)
    sparse = r.DownloadEditBits()[0]
    r.EditDeselectAll()
    r.EditSelectIslands(radius, 2)
    assert np.array_equal(r.DownloadEditBits()[0], sparse) and np.array_equal(sparse, IM.select_islands(zero, sizes, alive, 2)), (what, "islands 2 == sparse 1")
    big = max(ks) + 3
    r.EditDeselectAll()
    r.EditSelectIslands(radius, big)
    r.EditSelectIslands(radius, 2, subtract=True)
    want = IM.select_islands(IM.select_islands(zero, sizes, alive, big), sizes, alive, 2, subtract=True)
    assert np.array_equal(r.DownloadEditBits()[0], want), (what, "subtract")
    seed = zero.copy()
    seed[(n // 2) >> 5] = np.uint32(1) << np.uint32((n // 2) & 31)
    r.UploadSelectedBits(seed)
    r.EditGrowSelection(radius)
    got, want = r.DownloadEditBits()[0], IM.grow_selection(seed, labels, alive)
    assert np.array_equal(got, want), (what, "grow", np.flatnonzero(got != want)[:8])
    r.EditDeselectAll()


# ---- 1. sizes: the sort's small-partition edge, several workgroups; a radius that isolates everything, a typical one, one that makes a single cell ------
@pytest.mark.parametrize("n", [1, 2, 33, 255, 256, 257, 4095, 4097, 20000])
def test_sizes_with_isolating_typical_and_one_cell_radii(gpu_ctx, n):
    pos, radius = NR.gaussian(n, 100 + n)
    alive = np.ones(n, bool)
    r = point_renderer(gpu_ctx, pos)
    try:
        labels, sizes = check_components(r, pos, alive, NR.isolating_radius(pos), (n, "isolating"))
        assert np.array_equal(labels, np.arange(n)) and (sizes == 1).all()
        labels, sizes = check_components(r, pos, alive, radius, (n, "typical"))
        if n >= 255:
            assert sizes.max() > n // 4 and (sizes == 1).any() and len(np.unique(labels)) > 8
        check_select(r, pos, labels, sizes, alive, radius, (n, "typical"))
        if n <= 4097:
            labels, sizes = check_components(r, pos, alive, NR.one_cell_radius(pos), (n, "one cell"))
            assert not labels.any() and (sizes == n).all()
    finally:
        r.DisposeResourcesForAsset()


# ---- 2. the new families -----------------------------------------------------------------------------------------------------------------------------------
CHAIN_N = 4097
GAPS = (0, 255, 256, 1000, 2047, 4000, 4094)


@pytest.mark.parametrize("axis", range(3))
def test_a_shuffled_chain_is_one_component_labelled_0(gpu_ctx, axis):
    pos, radius, where = IM.chain(CHAIN_N, 4 + axis, axis)
    alive = np.ones(CHAIN_N, bool)
    r = point_renderer(gpu_ctx, pos)
    try:
        labels, sizes = check_components(r, pos, alive, radius, ("chain", axis))
        assert not labels.any() and (sizes == CHAIN_N).all() and where[0] != 0 and CHAIN_N > 16 * 256
        r.UploadSelectedBits(EM.pack_bits(np.arange(CHAIN_N) == where[CHAIN_N - 1], words_of(CHAIN_N)))      # the far end of the line
        r.EditGrowSelection(radius)
        assert np.array_equal(r.DownloadEditBits()[0], EM.pack_bits(alive, words_of(CHAIN_N)))
        assert r.editSelectedSplats == CHAIN_N
    finally:
        r.DisposeResourcesForAsset()


def test_a_broken_chain_has_the_closed_form_sizes(gpu_ctx):
    pos, radius, where, want = IM.broken_chain(CHAIN_N, 5, GAPS)
    alive = np.ones(CHAIN_N, bool)
    r = point_renderer(gpu_ctx, pos)
    try:
        labels, sizes = check_components(r, pos, alive, radius, "broken chain")
        piece = np.repeat(np.arange(len(want)), want)
        for k, size in enumerate(want):
            members = where[piece == k]
            assert (sizes[members] == size).all() and (labels[members] == members.min()).all(), k
        assert len(want) == len(GAPS) + 1 and len(np.unique(labels)) == len(want)
        check_select(r, pos, labels, sizes, alive, radius, "broken chain", ks=(2, 3, 95, 256))
    finally:
        r.DisposeResourcesForAsset()


def test_a_ring_closes_on_equal_roots(gpu_ctx):
    pos, radius, _ = IM.ring(CHAIN_N, 7)
    r = point_renderer(gpu_ctx, pos)
    try:
        labels, sizes = check_components(r, pos, np.ones(CHAIN_N, bool), radius, "ring")
        assert not labels.any() and (sizes == CHAIN_N).all()
    finally:
        r.DisposeResourcesForAsset()


def test_a_bridge_deleted_or_cut_splits_the_component(gpu_ctx):
    pos, radius, b = IM.bridge(100, 8)
    n = len(pos)
    asset = fp32_point_asset(pos)
    m = EM.EditModel(asset)
    r = pinned_renderer(gpu_ctx, asset)
    try:
        labels, sizes = check_components(r, pos, np.ones(n, bool), radius, "bridge")
        assert not labels.any() and (sizes == n).all()
        # deleted
        gone = np.arange(n) == b
        r.SetDeletedBits(EM.pack_bits(gone, words_of(n)))
        labels, sizes = check_components(r, pos, ~gone, radius, "bridge deleted")
        assert labels[b] == IM.NOT_ALIVE and sizes[b] == 0 and sorted(set(labels[~gone].tolist())) == [0, b + 1] and (sizes[~gone] == 100).all()
        seed = np.zeros(words_of(n), np.uint32)
        seed[0] = 1 << 3
        r.UploadSelectedBits(seed)
        r.EditGrowSelection(radius)
        assert np.array_equal(r.DownloadEditBits()[0], EM.pack_bits(np.arange(n) < b, words_of(n)))       # the first cluster, not the bridge, not the second
        # cut by a cutout, the deleted bit cleared again
        r.EditDeselectAll()
        r.SetDeletedBits(np.zeros(words_of(n), np.uint32))
        cuts = [GaussianCutout(Type.Ellipsoid, True, camera.Transform(position=(0.8, 0.0, 0.0), scale=(0.4, 0.4, 0.4)))]
        r.m_Cutouts = cuts
        m.set_cutouts(cuts, r.transform.localToWorldMatrix)
        assert m.cut.sum() == 1 and m.cut[b]
        labels, sizes = check_components(r, pos, ~m.cut, radius, "bridge cut")
        assert labels[b] == IM.NOT_ALIVE and sorted(set(labels[~m.cut].tolist())) == [0, b + 1]
        r.EditSelectIslands(radius, 101)
        assert np.array_equal(r.DownloadEditBits()[0], EM.pack_bits(~m.cut, words_of(n))) and r.editSelectedSplats == 200
    finally:
        r.DisposeResourcesForAsset()


def test_clumps_smaller_than_min_size_are_selected_and_edit_info_follows(gpu_ctx):
    groups = 24
    pos, radius, group = IM.clumps(groups, 9)
    n = len(pos)
    alive = np.ones(n, bool)
    asset = fp32_point_asset(pos)
    m = EM.EditModel(asset)
    r = pinned_renderer(gpu_ctx, asset)
    try:
        labels, sizes = check_components(r, pos, alive, radius, "clumps")
        assert np.array_equal(sizes, group) and len(np.unique(labels)) == groups
        for k in (0, 1, 2, 7, 24, 25, 1000):
            r.EditDeselectAll()
            r.EditSelectIslands(radius, k)
            words = r.DownloadEditBits()[0]
            assert np.array_equal(words, EM.pack_bits(group < k, words_of(n))), k
            kk = min(k, groups + 1)
            assert r.editSelectedSplats == max(kk - 1, 0) * kk // 2, k     # 1 + 2 + .. + (k - 1)
            m.upload_selected(words)
            assert np.array_equal(EM.info_words(edit_info(r)), m.info()), k
        # keep the main body, select the rest: everything but the largest group
        r.EditDeselectAll()
        r.EditSelectIslands(radius, int(sizes.max()))
        assert np.array_equal(r.DownloadEditBits()[0], EM.pack_bits(group < groups, words_of(n)))
    finally:
        r.DisposeResourcesForAsset()


# ---- 3. the families of the neighbour counts: the exact-radius lattice, the far clouds, ulp pairs, the clamp, duplicates, non-finite positions ------------
@pytest.mark.parametrize("family", range(8))
def test_adversarial_families(gpu_ctx, family):
    name, pos, radius = NR.adversarial(1500, 3)[family]
    alive = np.ones(len(pos), bool)
    r = point_renderer(gpu_ctx, pos)
    try:
        labels, sizes = check_components(r, pos, alive, radius, name)
        check_select(r, pos, labels, sizes, alive, radius, name)
    finally:
        r.DisposeResourcesForAsset()


def test_an_identical_cloud_is_one_component_at_any_radius(gpu_ctx):
    pos, radius = NR.identical(300)
    r = point_renderer(gpu_ctx, pos)
    try:
        for rad in (radius, 1.0e-15, 1.0e15):
            labels, sizes = check_components(r, pos, np.ones(300, bool), rad, "identical")
            assert not labels.any() and (sizes == 300).all()
    finally:
        r.DisposeResourcesForAsset()


def test_non_finite_positions_are_components_of_their_own(gpu_ctx):
    pos, radius = NR.non_finite(257, 4)
    bad = ~np.isfinite(pos).all(axis=1)
    assert bad.sum() == 7
    alive = np.ones(257, bool)
    r = point_renderer(gpu_ctx, pos)
    try:
        one = NR.one_cell_radius(pos[~bad])
        labels, sizes = check_components(r, pos, alive, one, "non-finite")
        assert np.array_equal(labels[bad], np.flatnonzero(bad)) and (sizes[bad] == 1).all() and (sizes[~bad] == 250).all() and not labels[~bad].any()
        r.EditSelectIslands(one, 2)
        assert np.array_equal(r.DownloadEditBits()[0], EM.pack_bits(bad, 9))
        r.EditGrowSelection(one)                                   # a non-finite seed grows to itself only
        assert np.array_equal(r.DownloadEditBits()[0], EM.pack_bits(bad, 9))
    finally:
        r.DisposeResourcesForAsset()


# ---- 4. sources: every preset's decode, and the private pos blob a translate made ---------------------------------------------------------------------------
@pytest.mark.parametrize("quality", PRESETS)
def test_every_preset_as_the_source(gpu_ctx, quality):
    # (a Cluster* SH table needs more splats than entries: those two presets at the 20,000 whose decode tests/test_gpu_copy.py shares)
    n, radius = (20000, 0.12) if quality in ("VeryLow", "Low") else (700, 0.35)
    pos = np.ascontiguousarray(decode_of(n, quality)[:, :3], f32)
    r = pinned_renderer(gpu_ctx, small_asset(n, 5, quality))
    try:
        labels, sizes = check_components(r, pos, np.ones(n, bool), radius, quality)
        assert sizes.max() >= 40 and (sizes == 1).sum() >= 40
        check_select(r, pos, labels, sizes, np.ones(n, bool), radius, quality, ks=(3,))
    finally:
        r.DisposeResourcesForAsset()


def test_moving_half_a_cluster_away_splits_it(gpu_ctx):
    n = 400
    pos = (np.random.default_rng(9).standard_normal((n, 3)) * 0.05).astype(f32)
    radius = 0.5
    r = point_renderer(gpu_ctx, pos)
    try:
        labels, sizes = check_components(r, pos, np.ones(n, bool), radius, "before")
        assert not labels.any() and (sizes == n).all()
        sel = np.zeros(n, bool)
        sel[1::2] = True
        r.UploadSelectedBits(EM.pack_bits(sel, words_of(n)))
        r.EditStorePosMouseDown()
        r.EditTranslateSelection((5.0, 0.25, -0.125))
        moved = np.frombuffer(r.DownloadPosOther()[0].tobytes(), f32)[:3 * n].reshape(n, 3)
        assert np.array_equal(moved[~sel], pos[~sel]) and not np.array_equal(moved[sel], pos[sel])
        labels, sizes = check_components(r, moved, np.ones(n, bool), radius, "after")
        assert np.array_equal(labels, np.where(sel, 1, 0)) and (sizes == n // 2).all()
    finally:
        r.DisposeResourcesForAsset()


# ---- 5. dead splats --------------------------------------------------------------------------------------------------------------------------------------------
def test_dead_splats_join_nothing_are_no_seeds_and_are_never_selected(gpu_ctx):
    n = 700
    asset = small_asset(n, 5, "Medium")
    m = EM.EditModel(asset)
    r = pinned_renderer(gpu_ctx, asset)
    nw = words_of(n)
    deleted = np.random.default_rng(5).random(n) < 0.3
    cuts = [GaussianCutout(Type.Ellipsoid, False, camera.Transform(position=(0.4, -0.2, 0.3), scale=(2.2, 1.6, 2.0)))]
    radius = 0.5
    try:
        everyone = check_components(r, m.pos, np.ones(n, bool), radius, "all alive")
        r.SetDeletedBits(EM.pack_bits(deleted, nw))
        r.m_Cutouts = cuts
        m.set_cutouts(cuts, r.transform.localToWorldMatrix)
        alive = NM.alive_flags(n, EM.pack_bits(deleted, nw), m.cut)
        assert 100 < alive.sum() < n - 100 and (m.cut & ~deleted).sum() > 50
        labels, sizes = check_components(r, m.pos, alive, radius, "deleted + cut")
        assert (sizes[alive] < everyone[1][alive]).any() and sizes.max() >= 20
        check_select(r, m.pos, labels, sizes, alive, radius, "deleted + cut")
        # seeds: a deleted splat's bit is no seed and stays as it is; an alive one grows
        big = int(np.flatnonzero(alive & (sizes == sizes.max()))[0])
        gone = int(np.flatnonzero(deleted)[0])
        for flags in ((np.arange(n) == gone), (np.arange(n) == gone) | (np.arange(n) == big)):
            seed = EM.pack_bits(flags, nw)
            r.UploadSelectedBits(seed)
            r.EditGrowSelection(radius)
            want = IM.grow_selection(seed, labels, alive)
            assert np.array_equal(r.DownloadEditBits()[0], want)
            assert EM.popcount(want) == (1 if flags.sum() == 1 else 1 + int(sizes.max()))
        r.EditDeselectAll()
        r.EditSelectIslands(radius, 100000)                        # everything alive, nothing dead
        assert np.array_equal(r.DownloadEditBits()[0], EM.pack_bits(alive, nw))
        r.SetDeletedBits(~np.zeros(nw, np.uint32))                 # nobody alive: no error, all ones and zeros, nothing selected
        r.EditDeselectAll()
        labels, sizes = r.EditComponents(radius)
        assert (labels == IM.NOT_ALIVE).all() and not sizes.any()
        r.EditSelectIslands(radius, 1000)
        r.EditGrowSelection(radius)
        assert not r.DownloadEditBits()[0].any()
    finally:
        r.DisposeResourcesForAsset()


# ---- 6. the words: min_size 0 and 1, N = 33, seeds in two components, an empty selection, the same call twice -------------------------------------------------
def test_words_at_33_the_quirk_bits_are_neither_seeds_nor_touched(gpu_ctx):
    pos, radius = NR.lattice(33)
    pos = pos.copy()
    pos[16:] += f32(4.0)                                           # two pieces: splats 0 .. 15 and 16 .. 32
    alive = np.ones(33, bool)
    r = point_renderer(gpu_ctx, pos)
    lib = _lib.lib()

    def upload(words):                                             # the C call itself
        _lib.check(lib.gs_renderer_edit_upload_selected_bits(r._r_h, words.ctypes.data, len(words)), "gs_renderer_edit_upload_selected_bits")

    try:
        labels, sizes = check_components(r, pos, alive, radius, "33")
        assert labels.tolist() == [0] * 16 + [16] * 17 and sizes.tolist() == [16] * 16 + [17] * 17
        for k in (0, 1):
            r.EditSelectIslands(radius, k)
            assert not r.DownloadEditBits()[0].any()
        r.EditSelectIslands(radius, 18)
        assert r.DownloadEditBits()[0].tolist() == [0xFFFFFFFF, 1] and r.editSelectedSplats == 33      # bits 33 .. 63 stay clear
        r.EditSelectAll()                                          # sets the tail bits: they survive a subtract, an add and a grow
        r.EditSelectIslands(radius, 17, subtract=True)
        assert r.DownloadEditBits()[0].tolist() == [0xFFFF0000, 0xFFFFFFFF]
        r.EditGrowSelection(radius)
        assert r.DownloadEditBits()[0].tolist() == [0xFFFF0000, 0xFFFFFFFF]
        tail = np.array([0, 0xFFFFFFFE], np.uint32)                # only bits at or beyond N: no seed, nothing grows
        upload(tail)
        r.EditGrowSelection(radius)
        assert r.DownloadEditBits()[0].tolist() == tail.tolist()
        r.EditSelectIslands(radius, 17)
        assert r.DownloadEditBits()[0].tolist() == [0x0000FFFF, 0xFFFFFFFE]
        # a single seed set through the C call; the same call twice; seeds in two components; an empty selection
        upload(np.array([1 << 25, 0], np.uint32))
        r.EditGrowSelection(radius)
        assert r.DownloadEditBits()[0].tolist() == [0xFFFF0000, 1]
        r.UpdateEditCountsAndBounds()
        assert r.editSelectedSplats == 17
        r.EditGrowSelection(radius)
        assert r.DownloadEditBits()[0].tolist() == [0xFFFF0000, 1]
        r.UploadSelectedBits(np.array([(1 << 25) | (1 << 3), 0], np.uint32))
        r.EditGrowSelection(radius)
        assert r.DownloadEditBits()[0].tolist() == [0xFFFFFFFF, 1]
        r.EditDeselectAll()
        r.EditGrowSelection(radius)
        assert not r.DownloadEditBits()[0].any() and r.editSelectedSplats == 0
        r.EditSelectIslands(radius, 17)
        first = r.DownloadEditBits()[0]
        r.EditSelectIslands(radius, 17)
        assert np.array_equal(r.DownloadEditBits()[0], first) and first.tolist() == [0x0000FFFF, 0]
        a, b = r.EditComponents(radius), r.EditComponents(radius)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(r.DownloadEditBits()[0], first)
    finally:
        r.DisposeResourcesForAsset()


def test_the_selecting_calls_make_the_edit_buffers(gpu_ctx):
    pos, radius, group = IM.clumps(8, 3)
    lib = _lib.lib()
    for call in ("islands", "grow"):
        r = point_renderer(gpu_ctx, pos)
        try:
            rc = lib.gs_renderer_edit_select_islands(r._r_h, C.c_float(radius), 4, 0) if call == "islands" else lib.gs_renderer_edit_grow_selection(r._r_h, C.c_float(radius))
            assert rc == 0
            r.m_GpuEditSelected = True
            assert EM.popcount(r.DownloadEditBits()[0]) == (6 if call == "islands" else 0)
        finally:
            r.DisposeResourcesForAsset()


# ---- 7. history and highlight ------------------------------------------------------------------------------------------------------------------------------------
def test_undo_and_redo_cover_both_selecting_calls(gpu_ctx):
    n = 700
    pos, radius = NR.gaussian(n, 11)
    alive = np.ones(n, bool)
    labels, sizes = IM.components(pos, alive, radius)
    r = point_renderer(gpu_ctx, pos)
    try:
        r.EditHistoryEnable(1 << 24)
        first = np.zeros(words_of(n), np.uint32)
        first[3] = 0x00F0F00F
        r.UploadSelectedBits(first)
        for call, want in ((lambda: r.EditSelectIslands(radius, 4), IM.select_islands(first, sizes, alive, 4)),
                           (lambda: r.EditGrowSelection(radius), IM.grow_selection(first, labels, alive))):
            with r.EditGesture():
                call()
            new = r.DownloadEditBits()[0]
            assert np.array_equal(new, want) and not np.array_equal(new, first)
            info = r.EditHistoryInfo()
            assert (info.undo_depth, info.redo_depth) == (1, 0)
            r.EditUndo()
            assert np.array_equal(r.DownloadEditBits()[0], first)
            assert (r.EditHistoryInfo().undo_depth, r.EditHistoryInfo().redo_depth) == (0, 1)
            r.EditRedo()
            assert np.array_equal(r.DownloadEditBits()[0], new)
            r.EditUndo()
            call()                                                 # a selection change: the redo side goes
            assert r.EditHistoryInfo().redo_depth == 0
            r.UploadSelectedBits(first)
            r.EditHistoryEnable(0)
            r.EditHistoryEnable(1 << 24)
    finally:
        r.DisposeResourcesForAsset()


def highlighted(ctx, asset):
    r = GaussianSplatRenderer(ctx, asset)
    r.sortMode = SortMode.Visible
    r.selectionHighlight = True                                    # applied when the native renderer is made
    r.OnEnable()
    r.SetTileShape(16, 16)
    return r


def test_two_frames_in_flight_show_the_new_selection(gpu_ctx):
    a = small_asset(3000, 5, "Medium")
    cams = [default_camera(W=160, H=100, az=25.0 + 40.0 * k) for k in range(3)]
    lanes, one = highlighted(gpu_ctx, a), highlighted(gpu_ctx, a)
    lanes.SetFramesInFlight(2)
    assert lanes.FramesInFlight() == (2, True)
    targets = [RenderTarget(gpu_ctx, 160, 100) for _ in range(3)]
    rt = RenderTarget(gpu_ctx, 160, 100)
    pos = np.ascontiguousarray(decode_of(3000, "Medium")[:, :3], f32)
    alive = np.ones(3000, bool)
    labels, sizes = IM.components(pos, alive, 0.3)
    try:
        def frame(r, cam, t):
            r.SortPoints(cam); r.CalcViewData(cam); t.Clear(); r.Draw(cam, t)

        def edit(r):
            r.EditSelectIslands(0.3, 6)
            r.EditSelectIslands(0.3, 2, subtract=True)
            r.EditGrowSelection(0.45)

        frame(lanes, cams[0], targets[0])                          # a frame in flight with nothing selected
        edit(lanes)
        for k in (1, 2):
            frame(lanes, cams[k], targets[k])
        got = [t.Download() for t in targets]
        words = lanes.DownloadEditBits()[0]
        zero = np.zeros(len(words), np.uint32)
        want = IM.select_islands(IM.select_islands(zero, sizes, alive, 6), sizes, alive, 2, subtract=True)
        want = IM.grow_selection(want, IM.components(pos, alive, 0.45)[0], alive)
        assert np.array_equal(words, want) and 50 < EM.popcount(words) < 2950
        plain = []
        for k in range(3):
            if k == 1:
                edit(one)
            frame(one, cams[k], rt)
            plain.append(rt.Download())
            assert np.array_equal(got[k], plain[k]), (k, int((got[k] != plain[k]).any(axis=-1).sum()))
        one.EditDeselectAll()
        frame(one, cams[1], rt)
        assert not np.array_equal(rt.Download(), plain[1])         # the selection is what those frames show
    finally:
        for t in targets + [rt]:
            t.Dispose()
        lanes.OnDisable(); one.OnDisable()


# ---- 8. refusals: the words and the history counters untouched -----------------------------------------------------------------------------------------------------
def raw_components(lib, r, radius, labels, sizes, count) -> int:
    return lib.gs_renderer_edit_components(r._r_h if r is not None else None, C.c_float(radius), labels.ctypes.data if labels is not None else None,
                                           sizes.ctypes.data if sizes is not None else None, count)


def raw_islands(lib, r, radius, min_size, subtract=0) -> int:
    return lib.gs_renderer_edit_select_islands(r._r_h if r is not None else None, C.c_float(radius), min_size, subtract)


def raw_grow(lib, r, radius) -> int:
    return lib.gs_renderer_edit_grow_selection(r._r_h if r is not None else None, C.c_float(radius))


def test_refusals_change_nothing(gpu_ctx):
    n = 257
    pos, radius = NR.gaussian(n, 13)
    r = point_renderer(gpu_ctx, pos)
    lib = _lib.lib()
    try:
        r.EditHistoryEnable(1 << 24)
        first = np.zeros(words_of(n), np.uint32)
        first[2] = 0x0F0F0F0F
        r.UploadSelectedBits(first)
        r.EditCheckpoint()
        r.EditSelectAll()
        r.EditUndo()                                               # one entry on the redo side: any selection change would drop it
        before = bytes(r.EditHistoryInfo())
        words = r.DownloadEditBits()[0]
        la, si = np.full(n, 0x12345678, np.uint32), np.full(n, 0x12345678, np.uint32)
        for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -1.0, 0.9e-15, 1.1e15):
            assert NM.radius_refused(bad)
            assert raw_components(lib, r, bad, la, si, n) == BAD, bad
            assert raw_islands(lib, r, bad, 4) == BAD and raw_islands(lib, r, bad, 0) == BAD, bad
            assert raw_grow(lib, r, bad) == BAD, bad
        assert raw_components(lib, r, radius, la, si, n - 1) == BAD and raw_components(lib, r, radius, la, si, n + 1) == BAD
        assert raw_components(lib, r, radius, None, None, n) == BAD and raw_components(lib, None, radius, la, si, n) == BAD
        assert raw_islands(lib, None, radius, 4) == BAD and raw_grow(lib, None, radius) == BAD
        assert (la == 0x12345678).all() and (si == 0x12345678).all()
        assert np.array_equal(r.DownloadEditBits()[0], words) and bytes(r.EditHistoryInfo()) == before
        # the components change nothing either, either output alone is served, and the edges of the radius range are accepted
        want = IM.components(pos, np.ones(n, bool), radius)
        assert raw_components(lib, r, radius, la, None, n) == 0 and np.array_equal(la, want[0]) and (si == 0x12345678).all()
        assert raw_components(lib, r, radius, None, si, n) == 0 and np.array_equal(si, want[1])
        for ok in (1.0e-15, 1.0e15, radius):
            assert not NM.radius_refused(ok)
            r.EditComponents(ok)
        assert np.array_equal(r.DownloadEditBits()[0], words) and bytes(r.EditHistoryInfo()) == before
    finally:
        r.DisposeResourcesForAsset()


def test_a_renderer_with_lanes_is_served_and_refuses_the_same(gpu_ctx):
    """(a lane's own handle never reaches the host: its refusal cannot be provoked through the ABI)"""
    a = small_asset(300, 5, "Medium")
    r = highlighted(gpu_ctx, a)
    r.SetFramesInFlight(2)
    try:
        with pytest.raises(GsError):
            r.EditComponents(float("nan"))
        pos = np.ascontiguousarray(decode_of(300, "Medium")[:, :3], f32)
        check_components(r, pos, np.ones(300, bool), 0.4, "lanes")
    finally:
        r.OnDisable()
