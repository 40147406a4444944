"""-m gpu: gs_renderer_edit_neighbour_counts and gs_renderer_edit_select_sparse against the numpy twin of tests/neighbour_model.py (brute force where it
is quick, the grid model -- held to brute force by tests/test_neighbour_model.py -- above that).  Exact integers and exact words: no tolerance."""
import numpy as np
import pytest

import edit_model as EM
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


def check_counts(r, pos, alive, radius, what, caps=(65535,)):
    """the call against the twin at every cap; returns the twin's uncapped counts"""
    alive = np.asarray(alive, bool)
    counts = NM.brute_counts(pos, alive, radius) if int(alive.sum()) <= 5000 else NM.grid_counts(pos, alive, radius)
    for cap in caps:
        got = r.EditNeighbourCounts(radius, cap)
        want = NM.counts_words(counts, alive, cap)
        assert np.array_equal(got, want), (what, radius, cap, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    return counts


def check_select(r, counts, alive, radius, what, ks=(0, 1, 4)):
    """add with every k on an empty selection, then subtract a smaller k from everything sparse at a larger one; the words equal the twin's"""
    n = len(counts)
    nw = (n + 31) // 32
    for k in ks:
        r.EditDeselectAll()
        r.EditSelectSparse(radius, k)
        want = NM.select_sparse(np.zeros(nw, np.uint32), counts, alive, k)
        got = r.DownloadEditBits()[0]
        assert np.array_equal(got, want), (what, "add", k, np.flatnonzero(got != want)[:8])
    big = max(ks) + 3
    r.EditDeselectAll()
    r.EditSelectSparse(radius, big)
    r.EditSelectSparse(radius, 1, subtract=True)
    want = NM.select_sparse(NM.select_sparse(np.zeros(nw, np.uint32), counts, alive, big), counts, alive, 1, subtract=True)
    assert np.array_equal(r.DownloadEditBits()[0], want), (what, "subtract")
    r.EditDeselectAll()


# ---- 1. sizes: the sort's small-partition edge, several partitions; a radius that isolates everything, one that makes a single cell -------------------
@pytest.mark.parametrize("n", [1, 2, 33, 255, 256, 257, 4095, 4097, 20000])
def test_sizes_with_isolating_typical_and_one_cell_radii(gpu_ctx, n):
    pos, radius = NR.gaussian(n, 100 + n)
    alive = np.ones(n, bool)
    r = point_renderer(gpu_ctx, pos)
    try:
        lonely = check_counts(r, pos, alive, NR.isolating_radius(pos), (n, "isolating"))
        assert not lonely.any()
        counts = check_counts(r, pos, alive, radius, (n, "typical"), caps=(65535, 3))
        if n >= 255:
            assert 4 <= np.median(counts) and counts.min() <= 1 < counts.max()
        check_select(r, counts, alive, radius, (n, "typical"))
        if n <= 4097:
            all_of_them = check_counts(r, pos, alive, NR.one_cell_radius(pos), (n, "one cell"), caps=(65535, 7))
            assert np.array_equal(all_of_them, np.full(n, n - 1))
    finally:
        r.DisposeResourcesForAsset()


def test_look_back_across_partitions_at_70001(gpu_ctx):
    n = 70001
    pos, radius = NR.gaussian(n, 7)
    r = point_renderer(gpu_ctx, pos)
    try:
        counts = check_counts(r, pos, np.ones(n, bool), radius, "70001")
        assert counts.max() > 16 and (counts == 0).any()
        r.EditSelectSparse(radius, 4)
        assert np.array_equal(r.DownloadEditBits()[0], NM.select_sparse(np.zeros((n + 31) // 32, np.uint32), counts, np.ones(n, bool), 4))
    finally:
        r.DisposeResourcesForAsset()


# ---- 2. the adversarial families: the exact-radius lattice, the far clouds, ulp pairs, the clamp, duplicates ---------------------------------------------
@pytest.mark.parametrize("family", range(8))
def test_adversarial_families(gpu_ctx, family):
    name, pos, radius = NR.adversarial(1500, 3)[family]
    alive = np.ones(len(pos), bool)
    r = point_renderer(gpu_ctx, pos)
    try:
        counts = check_counts(r, pos, alive, radius, name, caps=(65535, 1))
        check_select(r, counts, alive, radius, name, ks=(1, 4))
    finally:
        r.DisposeResourcesForAsset()


def test_an_identical_cloud_counts_n_minus_one_and_saturates_at_the_cap(gpu_ctx):
    pos, radius = NR.identical(300)
    r = point_renderer(gpu_ctx, pos)
    try:
        for rad in (radius, 1.0e-15, 1.0e15):
            counts = check_counts(r, pos, np.ones(300, bool), rad, "identical", caps=(1, 7, 65535))
            assert np.array_equal(counts, np.full(300, 299))
        for cap, want in ((1, 1), (7, 7), (65535, 299)):
            assert np.array_equal(r.EditNeighbourCounts(radius, cap), np.full(300, want, np.uint32))
    finally:
        r.DisposeResourcesForAsset()


def test_non_finite_positions_are_nobodys_neighbours_and_sparse(gpu_ctx):
    pos, radius = NR.non_finite(257, 4)
    bad = ~np.isfinite(pos).all(axis=1)
    assert bad.sum() == 7
    alive = np.ones(257, bool)
    r = point_renderer(gpu_ctx, pos)
    try:
        counts = check_counts(r, pos, alive, NR.one_cell_radius(pos[~bad]), "non-finite")
        assert np.array_equal(counts[~bad], np.full(250, 249)) and not counts[bad].any()
        r.EditSelectSparse(radius, 0)
        assert not r.DownloadEditBits()[0].any()
        r.EditSelectSparse(NR.one_cell_radius(pos[~bad]), 1)
        assert np.array_equal(r.DownloadEditBits()[0], EM.pack_bits(bad, 9))
    finally:
        r.DisposeResourcesForAsset()


# ---- 3. sources: every preset's decode, and the private pos blob a translate made ---------------------------------------------------------------------------
@pytest.mark.parametrize("quality", PRESETS)
def test_every_preset_as_the_source(gpu_ctx, quality):
    # (a Cluster* SH table needs more splats than entries: those two presets at the 20,000 whose decode tests/test_gpu_copy.py shares)
    n, radius = (20000, 0.12) if quality in ("VeryLow", "Low") else (700, 0.35)
    pos = np.ascontiguousarray(decode_of(n, quality)[:, :3], f32)
    r = pinned_renderer(gpu_ctx, small_asset(n, 5, quality))
    try:
        counts = check_counts(r, pos, np.ones(n, bool), radius, quality)
        assert counts.max() >= 4 and counts.min() <= 2
        check_select(r, counts, np.ones(n, bool), radius, quality, ks=(3,))
    finally:
        r.DisposeResourcesForAsset()


def test_a_translated_selection_is_read_from_the_private_pos_blob(gpu_ctx):
    n = 700
    pos, radius = NR.gaussian(n, 9)
    r = point_renderer(gpu_ctx, pos)
    try:
        before = check_counts(r, pos, np.ones(n, bool), radius, "before")
        sel = np.zeros(n, bool)
        sel[::2] = True
        r.UploadSelectedBits(EM.pack_bits(sel, (n + 31) // 32))
        r.EditStorePosMouseDown()
        r.EditTranslateSelection((5.0, 0.25, -0.125))
        moved = np.frombuffer(r.DownloadPosOther()[0].tobytes(), f32)[:3 * n].reshape(n, 3)
        assert np.array_equal(moved[~sel], pos[~sel]) and not np.array_equal(moved[sel], pos[sel])
        after = check_counts(r, moved, np.ones(n, bool), radius, "after")
        assert not np.array_equal(after, before)
    finally:
        r.DisposeResourcesForAsset()


# ---- 4. dead splats: deleted bits and cutouts -----------------------------------------------------------------------------------------------------------------
def test_dead_splats_get_all_ones_are_nobodys_neighbours_and_are_never_selected(gpu_ctx):
    n = 700
    asset = small_asset(n, 5, "Medium")
    m = EM.EditModel(asset)
    r = pinned_renderer(gpu_ctx, asset)
    nw = (n + 31) // 32
    deleted = np.random.default_rng(5).random(n) < 0.3
    cuts = [GaussianCutout(Type.Ellipsoid, False, camera.Transform(position=(0.4, -0.2, 0.3), scale=(2.2, 1.6, 2.0)))]
    try:
        everyone = check_counts(r, m.pos, np.ones(n, bool), 0.35, "all alive")
        r.SetDeletedBits(EM.pack_bits(deleted, nw))
        r.m_Cutouts = cuts
        m.set_cutouts(cuts, r.transform.localToWorldMatrix)
        alive = NM.alive_flags(n, EM.pack_bits(deleted, nw), m.cut)
        assert 100 < alive.sum() < n - 100 and (m.cut & ~deleted).sum() > 50
        counts = check_counts(r, m.pos, alive, 0.35, "deleted + cut")
        assert (counts[alive] < everyone[alive]).any()
        check_select(r, counts, alive, 0.35, "deleted + cut", ks=(2,))
        r.EditSelectSparse(0.35, 1000)                             # everything alive, nothing dead
        assert np.array_equal(r.DownloadEditBits()[0], EM.pack_bits(alive, nw))
        r.SetDeletedBits(~np.zeros(nw, np.uint32))                 # nobody alive: no error, all ones, nothing selected
        r.EditDeselectAll()
        assert np.array_equal(r.EditNeighbourCounts(0.35), np.full(n, NM.NOT_ALIVE, np.uint32))
        r.EditSelectSparse(0.35, 1000)
        assert not r.DownloadEditBits()[0].any()
    finally:
        r.DisposeResourcesForAsset()


# ---- 5. select_sparse: the words, N = 33, the counts and bounds that follow --------------------------------------------------------------------------------
def test_select_sparse_at_33_leaves_the_tail_bits_clear_and_edit_info_follows(gpu_ctx):
    pos, radius = NR.lattice(33)
    asset = fp32_point_asset(pos)
    m = EM.EditModel(asset)
    r = pinned_renderer(gpu_ctx, asset)
    alive = np.ones(33, bool)
    try:
        counts = check_counts(r, pos, alive, radius, "33")
        assert sorted(set(counts.tolist())) == [1, 3, 4, 5]
        for k in (0, 1, 4, 100):
            r.EditDeselectAll()
            r.EditSelectSparse(radius, k)
            words = r.DownloadEditBits()[0]
            assert np.array_equal(words, NM.select_sparse(np.zeros(2, np.uint32), counts, alive, k)), k
            assert words[1] <= 1                                   # bits 33 .. 63 stay clear (select-all sets them; this tool has no such quirk)
            m.upload_selected(words)
            assert np.array_equal(EM.info_words(edit_info(r)), m.info()), k
            assert r.editSelectedSplats == int((counts < k).sum())
        r.EditSelectAll()                                          # on the current selection: the tail bits select-all set survive an add and a subtract
        r.EditSelectSparse(radius, 4, subtract=True)
        want = NM.select_sparse(~np.zeros(2, np.uint32), counts, alive, 4, subtract=True)
        assert np.array_equal(r.DownloadEditBits()[0], want) and want[1] == 0xFFFFFFFE | int(counts[32] >= 4)
    finally:
        r.DisposeResourcesForAsset()


# ---- 6. history and highlight ------------------------------------------------------------------------------------------------------------------------------------
def test_undo_and_redo_cover_a_sparse_selection(gpu_ctx):
    n = 700
    pos, radius = NR.gaussian(n, 11)
    r = point_renderer(gpu_ctx, pos)
    try:
        r.EditHistoryEnable(1 << 24)
        first = np.zeros((n + 31) // 32, np.uint32)
        first[3] = 0x00F0F00F
        r.UploadSelectedBits(first)
        with r.EditGesture():
            r.EditSelectSparse(radius, 4)
        new = r.DownloadEditBits()[0]
        counts = NM.brute_counts(pos, np.ones(n, bool), radius)
        assert np.array_equal(new, NM.select_sparse(first, counts, np.ones(n, bool), 4)) and not np.array_equal(new, first)
        info = r.EditHistoryInfo()
        assert (info.undo_depth, info.redo_depth) == (1, 0)
        r.EditUndo()
        assert np.array_equal(r.DownloadEditBits()[0], first)
        assert (r.EditHistoryInfo().undo_depth, r.EditHistoryInfo().redo_depth) == (0, 1)
        r.EditRedo()
        assert np.array_equal(r.DownloadEditBits()[0], new)
        r.EditUndo()
        r.EditSelectSparse(radius, 2)                              # a selection change: the redo side goes
        assert r.EditHistoryInfo().redo_depth == 0
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
    try:
        def frame(r, cam, t):
            r.SortPoints(cam); r.CalcViewData(cam); t.Clear(); r.Draw(cam, t)
        frame(lanes, cams[0], targets[0])                          # a frame in flight with nothing selected
        lanes.EditSelectSparse(0.3, 6)
        for k in (1, 2):
            frame(lanes, cams[k], targets[k])
        got = [t.Download() for t in targets]
        words = lanes.DownloadEditBits()[0]
        pos = np.ascontiguousarray(decode_of(3000, "Medium")[:, :3], f32)
        want = NM.select_sparse(np.zeros(len(words), np.uint32), NM.brute_counts(pos, np.ones(3000, bool), 0.3), np.ones(3000, bool), 6)
        assert np.array_equal(words, want) and 50 < EM.popcount(words) < 2950
        plain = []
        for k in range(3):
            if k == 1:
                one.EditSelectSparse(0.3, 6)
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


# ---- 7. refusals: the words and the history counters untouched -----------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_ctx):
    n = 257
    pos, radius = NR.gaussian(n, 13)
    r = point_renderer(gpu_ctx, pos)
    lib = _lib.lib()
    try:
        r.EditHistoryEnable(1 << 24)
        first = np.zeros((n + 31) // 32, np.uint32)
        first[2] = 0x0F0F0F0F
        r.UploadSelectedBits(first)
        r.EditCheckpoint()
        r.EditSelectAll()
        r.EditUndo()                                               # one entry on the redo side: any selection change would drop it
        before = bytes(r.EditHistoryInfo())
        words = r.DownloadEditBits()[0]
        out = np.full(n, 0x12345678, np.uint32)
        for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -1.0, 0.9e-15, 1.1e15):
            assert NM.radius_refused(bad)
            assert NR.raw_counts(lib, r, bad, 65535, out, n) == BAD, bad
            assert NR.raw_select(lib, r, bad, 4) == BAD, bad
        assert NR.raw_counts(lib, r, radius, 0, out, n) == BAD                     # cap == 0
        assert NR.raw_counts(lib, r, radius, 65535, out, n - 1) == BAD and NR.raw_counts(lib, r, radius, 65535, out, n + 1) == BAD
        assert NR.raw_counts(lib, r, radius, 65535, None, n) == BAD and NR.raw_counts(lib, None, radius, 65535, out, n) == BAD
        assert NR.raw_select(lib, None, radius, 4) == BAD
        assert (out == 0x12345678).all()
        assert np.array_equal(r.DownloadEditBits()[0], words) and bytes(r.EditHistoryInfo()) == before
        # the counts change nothing either, and the edges of the radius range are accepted
        for ok in (1.0e-15, 1.0e15, radius):
            assert not NM.radius_refused(ok)
            r.EditNeighbourCounts(ok)
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
            r.EditNeighbourCounts(float("nan"))
        counts = r.EditNeighbourCounts(0.4)
        assert np.array_equal(counts, NM.counts_words(NM.brute_counts(np.ascontiguousarray(decode_of(300, "Medium")[:, :3], f32), np.ones(300, bool), 0.4),
                                                      np.ones(300, bool), 65535))
    finally:
        r.OnDisable()
