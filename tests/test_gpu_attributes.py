"""-m gpu: the attribute tools -- gs_renderer_edit_attribute_values / _select_range / _attribute_stats / _attribute_histogram / _attribute_ranks -- against
the numpy twin of tests/attribute_model.py.  Exact bits, exact integers and exact words: no tolerance (a NaN value equals any NaN: its sign and
payload carry no meaning)."""
import ctypes as C

import numpy as np
import pytest

import attribute_model as AM
import attribute_rig as AR
import copy_model as CM
import edit_model as EM
import neighbour_model as NM
from builders import decode_of
from common import PRESETS, default_camera, small_asset
from gpu_rig import BAD, edit_info, pinned_renderer
from unitygaussiansplatting_amd import _abi, _lib, asset as A, camera
from unitygaussiansplatting_amd.cutout import GaussianCutout, Type
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
f32 = np.float32
P = AR.POINT


def field_renderer(ctx, fields):
    return pinned_renderer(ctx, AR.attribute_asset(*fields))


def bounds_of(v, alive):
    """a range for the histogram and the selections from the twin's own values: the 10 % and 90 % order statistics of the alive numbers (lo < hi), or
    the family's fixed range where they do not make one"""
    k = AM.population_keys(v, alive & np.isfinite(v))
    if len(k) >= 2:
        lo, hi = AM.key_values(k[[len(k) // 10, (9 * len(k)) // 10]])
        if AM.hist_scale(lo, hi, 64) is not None:
            return float(lo), float(hi)
    return AR.HIST_LO, AR.HIST_HI


def check_attr(r, dec, alive, attr, what, bins_list=(64,), sel_words=None, lohi=None):
    """every call of one attribute against the twin; the selection is left as it was found (sel_words, or empty)"""
    n = len(dec)
    nw = (n + 31) // 32
    v = AM.values(dec, attr, P)
    tag = (what, attr)
    got = r.EditAttributeValues(attr, P).view(np.uint32)
    want = AM.value_words(v, alive)
    same = AM.same_words(got, want)
    assert same.all(), (tag, "values", np.flatnonzero(~same)[:8], got[~same][:8], want[~same][:8])
    lo, hi = lohi if lohi is not None else bounds_of(v, alive)
    for selected_only in ((False, True) if sel_words is not None else (False,)):
        members = AM.scope_flags(alive, sel_words, selected_only)
        assert AR.stats_tuple(r.EditAttributeStats(attr, selected_only, P)) == AM.stats(v, members), (tag, "stats", selected_only)
        for bins in bins_list:
            h, below, above, nans = r.EditAttributeHistogram(attr, lo, hi, bins, selected_only, P)
            wh = AM.histogram(v, members, lo, hi, bins)
            assert np.array_equal(np.concatenate([h, [below, above, nans]]).astype(np.uint32), wh), (tag, "histogram", bins, selected_only, lo, hi)
            assert int(h.sum()) + below + above + nans == int(members.sum())
        pop = len(AM.population_keys(v, members))
        rk = [0, pop // 2, max(pop - 1, 0), pop]
        vals, gp = r.EditAttributeRanks(attr, rk, selected_only, P)
        ww, wp = AM.ranks(v, members, rk)
        assert gp == wp == pop and np.array_equal(vals.view(np.uint32), ww), (tag, "ranks", selected_only, vals.view(np.uint32), ww)
        assert r.EditAttributeRanks(attr, [], selected_only, P)[1] == pop
    # a range select: add on what is selected, then subtract the upper half of the range
    first = np.zeros(nw, np.uint32) if sel_words is None else np.ascontiguousarray(sel_words, np.uint32)
    if sel_words is None:
        r.EditDeselectAll()
    mid = f32(lo) + (f32(hi) - f32(lo)) * f32(0.5)
    r.EditSelectRange(attr, lo, hi, point=P)
    added = AM.select_range(first, v, alive, lo, hi)
    words = r.DownloadEditBits()[0]
    assert np.array_equal(words, added), (tag, "add", lo, hi, np.flatnonzero(words != added)[:8])
    r.EditSelectRange(attr, mid, np.inf, subtract=True, point=P)
    taken = AM.select_range(added, v, alive, mid, np.inf, subtract=True)
    words = r.DownloadEditBits()[0]
    assert np.array_equal(words, taken), (tag, "subtract", np.flatnonzero(words != taken)[:8])
    if sel_words is None:
        r.EditDeselectAll()
    else:
        r.UploadSelectedBits(first)
    return v


# ---- 1. sizes: one chunk and less, the chunk edge, the sort's small-partition edge, several workgroups ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 33, 255, 256, 257, 4095, 4097, 20000])
def test_sizes_every_attribute(gpu_ctx, n):
    fields = AR.plain(n, 200 + n)
    dec = AR.fields_of(*fields)
    r = field_renderer(gpu_ctx, fields)
    try:
        for attr in AM.ATTRS:
            check_attr(r, dec, np.ones(n, bool), attr, n)
    finally:
        r.DisposeResourcesForAsset()


def test_ranks_sort_across_partitions_at_70001(gpu_ctx):
    n = 70001
    fields = AR.plain(n, 7)
    dec = AR.fields_of(*fields)
    r = field_renderer(gpu_ctx, fields)
    try:
        for attr in (AM.OPACITY, AM.VOLUME, AM.POS_Y):             # opacity: long runs of equal keys at 0 and 1
            v = AM.values(dec, attr, P)
            rk = np.unique(np.concatenate([np.linspace(0, n - 1, 4000).astype(np.int64), [0, 1, n - 2, n - 1, n, n + 7]]))
            vals, pop = r.EditAttributeRanks(attr, rk, point=P)
            ww, wp = AM.ranks(v, np.ones(n, bool), rk)
            assert pop == wp == n and np.array_equal(vals.view(np.uint32), ww), (attr, np.flatnonzero(vals.view(np.uint32) != ww)[:8])
        q, pop = r.EditAttributeQuantiles(AM.VOLUME, [0.0, 0.25, 0.5, 0.999, 1.0])
        v = AM.values(dec, AM.VOLUME)
        assert np.array_equal(q.view(np.uint32), AM.ranks(v, np.ones(n, bool), AM.quantile_ranks([0.0, 0.25, 0.5, 0.999, 1.0], n))[0])
    finally:
        r.DisposeResourcesForAsset()


# ---- 2. sources: every preset's decode (the chunk tail, BC7 colour, Cluster* other records), all four classes ----------------------------------------------
@pytest.mark.parametrize("quality", PRESETS + ["Medium+BC7"])
def test_every_preset_as_the_source(gpu_ctx, quality):
    # (a Cluster* SH table needs more splats than entries: those two presets at the 20,000 whose decode tests/test_gpu_copy.py shares)
    if quality == "Medium+BC7":
        asset = small_asset(700, 5, "Medium", formatColor=A.ColorFormat.BC7)
        dec = CM.decode(asset)
    else:
        n = 20000 if quality in ("VeryLow", "Low") else 700
        asset, dec = small_asset(n, 5, quality), decode_of(n, quality)
    n = asset.splatCount
    r = pinned_renderer(gpu_ctx, asset)
    try:
        for attr in AM.ATTRS:
            v = check_attr(r, dec, np.ones(n, bool), attr, quality)
            assert len(np.unique(v.view(np.uint32))) > 8
    finally:
        r.DisposeResourcesForAsset()


# ---- 3. the adversarial family: NaN, +-inf, +-0, denormals, products that under- and overflow, values either side of every bin edge ---------------------------
@pytest.mark.parametrize("attr", AM.ATTRS)
def test_adversarial_family(gpu_ctx, attr):
    fields = AR.adversarial(1500)
    dec = AR.fields_of(*fields)
    r = field_renderer(gpu_ctx, fields)
    try:
        check_attr(r, dec, np.ones(1500, bool), attr, "adversarial", bins_list=AR.FAMILY_BINS, lohi=(AR.HIST_LO, AR.HIST_HI))
        v = AM.values(dec, attr, P)
        nw = (1500 + 31) // 32
        for lo, hi in ((-np.inf, np.inf), (-0.0, 0.0), (np.inf, np.inf), (-1e-40, 1e-40)):
            r.EditDeselectAll()
            r.EditSelectRange(attr, lo, hi, point=P)
            assert np.array_equal(r.DownloadEditBits()[0], AM.select_range(np.zeros(nw, np.uint32), v, np.ones(1500, bool), lo, hi)), (attr, lo, hi)
    finally:
        r.DisposeResourcesForAsset()


# ---- 4. contention: every value equal, one bin takes all 20,000 --------------------------------------------------------------------------------------------
def test_all_equal_values_count_exactly(gpu_ctx):
    n = 20000
    fields = AR.all_equal(n)
    dec = AR.fields_of(*fields)
    r = field_renderer(gpu_ctx, fields)
    try:
        for attr in AM.ONE_PER_CLASS:
            v = AM.values(dec, attr, P)
            assert len(np.unique(v)) == 1
            for bins in (1, 64, 4096):
                for lo, hi in ((0.0, 1.0), (float(v[0]), float(v[0]) + 1.0), (float(v[0]) - 1.0, float(v[0]))):
                    h, below, above, nans = r.EditAttributeHistogram(attr, lo, hi, bins, point=P)
                    wh = AM.histogram(v, np.ones(n, bool), lo, hi, bins)
                    assert np.array_equal(np.concatenate([h, [below, above, nans]]).astype(np.uint32), wh) and int(wh.max()) == n, (attr, bins, lo, hi)
            s = r.EditAttributeStats(attr, point=P)
            assert (s.members, s.nans) == (n, 0) and f32(s.vmin) == f32(s.vmax) == v[0]
            vals, pop = r.EditAttributeRanks(attr, [0, n - 1, n], point=P)
            assert pop == n and np.array_equal(vals.view(np.uint32), AM.ranks(v, np.ones(n, bool), [0, n - 1, n])[0])
    finally:
        r.DisposeResourcesForAsset()


# ---- 5. scope: deleted bits, cutouts and a selection ---------------------------------------------------------------------------------------------------------
def test_scopes_with_deleted_bits_cutouts_and_a_selection(gpu_ctx):
    n = 700
    asset = small_asset(n, 5, "Medium")
    dec = decode_of(n, "Medium")
    m = EM.EditModel(asset)
    r = pinned_renderer(gpu_ctx, asset)
    nw = (n + 31) // 32
    rng = np.random.default_rng(5)
    deleted = rng.random(n) < 0.3
    cuts = [GaussianCutout(Type.Ellipsoid, False, camera.Transform(position=(0.4, -0.2, 0.3), scale=(2.2, 1.6, 2.0)))]
    try:
        s = r.EditAttributeStats(AM.OPACITY, selectedOnly=True)    # no edit buffers yet: the selected scope is empty
        assert AR.stats_tuple(s) == AM.stats(AM.values(dec, AM.OPACITY), np.zeros(n, bool))
        assert r.EditAttributeRanks(AM.OPACITY, [0], selectedOnly=True)[1] == 0
        r.SetDeletedBits(EM.pack_bits(deleted, nw))
        r.m_Cutouts = cuts
        m.set_cutouts(cuts, r.transform.localToWorldMatrix)
        alive = NM.alive_flags(n, EM.pack_bits(deleted, nw), m.cut)
        assert 100 < alive.sum() < n - 100 and (m.cut & ~deleted).sum() > 50
        sel = EM.pack_bits(rng.random(n) < 0.5, nw)
        sel[-1] |= np.uint32(0xFFFFFFFF << (n % 32) & 0xFFFFFFFF)  # tail bits beyond N, as select-all leaves them
        r.UploadSelectedBits(sel)
        members = AM.scope_flags(alive, sel, True)
        assert 50 < members.sum() < alive.sum() - 50
        for attr in AM.ONE_PER_CLASS:
            check_attr(r, dec, alive, attr, "scope", sel_words=sel)
        r.SetDeletedBits(~np.zeros(nw, np.uint32))                 # nobody alive: no error
        assert (r.EditAttributeValues(AM.LUMA).view(np.uint32) == AM.NOT_ALIVE).all()
        assert AR.stats_tuple(r.EditAttributeStats(AM.LUMA)) == (0, 0, int(f32(np.inf).view(np.uint32)), int(f32(-np.inf).view(np.uint32)))
        assert not np.concatenate([r.EditAttributeHistogram(AM.LUMA, 0.0, 1.0, 8)[0]]).any() and r.EditAttributeRanks(AM.LUMA, [0])[1] == 0
        r.EditDeselectAll()
        r.EditSelectRange(AM.LUMA, -np.inf, np.inf)
        assert not r.DownloadEditBits()[0].any()
    finally:
        r.DisposeResourcesForAsset()


def test_select_all_on_33_counts_33_members(gpu_ctx):
    fields = AR.plain(33, 9)
    dec = AR.fields_of(*fields)
    r = field_renderer(gpu_ctx, fields)
    try:
        r.EditSelectAll()
        words = r.DownloadEditBits()[0]
        assert words.tolist() == [0xFFFFFFFF, 0xFFFFFFFF] and r.editSelectedSplats == 64      # the reference's quirk: the tail bits are set and counted
        for attr in AM.ONE_PER_CLASS:
            s = r.EditAttributeStats(attr, selectedOnly=True, point=P)
            assert AR.stats_tuple(s) == AM.stats(AM.values(dec, attr, P), np.ones(33, bool)) and s.members == 33
            h, below, above, nans = r.EditAttributeHistogram(attr, 0.0, 1.0, 4, selectedOnly=True, point=P)
            assert int(h.sum()) + below + above + nans == 33
            assert r.EditAttributeRanks(attr, [], selectedOnly=True, point=P)[1] == 33
    finally:
        r.DisposeResourcesForAsset()


# ---- 6. select range: the words, the tail, the buffers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 257])
def test_select_range_bounds_tail_bits_and_first_use(gpu_ctx, n):
    pos, scale, opacity, col = (x.copy() for x in AR.plain(n, 11))
    opacity[::5] = np.nan
    fields = (pos, scale, opacity, col)
    asset = AR.attribute_asset(*fields)
    dec = AR.fields_of(*fields)
    m = EM.EditModel(asset)
    r = pinned_renderer(gpu_ctx, asset)
    nw = (n + 31) // 32
    alive = np.ones(n, bool)
    v = AM.values(dec, AM.OPACITY)
    tail = np.uint32(0xFFFFFFFF << (n % 32) & 0xFFFFFFFF)
    try:
        assert not r.m_GpuEditSelected
        r.EditSelectRange(AM.OPACITY, 0.75, 0.25)                  # lo > hi: nothing selected, no error -- and the edit buffers are made on this first use
        assert r.m_GpuEditSelected and not r.DownloadEditBits()[0].any()
        r.EditSelectRange(AM.OPACITY, -np.inf, np.inf)             # every alive splat whose value is not NaN
        words = r.DownloadEditBits()[0]
        assert np.array_equal(words, AM.pack_bits(~np.isnan(v), nw)) and not (words[-1] & tail)
        m.upload_selected(words)
        assert np.array_equal(EM.info_words(edit_info(r)), m.info())
        assert r.editSelectedSplats == int((~np.isnan(v)).sum())
        for attr in AM.ONE_PER_CLASS:                              # no bit at or beyond N from any class
            r.EditDeselectAll()
            r.EditSelectRange(attr, -np.inf, np.inf, point=P)
            words = r.DownloadEditBits()[0]
            assert np.array_equal(words, AM.select_range(np.zeros(nw, np.uint32), AM.values(dec, attr, P), alive, -np.inf, np.inf)) and not (words[-1] & tail)
        r.EditSelectAll()                                          # the tail bits select-all set survive an add and a subtract
        r.EditSelectRange(AM.OPACITY, 0.25, 0.75, subtract=True)
        want = AM.select_range(~np.zeros(nw, np.uint32), v, alive, 0.25, 0.75, subtract=True)
        assert np.array_equal(r.DownloadEditBits()[0], want) and (want[-1] & tail) == tail
        r.EditSelectRange(AM.OPACITY, 0.0, 1.0)
        assert np.array_equal(r.DownloadEditBits()[0], AM.select_range(want, v, alive, 0.0, 1.0))
    finally:
        r.DisposeResourcesForAsset()


def test_select_top_takes_the_quantile_and_its_ties(gpu_ctx):
    n = 4097
    fields = AR.plain(n, 13)
    dec = AR.fields_of(*fields)
    r = field_renderer(gpu_ctx, fields)
    try:
        v = AM.values(dec, AM.OPACITY)                             # piled up at 0 and 1: ties at both thresholds
        for fraction, largest in ((0.1, True), (0.1, False), (0.5, True)):
            r.EditDeselectAll()
            r.EditSelectTop(AM.OPACITY, fraction, largest=largest)
            t = AM.ranks(v, np.ones(n, bool), AM.quantile_ranks([1.0 - fraction if largest else fraction], n))[0].view(f32)[0]
            want = AM.pack_bits((v >= t) if largest else (v <= t), (n + 31) // 32)
            assert np.array_equal(r.DownloadEditBits()[0], want), (fraction, largest)
            assert EM.popcount(want) >= int(fraction * n)
    finally:
        r.DisposeResourcesForAsset()


# ---- 7. with the rest of the edit path: history, highlight and lanes, a transform's private blob -------------------------------------------------------------
def test_undo_and_redo_cover_a_range_selection(gpu_ctx):
    n = 700
    fields = AR.plain(n, 15)
    dec = AR.fields_of(*fields)
    r = field_renderer(gpu_ctx, fields)
    try:
        r.EditHistoryEnable(1 << 24)
        first = np.zeros((n + 31) // 32, np.uint32)
        first[3] = 0x00F0F00F
        r.UploadSelectedBits(first)
        r.EditCheckpoint()
        r.EditSelectRange(AM.SCALE_MAX, 0.02, np.inf)
        new = r.DownloadEditBits()[0]
        assert np.array_equal(new, AM.select_range(first, AM.values(dec, AM.SCALE_MAX), np.ones(n, bool), 0.02, np.inf)) and not np.array_equal(new, first)
        info = r.EditHistoryInfo()
        assert (info.undo_depth, info.redo_depth) == (1, 0)
        r.EditUndo()
        assert np.array_equal(r.DownloadEditBits()[0], first)
        assert (r.EditHistoryInfo().undo_depth, r.EditHistoryInfo().redo_depth) == (0, 1)
        r.EditRedo()
        assert np.array_equal(r.DownloadEditBits()[0], new)
        r.EditUndo()
        r.EditSelectRange(AM.OPACITY, 0.0, 0.1)                    # a selection change: the redo side goes
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
        lanes.EditSelectRange(AM.OPACITY, 0.5, np.inf)
        for k in (1, 2):
            frame(lanes, cams[k], targets[k])
        got = [t.Download() for t in targets]
        words = lanes.DownloadEditBits()[0]
        v = AM.values(decode_of(3000, "Medium"), AM.OPACITY)
        want = AM.select_range(np.zeros(len(words), np.uint32), v, np.ones(3000, bool), 0.5, np.inf)
        assert np.array_equal(words, want) and 50 < EM.popcount(words) < 2950
        plain = []
        for k in range(3):
            if k == 1:
                one.EditSelectRange(AM.OPACITY, 0.5, np.inf)
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


def test_a_translated_selection_is_read_from_the_private_pos_blob(gpu_ctx):
    n = 700
    pos, scale, opacity, col = AR.plain(n, 17)
    r = field_renderer(gpu_ctx, (pos, scale, opacity, col))
    try:
        sel = np.zeros(n, bool)
        sel[::2] = True
        r.UploadSelectedBits(EM.pack_bits(sel, (n + 31) // 32))
        r.EditStorePosMouseDown()
        r.EditTranslateSelection((5.0, 0.25, -0.125))
        moved = np.frombuffer(r.DownloadPosOther()[0].tobytes(), f32)[:3 * n].reshape(n, 3)
        assert np.array_equal(moved[~sel], pos[~sel]) and not np.array_equal(moved[sel], pos[sel])
        dec = AR.fields_of(moved, scale, opacity, col)
        for attr in (AM.POS_X, AM.DIST2):
            got = r.EditAttributeValues(attr, P).view(np.uint32)
            assert np.array_equal(got, AM.values(dec, attr, P).view(np.uint32)), attr
        r.EditDeselectAll()
        r.EditSelectRange(AM.POS_X, 2.5, np.inf)
        assert np.array_equal(r.DownloadEditBits()[0], AM.select_range(np.zeros((n + 31) // 32, np.uint32), moved[:, 0], np.ones(n, bool), 2.5, np.inf))
    finally:
        r.DisposeResourcesForAsset()


# ---- 8. refusals: bits, buffers and the history untouched ------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_ctx):
    n = 257
    fields = AR.plain(n, 19)
    r = field_renderer(gpu_ctx, fields)
    fresh = field_renderer(gpu_ctx, fields)                        # never edited: a refused select_range must not make its edit buffers
    fresh.SetDeletedBits(np.array([0x1F] + [0] * ((n + 31) // 32 - 1), np.uint32))
    lib = _lib.lib()
    nan, inf = float("nan"), float("inf")
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
        info = bytes(edit_info(r))
        out = np.full(n, 0x12345678, np.uint32)
        hist = np.full(67, 0x12345678, np.uint32)
        ranks = np.array([0, 1], np.uint32)
        rout = np.full(2, 0x12345678, np.uint32)
        st = _abi.gs_attribute_stats(7, 7, 7.0, 7.0)
        pop = C.c_uint32(0x12345678)
        q = np.array(P, f32)
        for rr in (r, fresh):
            # a NULL renderer, a NULL required output
            assert AR.raw_values(lib, None, AM.OPACITY, None, out, n) == BAD and AR.raw_values(lib, rr, AM.OPACITY, None, None, n) == BAD
            assert AR.raw_select(lib, None, AM.OPACITY, None, 0.0, 1.0) == BAD
            assert AR.raw_stats(lib, None, AM.OPACITY, None, 0, st) == BAD and AR.raw_stats(lib, rr, AM.OPACITY, None, 0, None) == BAD
            assert AR.raw_histogram(lib, None, AM.OPACITY, None, 0, 0.0, 1.0, 64, hist, 67) == BAD and AR.raw_histogram(lib, rr, AM.OPACITY, None, 0, 0.0, 1.0, 64, None, 67) == BAD
            assert AR.raw_ranks(lib, None, AM.OPACITY, None, 0, ranks, 2, rout, pop) == BAD and AR.raw_ranks(lib, rr, AM.OPACITY, None, 0, ranks, 2, rout, None) == BAD
            assert AR.raw_ranks(lib, rr, AM.OPACITY, None, 0, None, 2, rout, pop) == BAD and AR.raw_ranks(lib, rr, AM.OPACITY, None, 0, ranks, 2, None, pop) == BAD
            # an unknown attribute or scope
            for attr in (-1, 12, 1000):
                assert AR.raw_values(lib, rr, attr, q, out, n) == BAD and AR.raw_select(lib, rr, attr, q, 0.0, 1.0) == BAD and AR.raw_stats(lib, rr, attr, q, 0, st) == BAD
                assert AR.raw_histogram(lib, rr, attr, q, 0, 0.0, 1.0, 64, hist, 67) == BAD and AR.raw_ranks(lib, rr, attr, q, 0, ranks, 2, rout, pop) == BAD
            for scope in (-1, 2):
                assert AR.raw_stats(lib, rr, AM.OPACITY, None, scope, st) == BAD and AR.raw_histogram(lib, rr, AM.OPACITY, None, scope, 0.0, 1.0, 64, hist, 67) == BAD
                assert AR.raw_ranks(lib, rr, AM.OPACITY, None, scope, ranks, 2, rout, pop) == BAD
            # a wrong count
            assert AR.raw_values(lib, rr, AM.OPACITY, None, out, n - 1) == BAD and AR.raw_values(lib, rr, AM.OPACITY, None, out, n + 1) == BAD
            assert AR.raw_histogram(lib, rr, AM.OPACITY, None, 0, 0.0, 1.0, 64, hist, 64) == BAD and AR.raw_histogram(lib, rr, AM.OPACITY, None, 0, 0.0, 1.0, 64, hist, 68) == BAD
            assert AR.raw_ranks(lib, rr, AM.OPACITY, None, 0, np.zeros(4097, np.uint32), 4097, np.zeros(4097, np.uint32), pop) == BAD
            # a NaN lo or hi; the histogram's own conditions
            for lo, hi in ((nan, 1.0), (0.0, nan), (nan, nan)):
                assert AR.raw_select(lib, rr, AM.OPACITY, None, lo, hi) == BAD and AR.raw_histogram(lib, rr, AM.OPACITY, None, 0, lo, hi, 64, hist, 67) == BAD
            for lo, hi, bins in ((0.0, 1.0, 0), (0.0, 1.0, 4097), (1.0, 1.0, 64), (2.0, 1.0, 64), (-inf, 1.0, 64), (0.0, inf, 64), (-3e38, 3e38, 64), (0.0, 1e-42, 64)):
                assert AM.hist_scale(lo, hi, bins) is None
                assert AR.raw_histogram(lib, rr, AM.OPACITY, None, 0, lo, hi, bins, np.zeros(bins + 3, np.uint32), bins + 3) == BAD, (lo, hi, bins)
            # GS_ATTR_DIST2: a NULL or non-finite point
            for point in (None, np.array([nan, 0, 0], f32), np.array([0, inf, 0], f32), np.array([0, 0, -inf], f32)):
                assert AR.raw_values(lib, rr, AM.DIST2, point, out, n) == BAD and AR.raw_select(lib, rr, AM.DIST2, point, 0.0, 1.0) == BAD
                assert AR.raw_stats(lib, rr, AM.DIST2, point, 0, st) == BAD and AR.raw_histogram(lib, rr, AM.DIST2, point, 0, 0.0, 1.0, 64, hist, 67) == BAD
                assert AR.raw_ranks(lib, rr, AM.DIST2, point, 0, ranks, 2, rout, pop) == BAD
        assert (out == 0x12345678).all() and (hist == 0x12345678).all() and (rout == 0x12345678).all() and pop.value == 0x12345678
        assert (st.members, st.nans, st.vmin, st.vmax) == (7, 7, 7.0, 7.0)
        assert np.array_equal(r.DownloadEditBits()[0], words) and bytes(r.EditHistoryInfo()) == before and bytes(edit_info(r)) == info
        # without edit buffers gs_renderer_edit_info reports nothing, the deleted splats included: the refusals made none, the first accepted call does
        assert bytes(edit_info(fresh)) == bytes(_abi.gs_edit_info())
        assert AR.raw_select(lib, fresh, AM.OPACITY, None, 0.75, 0.25) == 0 and edit_info(fresh).deleted == 5
        # the reading calls change nothing either; the point is ignored for the other attributes, NULL or not finite
        bad_point = np.array([nan, inf, 0], f32)
        assert AR.raw_values(lib, r, AM.OPACITY, bad_point, out, n) == 0 and AR.raw_stats(lib, r, AM.LUMA, None, 1, st) == 0
        assert AR.raw_histogram(lib, r, AM.VOLUME, bad_point, 1, 0.0, 1.0, 64, hist, 67) == 0 and AR.raw_ranks(lib, r, AM.POS_Z, None, 0, None, 0, None, pop) == 0
        assert pop.value == n and int(hist.sum()) == st.members == EM.popcount(words & AM.pack_bits(np.ones(n, bool), len(words)))
        assert np.array_equal(r.DownloadEditBits()[0], words) and bytes(r.EditHistoryInfo()) == before and bytes(edit_info(r)) == info
    finally:
        r.DisposeResourcesForAsset()
        fresh.DisposeResourcesForAsset()


def test_a_renderer_with_lanes_is_served(gpu_ctx):
    """(a lane's own handle never reaches the host: its refusal cannot be provoked through the ABI)"""
    a = small_asset(300, 5, "Medium")
    r = highlighted(gpu_ctx, a)
    r.SetFramesInFlight(2)
    try:
        dec = decode_of(300, "Medium")
        for attr in AM.ONE_PER_CLASS:
            check_attr(r, dec, np.ones(300, bool), attr, "lanes")
    finally:
        r.OnDisable()
