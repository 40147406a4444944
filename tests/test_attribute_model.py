"""CPU: the premises of the numpy twin of the attribute tools (tests/attribute_model.py) and of the adversarial family of tests/attribute_rig.py -- every
member of the family lands where the suites that use it say, the histogram words sum to the members, the ranks are a float64 sort wherever no +-0 tie
decides, and the key order is the total order the contract names."""
import numpy as np
import pytest

import attribute_model as AM
import attribute_rig as AR

f32 = np.float32


@pytest.fixture(scope="module")
def family():
    pos, scale, opacity, col = AR.adversarial()
    return AR.fields_of(pos, scale, opacity, col)


def test_the_key_is_a_total_order_with_minus_zero_before_plus_zero():
    v = np.array([-np.inf, -3e38, -1.0, -1e-40, -1.4e-45, -0.0, 0.0, 1.4e-45, 1e-40, 1.0, 3e38, np.inf], f32)
    k = AM.keys(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert int(k[6]) - int(k[5]) == 1                              # -0 and +0 are neighbours, -0 first
    assert np.array_equal(AM.key_values(k).view(np.uint32), v.view(np.uint32))
    nan = AM.keys(np.array([np.nan, -np.nan], f32))
    assert nan[0] > k[-1] and nan[1] < k[0]                        # a NaN's key lies outside the numbers': the tools never sort one


def test_fmax_and_fmin_ignore_nan_and_pin_the_zero_tie():
    a = np.array([1.0, np.nan, 2.0, np.nan, -0.0, 0.0, -1.0], f32)
    b = np.array([2.0, 3.0, np.nan, np.nan, 0.0, -0.0, -1.0], f32)
    mx, mn = AM.fmax(a, b), AM.fmin(a, b)
    assert np.array_equal(mx.view(np.uint32)[[0, 1, 2, 4, 5, 6]], np.array([2.0, 3.0, 2.0, -0.0, 0.0, -1.0], f32).view(np.uint32))
    assert np.array_equal(mn.view(np.uint32)[[0, 1, 2, 4, 5, 6]], np.array([1.0, 3.0, 2.0, -0.0, 0.0, -1.0], f32).view(np.uint32))
    assert np.isnan(mx[3]) and np.isnan(mn[3])
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal(4000).astype(f32), rng.standard_normal(4000).astype(f32)
    x[::7] = np.nan; y[::5] = np.nan
    for ours, theirs in ((AM.fmax, np.fmax), (AM.fmin, np.fmin)):  # np.fmax / np.fmin wherever no +-0 tie decides
        g, w = ours(x, y), theirs(x, y)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(g)], w[~np.isnan(w)])


def test_every_member_of_the_family_lands_where_stated(family):
    n = len(family)
    alive = np.ones(n, bool)
    for attr in AM.ATTRS:
        v = AM.values(family, attr, AR.POINT)
        assert v.dtype == f32 and len(v) == n
        for bins in AR.FAMILY_BINS:
            h = AM.histogram(v, alive, AR.HIST_LO, AR.HIST_HI, bins)
            assert len(h) == bins + 3 and int(h.sum()) == n, (attr, bins)
            assert h[bins] > 0 and h[bins + 1] > 0 and h[bins + 2] > 0, (attr, bins, h[bins:])      # below, above and NaN are each non-zero
        members, nans, vmin, vmax = AM.stats(v, alive)
        assert members == n and 0 < nans < n
        if attr == AM.DIST2:                                       # a sum of squares: never negative, never -inf
            assert vmin == 0 or not (vmin >> 31)
        assert vmax == int(f32(np.inf).view(np.uint32))
    # the opacity column holds every edge value, lo and hi themselves among them, and they fall in the first and the last bin
    o = AM.values(family, AM.OPACITY)
    edges = AR.bin_edge_values()
    assert set(edges.view(np.uint32).tolist()) <= set(o.view(np.uint32).tolist())
    for bins in AR.FAMILY_BINS:
        b = AM.bin_of(np.array([AR.HIST_LO, AR.HIST_HI], f32), AR.HIST_LO, AR.HIST_HI, bins)
        assert b.tolist() == [0, bins - 1]
        around = AM.bin_of(edges, AR.HIST_LO, AR.HIST_HI, bins)
        assert (around == bins).any() and (around == bins + 1).any() and len(set(around.tolist())) >= min(bins, 4)
    # under- and overflowing products, and the +-0 scale triples
    vol = AM.values(family, AM.VOLUME)
    assert (vol == 0).any() and np.isinf(vol).any() and (np.abs(vol[np.isfinite(vol) & (vol != 0)]) < 1.2e-38).any()
    mx = AM.values(family, AM.SCALE_MAX).view(np.uint32)
    assert mx[0] == 0x7FC00000 or np.isnan(mx[:1].view(f32))[0]
    assert mx[1] == 0 and mx[2] == 0x80000000 and mx[3] == 0x80000000
    assert mx[4] == f32(2.0).view(np.uint32) and mx[5] == f32(3.0).view(np.uint32) and mx[6] == f32(-1.0).view(np.uint32)


def test_a_rounded_sum_differs_from_a_fused_one_somewhere_in_the_family(family):
    """what `nothing fused` decides: luma and d2 computed in float64 and rounded once differ from the contract's fp32 bits for some splats"""
    for attr, wide in ((AM.LUMA, lambda d: 0.299 * d[:, 11].astype(np.float64) + 0.587 * d[:, 12].astype(np.float64) + 0.114 * d[:, 13].astype(np.float64)),
                       (AM.DIST2, lambda d: ((d[:, 0:3].astype(np.float64) - np.asarray(AR.POINT, f32).astype(np.float64)) ** 2).sum(axis=1))):
        v = AM.values(family, attr, AR.POINT)
        with np.errstate(all="ignore"):
            w = wide(family).astype(f32)
        ok = np.isfinite(v) & np.isfinite(w)
        assert (v[ok] != w[ok]).any(), attr


def test_ranks_agree_with_a_float64_argsort_where_no_zero_tie_decides(family):
    rng = np.random.default_rng(2)
    members = rng.random(len(family)) < 0.7
    for attr in AM.ATTRS:
        v = AM.values(family, attr, AR.POINT)
        k = AM.population_keys(v, members)
        pop = v[members & ~np.isnan(v)]
        assert len(k) == len(pop)
        want = np.sort(pop.astype(np.float64), kind="stable")
        got = AM.key_values(k).astype(np.float64)
        assert np.array_equal(got, want)                           # as numbers (-0 == +0) ...
        zeros = got == 0
        if zeros.any():                                            # ... and among the zeros every -0 stands before every +0
            sign = np.signbit(AM.key_values(k)[zeros])
            assert (np.diff(sign.astype(np.int8)) <= 0).all()
        words, population = AM.ranks(v, members, [0, len(k) // 2, len(k) - 1, len(k), len(k) + 5])
        assert population == len(k) and words[3] == AM.NOT_ALIVE and words[4] == AM.NOT_ALIVE
        assert np.array_equal(words[:3].view(f32).astype(np.float64), want[[0, len(k) // 2, len(k) - 1]])


def test_select_range_words_and_the_scopes(family):
    n = len(family)
    nw = (n + 31) // 32
    rng = np.random.default_rng(3)
    alive = rng.random(n) < 0.8
    v = AM.values(family, AM.OPACITY)
    everything = AM.select_range(np.zeros(nw, np.uint32), v, alive, -np.inf, np.inf)
    assert np.array_equal(everything, AM.pack_bits(alive & ~np.isnan(v), nw))       # +-inf bounds: every alive splat whose value is not NaN
    assert not AM.select_range(np.zeros(nw, np.uint32), v, alive, 0.75, 0.25).any()   # lo > hi: nothing
    full = ~np.zeros(nw, np.uint32)
    sub = AM.select_range(full, v, alive, 0.25, 0.75, subtract=True)
    assert np.array_equal(full & ~sub, AM.pack_bits(alive & (v >= f32(0.25)) & (v <= f32(0.75)), nw))
    assert (sub[-1] >> (n % 32)) == (0xFFFFFFFF >> (n % 32))       # the tail bits beyond N survive a subtract
    # scope: the tail bits that select-all sets never count, no words means nobody
    assert AM.scope_flags(np.ones(33, bool), ~np.zeros(2, np.uint32), True).sum() == 33
    assert AM.scope_flags(np.ones(33, bool), None, True).sum() == 0
    assert AM.scope_flags(alive, None, False).sum() == alive.sum()


def test_hist_scale_refusals():
    assert AM.hist_scale(0.0, 1.0, 64) == f32(64.0)
    for lo, hi, bins in ((0.0, 1.0, 0), (0.0, 1.0, 4097), (1.0, 1.0, 4), (2.0, 1.0, 4), (np.nan, 1.0, 4), (0.0, np.inf, 4), (-3e38, 3e38, 4), (0.0, 1e-42, 4096)):
        assert AM.hist_scale(lo, hi, bins) is None, (lo, hi, bins)
    assert AM.quantile_ranks([0.0, 0.5, 0.999, 1.0], 10).tolist() == [0, 5, 9, 9]
