"""CPU: the grid model of tests/neighbour_model.py -- the cell rule, nine runs, out-of-range rows skipped: what the kernels of gs_neighbours.hip do --
equals the brute-force count of the contract on the adversarial families of tests/neighbour_rig.py, and every family really holds what it claims to:
the premises are asserted, so that a family that stopped being adversarial fails here and not silently on the GPU."""
import numpy as np
import pytest

import neighbour_model as NM
import neighbour_rig as NR

f32 = np.float32
N = 1500
SEEDS = (1, 2, 3, 4, 5, 6, 7)


def all_alive(pos):
    return np.ones(len(pos), bool)


@pytest.mark.parametrize("seed", SEEDS)
def test_grid_model_equals_brute_force_on_every_family(seed):
    for name, pos, radius in NR.adversarial(N, seed):
        alive = all_alive(pos)
        want = NM.brute_counts(pos, alive, radius)
        got = NM.grid_counts(pos, alive, radius)
        assert np.array_equal(got, want), (name, seed, np.flatnonzero(got != want)[:8])
        # no neighbour pair lies more than one cell apart: the grid argument itself
        cells, _ = NM.cell_coords(pos, NM.listed_flags(pos, alive), radius)
        p = pos[NM.listed_flags(pos, alive)]
        r2 = f32(radius) * f32(radius)
        worst = 0
        for s in range(0, len(p), 256):
            hit = NM.neighbour(p[s:s + 256, None, :], p[None, :, :], r2)
            i, j = np.nonzero(hit)
            if len(i):
                worst = max(worst, int(np.abs(cells[s + i] - cells[j]).max()))
        assert worst <= 1, (name, seed, worst)


@pytest.mark.parametrize("seed", SEEDS[:3])
def test_grid_model_with_dead_splats_radii_and_limits(seed):
    rng = np.random.default_rng(seed)
    for name, pos, radius in NR.adversarial(700, seed):
        alive = rng.random(len(pos)) < 0.7
        for r in (radius, NR.isolating_radius(pos), radius * 3.0):
            want = NM.brute_counts(pos, alive, r)
            assert np.array_equal(NM.grid_counts(pos, alive, r), want), (name, r)
            assert not want[~alive].any()
            for limit in (1, 4):
                assert np.array_equal(NM.grid_counts(pos, alive, r, limit=limit), np.minimum(want, limit)), (name, r, limit)
    pos, _ = NR.gaussian(300, seed)
    finite = NR.one_cell_radius(pos)
    assert np.array_equal(NM.brute_counts(pos, all_alive(pos), finite), np.full(300, 299))
    assert np.array_equal(NM.grid_counts(pos, all_alive(pos), finite), np.full(300, 299))


def test_the_families_hold_what_they_claim():
    seed = 3
    fam = {name: (pos, radius) for name, pos, radius in NR.adversarial(N, seed)}
    # pairs with d2 == r2: the lattice at radius (three per inner point and direction), and `<` for `<=` loses exactly them
    pos, radius = fam["lattice at radius"]
    alive = all_alive(pos)
    assert NM.exact_boundary_pairs(pos, alive, radius) >= 2 * N
    want = NM.brute_counts(pos, alive, radius)
    assert want.max() == 6 and NM.grid_counts(pos, alive, radius, strict=True).max() == 0
    # clamped cells: the outliers' cells lie beyond 2^21 - 1 before the clamp
    pos, radius = fam["outliers"]
    alive = all_alive(pos)
    cells, raw = NM.cell_coords(pos, NM.listed_flags(pos, alive), radius)
    assert (raw > NM.CELL_MAX).any() and cells.max() == NM.CELL_MAX
    # a pair an unskipped out-of-range row of cells would count twice: clamping instead of skipping changes the counts
    assert not np.array_equal(NM.grid_counts(pos, alive, radius, skip=False), NM.brute_counts(pos, alive, radius))
    # ... as it does wherever two neighbours share a cell at the grid's floor: the identical cloud
    pos, radius = NR.identical(40)
    assert np.array_equal(NM.brute_counts(pos, all_alive(pos), radius), np.full(40, 39))
    assert NM.grid_counts(pos, all_alive(pos), radius, skip=False).max() > 39
    # no self-exclusion: one more everywhere
    assert np.array_equal(NM.grid_counts(pos, all_alive(pos), radius, exclude_self=False), np.full(40, 40))
    # h = radius without the margin: the ulp triples are neighbours in fp32 two such cells apart
    pos, radius = fam["ulp pairs"]
    alive = all_alive(pos)
    want = NM.brute_counts(pos, alive, radius)
    assert want[1] >= 2 and want[2] >= 1                            # 1 - 2^-24 sees 0 and 2 on its axis
    assert not np.array_equal(NM.grid_counts(pos, alive, radius, margin=False), want)
    # fp32 cell arithmetic: two million cells from the origin it cannot tell neighbouring cells apart
    pos, radius = fam["far line + anchor"]
    alive = all_alive(pos)
    assert NM.exact_boundary_pairs(pos, alive, radius) >= 2 * (N - 100)
    assert not np.array_equal(NM.grid_counts(pos, alive, radius, fp64=False), NM.brute_counts(pos, alive, radius))
    # duplicates are neighbours of one another; non-finite positions are nobody's and have none
    pos, radius = fam["duplicates"]
    assert NM.brute_counts(pos, all_alive(pos), radius).min() >= 2
    pos, radius = fam["non-finite"]
    alive = all_alive(pos)
    want = NM.brute_counts(pos, alive, radius)
    bad = ~np.isfinite(pos).all(axis=1)
    assert bad.sum() == 7 and not want[bad].any()
    clean = NM.brute_counts(pos[~bad], np.ones(int((~bad).sum()), bool), radius)
    assert np.array_equal(want[~bad], clean)


def test_words_and_selection_of_the_twin():
    pos, radius = NR.lattice(33)
    alive = np.ones(33, bool)
    alive[[5, 32]] = False
    counts = NM.brute_counts(pos, alive, radius)
    words = NM.counts_words(counts, alive, 2)
    assert words[5] == words[32] == NM.NOT_ALIVE and words[alive].max() == 2
    zero = np.zeros(2, np.uint32)
    assert np.array_equal(NM.select_sparse(zero, counts, alive, 0), zero)
    everything = NM.select_sparse(zero, counts, alive, 100)
    assert everything.tolist() == [0xFFFFFFFF & ~(1 << 5), 0]      # 33 splats: bit 32 is dead, bits 33 .. 63 are never set
    some = NM.select_sparse(zero, counts, alive, 4)
    assert np.array_equal(NM.select_sparse(everything, counts, alive, 4, subtract=True), everything & ~some)
    nan = pos.copy()
    nan[7] = (np.nan, 0, 0)
    assert NM.sparse_flags(NM.brute_counts(nan, alive, radius), alive, 1)[7] and not NM.sparse_flags(NM.brute_counts(nan, alive, radius), alive, 0)[7]
    for r, refused in ((np.nan, True), (np.inf, True), (0.0, True), (-1.0, True), (9e-16, True), (1e-15, False), (1e15, False), (1.1e15, True), (0.5, False)):
        assert NM.radius_refused(r) == refused, r
