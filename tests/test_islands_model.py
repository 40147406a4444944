"""CPU: the grid model of tests/islands_model.py -- the edges the way the kernels of gs_neighbours.hip find them -- gives the components brute force
gives, on the families of tests/neighbour_rig.py and on the new ones, whose premises are asserted and not assumed; and a model of cc_link, the
lock-free union-find, stepped one atomic operation at a time under adversarial schedules with loads that may be stale."""
import random

import numpy as np
import pytest

import islands_model as IM
import neighbour_model as NM
import neighbour_rig as NR

f32 = np.float32
N = 1500
SEEDS = (1, 2, 3)


def same_partition(a, b, alive) -> bool:
    la, lb = IM.labels_sizes(a, alive), IM.labels_sizes(b, alive)
    return np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])


@pytest.mark.parametrize("seed", SEEDS)
def test_grid_components_equal_brute_force_on_every_family(seed):
    rng = np.random.default_rng(seed)
    for name, pos, radius in NR.adversarial(N, seed) + IM.new_families(seed, N) + [("identical",) + NR.identical(300)]:
        for alive in (np.ones(len(pos), bool), rng.random(len(pos)) < 0.7):
            for r in (radius, NR.isolating_radius(pos), radius * 3.0):
                want = IM.brute_components(pos, alive, r)          # (asserts N(i, j) == N(j, i) on every pair it looks at)
                assert same_partition(IM.grid_components(pos, alive, r), want, alive), (name, seed, r)
                # visiting j != i and not only j < i finds every edge twice: the same partition (a premise of NeighbourForEach, not a failure)
                if r == radius:
                    assert same_partition(IM.grid_components(pos, alive, r, lower_only=False), want, alive), (name, seed, r)
                labels, sizes = IM.labels_sizes(want, alive)
                assert (labels[~alive] == IM.NOT_ALIVE).all() and not sizes[~alive].any()
                assert (labels[alive] <= np.flatnonzero(alive)).all() and (labels[labels[alive]] == labels[alive]).all()
                assert np.array_equal(np.bincount(labels[alive], minlength=len(pos))[labels[alive]], sizes[alive])


def test_islands_of_size_below_two_are_the_sparse_splats_with_no_neighbour():
    for name, pos, radius in NR.adversarial(N, 3) + IM.new_families(3, N):
        alive = np.random.default_rng(5).random(len(pos)) < 0.8
        _, sizes = IM.components(pos, alive, radius)
        zero = np.zeros((len(pos) + 31) // 32, np.uint32)
        assert np.array_equal(IM.select_islands(zero, sizes, alive, 2), NM.select_sparse(zero, NM.brute_counts(pos, alive, radius), alive, 1)), name
        assert not IM.select_islands(zero, sizes, alive, 0).any() and not IM.select_islands(zero, sizes, alive, 1).any()


def test_the_new_families_hold_what_they_claim():
    n = 4097
    # the chain: one component, label 0, longer than 16 workgroups of 256 sorted positions; every link is inside the radius, every other pair beyond it
    pos, radius, where = IM.chain(n, 4)
    alive = np.ones(n, bool)
    counts = NM.brute_counts(pos, alive, radius)
    inv = np.argsort(where)                                        # inv[k] = the line's point at splat index k ... where[point] = index
    assert sorted(counts.tolist()) == [1, 1] + [2] * (n - 2) and counts[where[0]] == counts[where[n - 1]] == 1
    roots, order = IM.grid_components(pos, alive, radius, with_order=True)
    labels, sizes = IM.labels_sizes(roots, alive)
    assert (labels == 0).all() and (sizes == n).all() and n > 16 * 256
    assert not np.array_equal(order, np.arange(n)) and np.abs(inv[order] - np.arange(n)).max() <= 1      # sorted order is the line's (two points of one cell
    # may swap), the indices are not
    assert same_partition(IM.brute_components(pos, alive, radius), roots, alive)
    # `<` for `<=` changes nothing here (no pair at exactly the radius); a link IS exact: one lattice unit more and it breaks
    assert NM.exact_boundary_pairs(pos, alive, radius) == 0
    assert f32(IM.CHAIN_LINK) ** 2 < f32(radius) ** 2 < f32(IM.CHAIN_GAP) ** 2
    # the broken chain: k gaps, k + 1 components of the closed-form sizes, each labelled by its smallest index
    gaps = (0, 255, 256, 1000, 2047, 4000, 4094)
    pos, radius, where, want = IM.broken_chain(n, 5, gaps)
    assert want.tolist() == [1, 255, 1, 744, 1047, 1953, 94, 2] and want.sum() == n
    labels, sizes = IM.labels_sizes(IM.brute_components(pos, alive, radius), alive)
    piece = np.repeat(np.arange(len(want)), want)                  # of the line's points
    for k, size in enumerate(want):
        members = where[piece == k]
        assert (sizes[members] == size).all() and (labels[members] == members.min()).all(), k
    assert same_partition(IM.grid_components(pos, alive, radius), IM.brute_components(pos, alive, radius), alive)
    # the label is the component's minimum, not the index of whatever splat the union-find ends on: on a shuffled chain the first sorted position
    # (the root of a union by sorted position) is index 0 in one shuffle out of n
    pos, radius, where = IM.chain(257, 6)
    assert where[0] != 0
    # the ring: one component, every splat has exactly two neighbours
    pos, radius, where = IM.ring(n, 7)
    assert (NM.brute_counts(pos, alive, radius) == 2).all()
    labels, sizes = IM.labels_sizes(IM.brute_components(pos, alive, radius), alive)
    assert (labels == 0).all() and (sizes == n).all()
    # the bridge: one component with it, two without it, and it alone joins them
    pos, radius, b = IM.bridge(100, 8)
    alive = np.ones(len(pos), bool)
    labels, sizes = IM.labels_sizes(IM.brute_components(pos, alive, radius), alive)
    assert (labels == 0).all() and (sizes == 201).all()
    alive[b] = False
    labels, sizes = IM.labels_sizes(IM.brute_components(pos, alive, radius), alive)
    assert labels[b] == IM.NOT_ALIVE and sorted(set(labels[alive].tolist())) == [0, b + 1] and (sizes[alive] == 100).all()
    # the clumps: G groups of 1 .. G splats: the component of a splat is its group
    pos, radius, group = IM.clumps(24, 9)
    alive = np.ones(len(pos), bool)
    labels, sizes = IM.labels_sizes(IM.brute_components(pos, alive, radius), alive)
    assert np.array_equal(sizes, group) and len(set(labels.tolist())) == 24 and len(pos) == 300
    for k in (0, 1, 2, 7, 24, 25):
        assert int(IM.island_flags(sizes, alive, k).sum()) == max(k - 1, 0) * k // 2, k


def test_each_mutation_is_seen_by_the_family_named():
    seed = 3
    fam = {name: (pos, radius) for name, pos, radius in NR.adversarial(N, seed) + IM.new_families(seed, N)}

    def differs(name, **mutation):
        pos, radius = fam[name]
        alive = np.ones(len(pos), bool)
        return not same_partition(IM.grid_components(pos, alive, radius, **mutation), IM.brute_components(pos, alive, radius), alive)

    # a dropped (dy, dz) row: the chain along y loses (dy = -1, dz = 0), the chain along z (0, -1); the chain along x needs only the splat's own row
    rows = lambda dy, dz: tuple(r for r in IM.ROWS if r != (dy, dz))
    assert differs("chain along y", rows=rows(-1, 0)) and differs("chain along z", rows=rows(0, -1))
    assert not differs("chain", rows=((0, 0),)) and differs("chain", rows=rows(0, 0))
    # `<` for `<=`: the lattice at the radius falls apart into single splats
    assert differs("lattice at radius", strict=True)
    # clamping an out-of-range row and not skipping it finds no edge that is not there (an edge found twice is the same edge): unlike the counts of
    # section 4.17 the partition does not change -- stated, not hidden
    assert not differs("outliers", skip=False) and not differs("lattice at radius", skip=False)


def test_words_of_the_twin_at_33():
    pos, radius = NR.lattice(33)
    alive = np.ones(33, bool)
    alive[[5, 32]] = False
    labels, sizes = IM.components(pos, alive, radius)
    assert labels[5] == labels[32] == IM.NOT_ALIVE and sizes[5] == sizes[32] == 0
    everything = ~np.zeros(2, np.uint32)                           # select-all's quirk: bits 33 .. 63 set
    assert np.array_equal(IM.grow_selection(everything, labels, alive), everything)
    tail = np.array([0, 0xFFFFFFFE], np.uint32)                    # only bits at or beyond N: no seed
    assert np.array_equal(IM.grow_selection(tail, labels, alive), tail)
    dead = np.array([1 << 5, 0], np.uint32)                        # a deleted splat's bit: no seed, and it stays
    assert np.array_equal(IM.grow_selection(dead, labels, alive), dead)
    one = np.array([1 << 7, 0], np.uint32)
    grown = IM.grow_selection(one, labels, alive)
    assert np.array_equal(grown, NM.pack_bits(alive & (labels == labels[7]), 2)) and NM.pack_bits(alive, 2)[1] == 0
    assert np.array_equal(IM.select_islands(everything, sizes, alive, 100, subtract=True), everything & ~NM.pack_bits(alive, 2))


# ---- cc_link under adversarial interleavings --------------------------------------------------------------------------------------------------------------
# The memory: every word of parent[] keeps all the values it ever held.  A load may return ANY of them (what a cache that nobody invalidates can do);
# a store appends; a compare-and-swap acts on the newest.  Threads are generators that yield one atomic operation at a time: the text of cc_find /
# cc_union / cc_link_kernel, operation for operation.
def cc_find(x):
    while True:
        p = yield ("ld", x)
        if p == x:
            return x
        g = yield ("ld", p)
        if g == p:
            return p
        yield ("st", x, g)
        x = g


def cc_union(a, b):
    b = yield from cc_find(b)
    if b == a:
        return a
    while True:
        a = yield from cc_find(a)
        if a == b:
            return a
        hi, lo = max(a, b), min(a, b)
        seen = yield ("cas", hi, lo)
        if seen == hi:
            return lo
        a = lo
        b = yield from cc_find(seen)


def cc_thread(i, edges):
    mine = i
    for j in edges:
        mine = yield from cc_union(mine, j)


def op_bound(m: int, edges: int) -> int:
    """atomic operations one thread can need for `edges` unions over m positions.  One union: the first find descends from below m, two positions
    per three operations, and ends in at most two more; in the loop a + b < 2 m falls with every find step and by at least one with every failed
    compare-and-swap, an iteration costs two finds' ends (four operations) and the compare-and-swap besides the descent: 3 m / 2 + 2 + 3 m + 5 * 2 m"""
    return edges * (15 * m + 2)


def run_link(m, edges_of, schedule, stale, seed):
    """steps every thread to its end; returns the final parent[] and asserts the invariant and the bound on the way"""
    rng = random.Random(seed)
    hist = [[x] for x in range(m)]
    threads = {i: cc_thread(i, edges_of[i]) for i in range(m) if edges_of[i]}
    pending, ops = {}, {i: 0 for i in threads}
    for i, t in list(threads.items()):
        pending[i] = next(t)
    turn = 0
    while threads:
        if schedule == "random":
            i = rng.choice(sorted(threads))
        elif schedule == "lockstep":                               # a wave: every thread one operation, in turn
            live = sorted(threads)
            i = live[turn % len(live)]; turn += 1
        elif schedule == "reverse lockstep":
            live = sorted(threads, reverse=True)
            i = live[turn % len(live)]; turn += 1
        elif schedule == "one at a time":                          # serial, highest first
            i = max(threads)
        else:                                                      # "starve the lowest": whoever is not the lowest live thread, the lowest only when alone or rarely
            live = sorted(threads)
            i = rng.choice(live[1:]) if len(live) > 1 and rng.random() < 0.95 else live[0]
        op = pending[i]
        ops[i] += 1
        assert ops[i] <= op_bound(m, len(edges_of[i])), (schedule, stale, seed, i)
        if op[0] == "ld":
            h = hist[op[1]]
            result = h[-1] if stale == "fresh" else h[0] if stale == "oldest" else rng.choice(h)
        elif op[0] == "st":
            assert op[2] <= op[1]
            hist[op[1]].append(op[2]); result = None
        else:
            result = hist[op[1]][-1]
            if result == op[1]:
                assert op[2] < op[1]
                hist[op[1]].append(op[2])
        assert all(h[-1] <= x for x, h in enumerate(hist))         # parent[x] <= x at every step
        try:
            pending[i] = threads[i].send(result)
        except StopIteration:
            del threads[i], pending[i]
    return [h[-1] for h in hist]


def serial_partition(m, edges_of):
    uf = IM.UnionFind(m)
    for i in range(m):
        for j in edges_of[i]:
            uf.union(i, j)
    return uf.roots().copy()


def partition_of(parent):
    p = np.asarray(parent, np.int64).copy()
    while not np.array_equal(p[p], p):
        p = p[p]
    return p


def link_graphs(seed):
    """(name, m, edges_of[i] = the positions j < i thread i joins itself to)"""
    rng = random.Random(seed)
    out = []
    m = 24
    out.append(("chain", m, [[i - 1] if i else [] for i in range(m)]))
    out.append(("ring", m, [[i - 1] if i else [] for i in range(m - 1)] + [[m - 2, 0]]))
    out.append(("complete", 10, [list(range(i)) for i in range(10)]))
    out.append(("star to the last", m, [[] for _ in range(m - 1)] + [list(range(m - 1))]))
    out.append(("two combs", m, [[i - 2] if i >= 2 else [] for i in range(m)]))
    out.append(("random sparse", m, [[j for j in range(i) if rng.random() < 0.08] for i in range(m)]))
    out.append(("random dense", 16, [[j for j in range(i) if rng.random() < 0.5] for i in range(16)]))
    out.append(("pairs", m, [[i - 1] if i % 2 else [] for i in range(m)]))
    return out


@pytest.mark.parametrize("schedule", ["random", "lockstep", "reverse lockstep", "one at a time", "starve the lowest"])
@pytest.mark.parametrize("stale", ["fresh", "oldest", "any"])
def test_cc_link_model_under_adversarial_schedules(schedule, stale):
    for seed in range(6):
        for name, m, edges_of in link_graphs(seed):
            parent = run_link(m, edges_of, schedule, stale, seed)
            assert all(p <= x for x, p in enumerate(parent))
            assert np.array_equal(partition_of(parent), serial_partition(m, edges_of)), (name, schedule, stale, seed)
