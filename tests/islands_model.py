"""The numpy twin of gs_renderer_edit_components / gs_renderer_edit_select_islands / gs_renderer_edit_grow_selection (helper, not a test): the contract
of DESIGN.md section 4.18 on top of tests/neighbour_model.py, so that it gives the same integers and words as the kernels.

  brute_components   the edges straight from the definition -- every pair through neighbour_model.neighbour -- then a plain union-find, O(n^2)
  grid_components    the edges the way the kernels find them: cell_coords, the stable sort by key, nine runs per splat, out-of-range rows skipped, only
                     the sorted positions j < i -- for sizes where O(n^2) is too slow; tests/test_islands_model.py holds it to brute_components.  Its
                     keyword switches are the mutations section 4.18 lists
  labels_sizes       label(i) = the smallest index of i's component, size(i) = its splats; 0xFFFFFFFF and 0 for a splat that is not alive
  island_flags, select_islands, grow_selection   the two selecting calls on packed words
  chain, broken_chain, ring, bridge, clumps      the point families of the component suites, each a (positions, radius, ...)

A component is a class of the transitive closure of N over the ALIVE splats; an alive splat whose position is not finite has no edges."""
from __future__ import annotations

import numpy as np

import neighbour_model as NM

f32 = np.float32
NOT_ALIVE = NM.NOT_ALIVE


class UnionFind:
    """a plain union-find over 0 .. n - 1, the smaller root kept; union_pairs takes arrays of edges and leaves the loop to those that still join two trees"""

    def __init__(self, n: int):
        self.parent = np.arange(n, dtype=np.int64)

    def find(self, x: int) -> int:
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = int(p[x])
        return x

    def union(self, a: int, b: int) -> None:
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)

    def roots(self) -> np.ndarray:
        """root of every element (the parents fully compressed on the way)"""
        p = self.parent
        while True:
            q = p[p]
            if np.array_equal(q, p):
                return p
            p[:] = q

    def union_pairs(self, a, b) -> None:
        a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
        if len(a) == 0:
            return
        r = self.roots()
        ra, rb = r[a], r[b]
        keep = ra != rb
        if keep.any():
            n = len(r)
            for code in np.unique(ra[keep] * n + rb[keep]):
                self.union(int(code) // n, int(code) % n)


def brute_edges(pos, alive, radius, block: int = 256, strict: bool = False):
    """the edges (i, j), i < j, of the alive splats, straight from N, a block of rows at a time"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    idx = np.flatnonzero(np.asarray(alive, bool))
    p = pos[idx]
    r2 = f32(radius) * f32(radius)
    for s in range(0, len(idx), block):
        hit = NM.neighbour(p[s:s + block, None, :], p[None, :, :], r2, strict)
        back = NM.neighbour(p[None, :, :], p[s:s + block, None, :], r2, strict)
        assert np.array_equal(hit, back)                           # N is symmetric in fp32: asserted on whatever goes through here
        i, j = np.nonzero(hit)
        keep = (s + i) < j
        yield idx[s + i[keep]], idx[j[keep]]


def brute_components(pos, alive, radius, strict: bool = False) -> np.ndarray:
    """root[i] for every splat (a splat that is not alive is left a root of its own): edges from N over all pairs, then a plain union-find"""
    uf = UnionFind(len(np.asarray(alive)))
    for a, b in brute_edges(pos, alive, radius, strict=strict):
        uf.union_pairs(a, b)
    return uf.roots().copy()


ROWS = tuple((dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1))


def grid_components(pos, alive, radius, skip: bool = True, strict: bool = False, lower_only: bool = True, rows=ROWS, budget: int = 1 << 22,
                    with_order: bool = False):
    """root[i] for every splat, the edges found the way the kernels find them: the listed splats sorted stably by key, for each the nine runs
    (x-1 .. x+1, y + dy, z + dz), a row outside [0, 2^21 - 1] SKIPPED, and of a run only the sorted positions j < i.  The switches are the mutations:
    skip False clamps such a row, strict is `<` for `<=`, lower_only False visits j != i, rows drops some (dy, dz).
    with_order: also the splat indices in sorted order"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    n = len(pos)
    uf = UnionFind(n)
    listed = NM.listed_flags(pos, alive)
    src = np.flatnonzero(listed)
    m = len(src)
    if m == 0:
        return (uf.roots().copy(), src) if with_order else uf.roots().copy()
    cells, _ = NM.cell_coords(pos, listed, radius)
    keys = (cells[:, 0] | (cells[:, 1] << 21) | (cells[:, 2] << 42)).astype(np.uint64)
    order = np.argsort(keys, kind="stable")
    keys, cells, p, src = keys[order], cells[order], pos[src][order], src[order]
    r2 = f32(radius) * f32(radius)
    me = np.arange(m)
    CELL_MAX = NM.CELL_MAX
    for dy, dz in rows:
        y, z = cells[:, 1] + dy, cells[:, 2] + dz
        inside = (y >= 0) & (y <= CELL_MAX) & (z >= 0) & (z <= CELL_MAX)
        y, z = np.clip(y, 0, CELL_MAX), np.clip(z, 0, CELL_MAX)
        x0, x1 = np.maximum(cells[:, 0] - 1, 0), np.minimum(cells[:, 0] + 1, CELL_MAX)
        first = (x0 | (y << 21) | (z << 42)).astype(np.uint64)
        last = (x1 | (y << 21) | (z << 42)).astype(np.uint64)
        a = np.searchsorted(keys, first, side="left")
        b = np.searchsorted(keys, last, side="right")
        if skip:
            b = np.where(inside, b, a)
        if lower_only:
            b = np.maximum(np.minimum(b, me), a)                   # of a run only the sorted positions below i
        lens = b - a
        cum = np.cumsum(lens)
        start = 0
        while start < m:
            stop = max(int(np.searchsorted(cum, (cum[start - 1] if start else 0) + budget, side="right")), start + 1)
            ln = lens[start:stop]
            owner = np.repeat(me[start:stop], ln)
            j = np.repeat(a[start:stop], ln) + np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
            hit = NM.neighbour(p[owner], p[j], r2, strict) & (j != owner)
            uf.union_pairs(src[owner[hit]], src[j[hit]])
            start = stop
    return (uf.roots().copy(), src) if with_order else uf.roots().copy()


def labels_sizes(roots, alive):
    """(labels, sizes) as gs_renderer_edit_components writes them, from any array that is constant exactly on the components of the alive splats"""
    roots = np.asarray(roots, np.int64)
    alive = np.asarray(alive, bool)
    n = len(roots)
    labels, sizes = np.full(n, NOT_ALIVE, np.uint32), np.zeros(n, np.uint32)
    idx = np.flatnonzero(alive)
    if len(idx) == 0:
        return labels, sizes
    _, inv, cnt = np.unique(roots[idx], return_inverse=True, return_counts=True)
    low = np.full(len(cnt), n, np.int64)
    np.minimum.at(low, inv, idx)
    labels[idx] = low[inv]
    sizes[idx] = cnt[inv]
    return labels, sizes


def components(pos, alive, radius, brute_up_to: int = 5000):
    """(labels, sizes) by brute force where it is quick, by the grid above that"""
    alive = np.asarray(alive, bool)
    roots = brute_components(pos, alive, radius) if int(alive.sum()) <= brute_up_to else grid_components(pos, alive, radius)
    return labels_sizes(roots, alive)


def island_flags(sizes, alive, min_size: int) -> np.ndarray:
    return np.asarray(alive, bool) & (np.asarray(sizes, np.int64) < int(min_size))


def select_islands(selected_words, sizes, alive, min_size: int, subtract: bool = False) -> np.ndarray:
    """the selection words after gs_renderer_edit_select_islands: |= island, or &= ~island; no bit at or beyond N comes from it"""
    sel = np.ascontiguousarray(selected_words, np.uint32).copy()
    w = NM.pack_bits(island_flags(sizes, alive, min_size), len(sel))
    return (sel & ~w) if subtract else (sel | w)


def grow_selection(selected_words, labels, alive) -> np.ndarray:
    """the selection words after gs_renderer_edit_grow_selection: a seed is an alive splat (index < N) whose bit is set; every alive splat whose label
    is a seed's is added; no bit is cleared, none at or beyond N is set"""
    sel = np.ascontiguousarray(selected_words, np.uint32).copy()
    alive = np.asarray(alive, bool)
    n = len(alive)
    bits = np.unpackbits(sel.view(np.uint8), bitorder="little")[:n].astype(bool)
    seeds = alive & bits
    grown = alive & np.isin(np.asarray(labels), np.unique(np.asarray(labels)[seeds]))
    return sel | NM.pack_bits(grown, len(sel))


# ---- the families ---------------------------------------------------------------------------------------------------------------------------------------
# The chains live on multiples of 0.5 below 2^23: every position, every difference and every square is exact in fp32.  radius = 1024; a link is
# 1023.5 long (one unit of that lattice inside the radius), a gap 1024.5 (one beyond it), two links 2047.
CHAIN_RADIUS, CHAIN_LINK, CHAIN_GAP = 1024.0, 1023.5, 1024.5


def shuffled(pos, seed: int):
    """the points under a seeded permutation of their splat indices: (positions, where[k] = the index point k of the original order got)"""
    where = np.random.default_rng(seed).permutation(len(pos))
    out = np.empty_like(pos)
    out[where] = pos
    return out, where


def broken_chain(n: int, seed: int, gaps=(), axis: int = 0):
    """n points on a line along `axis`, consecutive ones a link apart but for the k given places (a gap follows point g of the line), their splat
    indices shuffled: (positions, radius, where, the closed-form sizes of the k + 1 pieces in line order)"""
    gaps = np.asarray(sorted(set(int(g) for g in gaps)), np.int64)
    assert len(gaps) == 0 or (gaps[0] >= 0 and gaps[-1] < n - 1)
    step = np.full(max(n - 1, 0), CHAIN_LINK)
    step[gaps] = CHAIN_GAP
    x = np.concatenate([[0.0], np.cumsum(step)])[:n]
    assert x.max() < 2.0 ** 23
    line = np.zeros((n, 3), f32)
    line[:, axis] = x.astype(f32)
    assert np.array_equal(line[:, axis].astype(np.float64), x)     # exact
    pos, where = shuffled(line, seed)
    sizes = np.diff(np.concatenate([[-1], gaps, [n - 1]]))
    return pos, CHAIN_RADIUS, where, sizes


def chain(n: int, seed: int, axis: int = 0):
    pos, radius, where, _ = broken_chain(n, seed, (), axis)
    return pos, radius, where


def ring(n: int, seed: int):
    """the chain closed: n points on a circle, neighbours on it 0.98 radius apart, the next but one nearly twice that; indices shuffled"""
    radius = 1.0
    rho = 0.98 * radius / (2.0 * np.sin(np.pi / n))
    t = 2.0 * np.pi * np.arange(n) / n
    circle = np.stack([rho * np.cos(t), rho * np.sin(t), np.zeros(n)], axis=1).astype(f32)
    pos, where = shuffled(circle, seed)
    return pos, radius, where


def bridge(k: int, seed: int):
    """two tight clusters of k splats 1.6 apart and one splat half way: (positions, radius 0.9, the bridge's index).  Without it the clusters are
    0.7 beyond each other's reach"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((k, 3)) * 0.02).clip(-0.06, 0.06)
    b = (rng.standard_normal((k, 3)) * 0.02).clip(-0.06, 0.06) + (1.6, 0.0, 0.0)
    pos = np.concatenate([a, [(0.8, 0.0, 0.0)], b]).astype(f32)
    return pos, 0.9, k


def clumps(groups: int, seed: int):
    """`groups` tight groups of 1 .. groups splats, 10 apart, indices shuffled: (positions, radius 0.5, group[i] = the size of the group splat i is in)"""
    rng = np.random.default_rng(seed)
    pts, size = [], []
    for g in range(1, groups + 1):
        centre = np.array([10.0 * (g % 5), 10.0 * ((g // 5) % 5), 10.0 * (g // 25)])
        pts.append(centre + (rng.random((g, 3)) - 0.5) * 0.2)
        size += [g] * g
    pos, where = shuffled(np.concatenate(pts).astype(f32), seed + 1)
    group = np.empty(len(size), np.int64)
    group[where] = size
    return pos, 0.5, group


def new_families(seed: int, n: int = 1500):
    """(name, positions, radius) of every new family at about n points"""
    k = 7
    gaps = np.sort(np.random.default_rng(seed).choice(n - 1, k, replace=False))
    return [("chain",) + chain(n, seed)[:2], ("chain along y",) + chain(n, seed, 1)[:2], ("chain along z",) + chain(n, seed, 2)[:2],
            ("broken chain",) + broken_chain(n, seed, gaps)[:2], ("ring",) + ring(n, seed)[:2], ("bridge",) + bridge(min(n // 2, 150), seed)[:2],
            ("clumps",) + clumps(24, seed)[:2]]
