"""The numpy twin of gs_renderer_edit_neighbour_counts / gs_renderer_edit_select_sparse (helper, not a test): the contract of DESIGN.md section 4.17
restated operation by operation, so that it gives the same integers as the kernels.

  brute_counts   count(i) straight from the definition, O(n^2): every pair through the fp32 predicate in the contract's operation order
  grid_counts    the same integers the way the kernels find them -- fp64 cell rule, stable sort by key, nine runs per splat, out-of-range rows of
                 cells skipped -- for sizes where O(n^2) is too slow; tests/test_neighbour_model.py holds it to brute_counts.  Its keyword switches
                 are the mutations section 4.17 lists: the tests assert that the families they use tell each of them from the contract.

Alive is the rule of the existing models: index < N, not deleted, not cut (edit_model.EditModel.cut, export_model.ExportModel.alive)."""
from __future__ import annotations

import numpy as np

f32 = np.float32
CELL_MAX = (1 << 21) - 1
NOT_ALIVE = 0xFFFFFFFF
RADIUS_MIN, RADIUS_MAX = 1e-15, 1e15


def alive_flags(n: int, deleted_words=None, cut=None) -> np.ndarray:
    alive = np.ones(n, bool)
    if deleted_words is not None:
        alive &= ~np.unpackbits(np.ascontiguousarray(deleted_words, np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)
    if cut is not None:
        alive &= ~np.asarray(cut, bool)
    return alive


def radius_refused(radius) -> bool:
    r = f32(radius)
    return not (np.isfinite(r) and f32(RADIUS_MIN) <= r <= f32(RADIUS_MAX))


def neighbour(pi: np.ndarray, pj: np.ndarray, r2, strict: bool = False) -> np.ndarray:
    """N(i, j) in fp32, one rounding per operation: dx = xj - xi, ...; d2 = (dx dx + dy dy) + dz dz; d2 <= r2.  strict: the mutation `<`"""
    with np.errstate(all="ignore"):
        dx, dy, dz = (pj[..., 0] - pi[..., 0]).astype(f32), (pj[..., 1] - pi[..., 1]).astype(f32), (pj[..., 2] - pi[..., 2]).astype(f32)
        d2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)
        return d2 < r2 if strict else d2 <= r2


def brute_counts(pos, alive, radius, block: int = 256) -> np.ndarray:
    """count(i) for every splat (0 for one that is not alive): the alive j != i with N(i, j)"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    n = len(pos)
    alive = np.asarray(alive, bool)
    r2 = f32(radius) * f32(radius)
    out = np.zeros(n, np.int64)
    idx = np.flatnonzero(alive)
    p = pos[idx]
    for s in range(0, len(idx), block):
        hit = neighbour(p[s:s + block, None, :], p[None, :, :], r2)
        hit[np.arange(len(hit)), np.arange(s, s + len(hit))] = False          # j != i
        out[idx[s:s + block]] = hit.sum(axis=1)
    return out


def exact_boundary_pairs(pos, alive, radius) -> int:
    """ordered alive pairs with d2 == r2 exactly (what tells `<` from `<=`)"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)[np.asarray(alive, bool)]
    r2 = f32(radius) * f32(radius)
    total = 0
    for s in range(0, len(pos), 256):
        a, b = pos[s:s + 256, None, :], pos[None, :, :]
        with np.errstate(all="ignore"):
            dx, dy, dz = (b[..., 0] - a[..., 0]).astype(f32), (b[..., 1] - a[..., 1]).astype(f32), (b[..., 2] - a[..., 2]).astype(f32)
            d2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)
        total += int((d2 == r2).sum())
    return total


def listed_flags(pos, alive) -> np.ndarray:
    """the splats the grid holds: alive, every component finite"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    return np.asarray(alive, bool) & np.isfinite(pos).all(axis=1)


def cell_coords(pos, listed, radius, margin: bool = True, fp64: bool = True):
    """(cells of the listed splats (m, 3) int64 after the clamp, the same before it as floats): h = (double) radius (1 + 2^-10),
    floor(((double) p - (double) origin) / h), clamped to [0, 2^21 - 1].  margin False / fp64 False: the mutations"""
    p = np.ascontiguousarray(pos, f32).reshape(-1, 3)[listed]
    if len(p) == 0:
        return np.zeros((0, 3), np.int64), np.zeros((0, 3))
    origin = p.min(axis=0)
    if fp64:
        h = np.float64(f32(radius)) * (1.0009765625 if margin else 1.0)
        q = np.floor((p.astype(np.float64) - origin.astype(np.float64)) / h)
    else:
        h = f32(np.float64(f32(radius)) * (1.0009765625 if margin else 1.0))
        with np.errstate(all="ignore"):
            q = np.floor(((p - origin).astype(f32) / h).astype(f32)).astype(np.float64)
    return np.clip(q, 0, CELL_MAX).astype(np.int64), q


def grid_counts(pos, alive, radius, limit=None, skip: bool = True, margin: bool = True, fp64: bool = True, strict: bool = False, exclude_self: bool = True,
                budget: int = 1 << 22) -> np.ndarray:
    """count(i) for every splat the way the kernels find it (min(count, limit) with a limit): the listed splats sorted stably by x | y << 21 | z << 42,
    and for each the nine runs (x-1 .. x+1, y + dy, z + dz), a row whose y or z falls outside [0, 2^21 - 1] SKIPPED (skip False: clamped, the mutation)"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    n = len(pos)
    out = np.zeros(n, np.int64)
    listed = listed_flags(pos, alive)
    src = np.flatnonzero(listed)
    m = len(src)
    if m == 0:
        return out
    cells, _ = cell_coords(pos, listed, radius, margin, fp64)
    keys = (cells[:, 0] | (cells[:, 1] << 21) | (cells[:, 2] << 42)).astype(np.uint64)
    order = np.argsort(keys, kind="stable")
    keys, cells, p, src = keys[order], cells[order], pos[src][order], src[order]
    r2 = f32(radius) * f32(radius)
    counts = np.zeros(m, np.int64)
    me = np.arange(m)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
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
            lens = b - a
            # the pairs of the runs, a budget of them at a time
            start = 0
            cum = np.cumsum(lens)
            while start < m:
                stop = int(np.searchsorted(cum, (cum[start - 1] if start else 0) + budget, side="right"))
                stop = max(stop, start + 1)
                ln = lens[start:stop]
                owner = np.repeat(me[start:stop], ln)
                offs = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
                j = np.repeat(a[start:stop], ln) + offs
                hit = neighbour(p[owner], p[j], r2, strict)
                if exclude_self:
                    hit &= j != owner
                counts += np.bincount(owner[hit], minlength=m)
                start = stop
    out[src] = counts
    return out if limit is None else np.minimum(out, int(limit))


def counts_words(counts, alive, cap: int) -> np.ndarray:
    """what gs_renderer_edit_neighbour_counts writes: min(count, cap) for an alive splat, 0xFFFFFFFF for every other one"""
    out = np.minimum(np.asarray(counts, np.int64), int(cap)).astype(np.uint32)
    out[~np.asarray(alive, bool)] = NOT_ALIVE
    return out


def sparse_flags(counts, alive, min_neighbours: int) -> np.ndarray:
    return np.asarray(alive, bool) & (np.asarray(counts, np.int64) < int(min_neighbours))


def pack_bits(flags, n_words: int) -> np.ndarray:
    m = np.zeros(n_words * 32, np.uint8)
    m[:len(flags)] = np.asarray(flags, bool)
    return np.packbits(m, bitorder="little").view(np.uint32).copy()


def select_sparse(selected_words, counts, alive, min_neighbours: int, subtract: bool = False) -> np.ndarray:
    """the selection words after gs_renderer_edit_select_sparse: |= sparse, or &= ~sparse; no bit at or beyond N comes from it"""
    sel = np.ascontiguousarray(selected_words, np.uint32).copy()
    w = pack_bits(sparse_flags(counts, alive, min_neighbours), len(sel))
    return (sel & ~w) if subtract else (sel | w)
