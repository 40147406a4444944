"""The cases of the neighbour-count suites (helper, not a test): seeded point families that are hard for a grid -- each a (name, positions, radius)
-- with the radii of the size sweep, and the raw C calls the refusal tests make.  Imports without a GPU; nothing here makes a context."""
import ctypes as C

import numpy as np

f32 = np.float32
ULP1 = f32(2.0 ** -24)                                             # half an ulp of 1.0: 1 - 2^-24 is the float below 1


def gaussian(n: int, seed: int, target: float = 16.0):
    """a unit Gaussian cloud and the radius at which a splat near the centre has about `target` neighbours"""
    rng = np.random.default_rng(seed)
    pos = rng.standard_normal((n, 3)).astype(f32)
    density = n / (2.0 * np.pi) ** 1.5                             # at the centre
    radius = (target / (density * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0) if n > 1 else 1.0
    return pos, float(f32(radius))


def far_cloud(n: int, seed: int):
    """the same cloud a million units from the origin of the space, where the fp32 lattice is 1/16 wide"""
    pos, radius = gaussian(n, seed)
    return (pos + f32(1.0e6)).astype(f32), max(radius, 0.25)


def far_line_with_anchor(n: int):
    """a line of points 3/16 apart a million units out -- every 85th pair at exactly the radius 15.9375 -- and one floater at -3e7: the grid's origin is
    then 1.9 million cells from the line, where fp32 cell arithmetic (p - origin rounds to multiples of 2, the quotient to eighths) puts some of those
    pairs two cells apart (from 257 points on)"""
    pos = np.full((n, 3), 1.0e6, f32)
    pos[:, 0] = (f32(1.0e6) + 288.0 + np.arange(n) * 0.1875).astype(f32)
    pos[0] = -3.0e7
    return pos, 15.9375


def lattice(n: int, spacing: float = 0.25):
    """a cubic lattice whose spacing IS the radius (a power of two: every d2 is exact): six neighbours at d2 == r2 inside"""
    k = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    return (g * spacing).astype(f32), float(spacing)


def ulp_pairs(n: int, seed: int):
    """pairs a few ulp either side of radius = 1 along every axis, and on each axis the triple 0, 1 - 2^-24, 2: the last two are neighbours in fp32
    (dx rounds to 1) at a real distance above the radius, two cells of width exactly `radius` apart"""
    rng = np.random.default_rng(seed)
    pts = [(0.0, 0.0, 0.0)]
    for axis in range(3):
        for v in (f32(1.0) - ULP1, f32(2.0)):
            p = [0.0, 0.0, 0.0]
            p[axis] = v
            pts.append(tuple(p))
    pts = np.array(pts, f32)
    while len(pts) < n:
        base = (rng.random(3) * 8.0 + 4.0).astype(f32)             # away from the triples
        axis = int(rng.integers(3))
        step = np.zeros(3, f32)
        step[axis] = f32(1.0) + f32(int(rng.integers(-3, 4))) * f32(2.0 ** -23)
        pts = np.concatenate([pts, base[None], (base + step).astype(f32)[None]])
    return pts[:n].astype(f32), 1.0


def outliers(n: int, seed: int):
    """a cloud with floaters scaled by 1e9: the far ones land in clamped cells, two of them close enough to be neighbours there"""
    pos, _ = gaussian(n, seed)
    k = max(n // 50, 4) if n >= 8 else 0
    rng = np.random.default_rng(seed + 1)
    pick = rng.choice(n, k, replace=False) if k else np.zeros(0, np.int64)
    pos[pick] = (pos[pick] * f32(1.0e9)).astype(f32)
    if k:
        pos[pick[1]] = pos[pick[0]]                                # a pair inside a clamped cell (identical: neighbours at any radius)
    return pos, 0.05


def duplicates(n: int, seed: int):
    pos, radius = gaussian(max(n // 3, 1), seed)
    return np.concatenate([pos] * 4)[:n].copy(), radius


def identical(n: int):
    return np.full((n, 3), 0.375, f32), 0.5


def non_finite(n: int, seed: int):
    pos, radius = gaussian(n, seed)
    bad = [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf), (np.inf, np.inf, np.inf), (np.nan, np.nan, np.nan), (np.inf, 0.0, 0.0), (np.inf, 0.0, 0.0)]
    for k, b in enumerate(bad):
        if 3 * k + 1 < n:
            pos[3 * k + 1] = b
    return pos, radius


def adversarial(n: int, seed: int):
    """every family at n points"""
    return [("gaussian",) + gaussian(n, seed), ("far cloud",) + far_cloud(n, seed), ("far line + anchor",) + far_line_with_anchor(n),
            ("lattice at radius",) + lattice(n), ("ulp pairs",) + ulp_pairs(n, seed), ("outliers",) + outliers(n, seed),
            ("duplicates",) + duplicates(n, seed), ("non-finite",) + non_finite(n, seed)]


def isolating_radius(pos) -> float:
    """a radius below every distance of a Gaussian cloud of this size (the caller checks that the model's counts are all 0).  Up to 5,000 points it is
    also small enough for the cloud to overrun the grid: the far cells clamp.  Above that it is not, so that the grid model stays quick"""
    return 1.0e-6 if len(pos) <= 5000 else 1.0e-5


def one_cell_radius(pos) -> float:
    """a radius above the cloud's diameter: one cell, every pair neighbours"""
    p = np.asarray(pos, np.float64)
    return float(f32(2.0 * np.linalg.norm(p.max(axis=0) - p.min(axis=0)) + 1.0))


# ---- driving a renderer ------------------------------------------------------------------------------------------------------------------------------
def raw_counts(lib, r, radius, cap, out, count) -> int:
    """the C call itself (for the refusals): out may be None"""
    return lib.gs_renderer_edit_neighbour_counts(r._r_h if r is not None else None, C.c_float(radius), cap, out.ctypes.data if out is not None else None, count)


def raw_select(lib, r, radius, min_neighbours, subtract=0) -> int:
    return lib.gs_renderer_edit_select_sparse(r._r_h if r is not None else None, C.c_float(radius), min_neighbours, subtract)
