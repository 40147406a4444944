"""The yardstick of the screen mask (helper, not a test): a numpy float32 twin of what gs_mask_fill_polygon and gs_mask_stroke leave in a mask and of the
two calls that select through one, written straight from the contract of include/gsplat_c.h.

Coverage is brute force: every pixel centre against every edge / every segment, one rounding per operation (numpy float32 arrays and scalars never widen) --
no boxes, no boundary counts, no scans.  A mask here is an H x W bool array, row 0 = top; words() packs it the way gs_mask_download hands it out.

The selection twins stand on tests/edit_model.py: its clip positions (the oracle's), its cut flags and its pixel_positions -- the projection twin of the
rectangle tool -- followed by the mask's own comparison: px >= 0 && px < W && py >= 0 && py < H, then bit ((uint)px, H - 1 - (uint)py)."""
from __future__ import annotations

import numpy as np

import edit_model as EM

f32 = np.float32
COORD_MAX = 65536.0
MAX_POINTS = 65536


def row_words(w: int) -> int:
    return (w + 31) // 32


def words(mask: np.ndarray) -> np.ndarray:
    """H x W bool -> H x ceil(W/32) words, bit x & 31 of word x >> 5 = pixel x, the bits beyond W zero"""
    m = np.asarray(mask, bool)
    h, w = m.shape
    padded = np.zeros((h, row_words(w) * 32), np.uint8)
    padded[:, :w] = m
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(h, row_words(w)).copy()


def from_words(wd: np.ndarray, w: int) -> np.ndarray:
    wd = np.ascontiguousarray(wd, np.uint32)
    return np.unpackbits(wd.view(np.uint8), axis=1, bitorder="little")[:, :w].astype(bool)


def padding_bits(wd: np.ndarray, w: int) -> int:
    """the bits beyond W that are set (must be none)"""
    return int(np.unpackbits(np.ascontiguousarray(wd, np.uint32).view(np.uint8), axis=1, bitorder="little")[:, w:].sum())


def centres(n: int) -> np.ndarray:
    return (np.arange(n, dtype=f32) + f32(0.5)).astype(f32)


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------------------
def polygon_coverage(w: int, h: int, points) -> np.ndarray:
    """even-odd: on the row yc the edge (a -> b) crosses iff (a.y <= yc) != (b.y <= yc), at xs = a.x + ((yc - a.y) * (b.x - a.x)) / (b.y - a.y), and toggles
    every pixel with xc < xs"""
    p = np.ascontiguousarray(points, f32).reshape(-1, 2)
    xc, yc = centres(w), centres(h)
    cov = np.zeros((h, w), bool)
    for i in range(len(p)):
        a, b = p[i], p[(i + 1) % len(p)]
        rows = np.flatnonzero((a[1] <= yc) != (b[1] <= yc))
        if not len(rows):
            continue
        xs = (a[0] + ((yc[rows] - a[1]) * (b[0] - a[0])) / (b[1] - a[1])).astype(f32)
        assert xs.dtype == f32
        cov[rows] ^= xc[None, :] < xs[:, None]
    return cov


def segments(points):
    p = np.ascontiguousarray(points, f32).reshape(-1, 2)
    return [(p[0], p[0])] if len(p) == 1 else [(p[i], p[i + 1]) for i in range(len(p) - 1)]


def stroke_coverage(w: int, h: int, points, radius: float) -> np.ndarray:
    """d = b - a, e = c - a, len2 = d.d; t = 0 if len2 == 0 else min(max(e.d / len2, 0), 1); q = e - t d; covered iff q.q <= radius radius for any segment"""
    cx, cy = np.meshgrid(centres(w), centres(h))
    r2 = f32(radius) * f32(radius)
    cov = np.zeros((h, w), bool)
    for a, b in segments(points):
        dx, dy = b[0] - a[0], b[1] - a[1]
        ex, ey = cx - a[0], cy - a[1]
        len2 = dx * dx + dy * dy
        if len2 == f32(0.0):
            t = np.zeros((h, w), f32)
        else:
            t = np.minimum(np.maximum((ex * dx + ey * dy) / len2, f32(0.0)), f32(1.0))
        qx, qy = ex - t * dx, ey - t * dy
        d2 = qx * qx + qy * qy
        assert d2.dtype == f32
        cov |= d2 <= r2
    return cov


def apply(mask: np.ndarray, cov: np.ndarray, subtract: bool) -> np.ndarray:
    return (mask & ~cov) if subtract else (mask | cov)


def refused(points, lo: int, radius=None) -> bool:
    """what both drawing calls refuse: the count, a coordinate that is not finite or beyond 65536 in magnitude, a radius outside (0, 65536]"""
    p = np.asarray(points, f32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        bad = not (lo <= len(p) <= MAX_POINTS) or not bool((np.abs(p) <= f32(COORD_MAX)).all())
        if radius is not None:
            bad = bad or not (f32(radius) > 0 and f32(radius) <= f32(COORD_MAX))
    return bad


# ---- the two selecting calls ------------------------------------------------------------------------------------------------------------------------
def mask_hit_flags(clip: np.ndarray, cut: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """gs_renderer_edit_update_selection_mask's test of every splat: CSSelectionUpdate's early-outs, then the mask's bit under the pixel position"""
    H, W = mask.shape
    cw = clip[:, 3].astype(f32)
    px, py = EM.pixel_positions(clip, W, H)
    with np.errstate(invalid="ignore"):
        behind = cw <= f32(0.0)
        inside = (px >= f32(0.0)) & (px < f32(W)) & (py >= f32(0.0)) & (py < f32(H))      # a NaN is inside nothing
    hit = np.zeros(len(clip), bool)
    xi, yi = px[inside].astype(np.uint32), py[inside].astype(np.uint32)                       # truncation
    hit[inside] = mask[H - 1 - yi.astype(np.int64), xi.astype(np.int64)]
    return ~np.asarray(cut, bool) & ~behind & hit


def update_selection_mask(model: EM.EditModel, P, mask: np.ndarray, subtract: bool) -> None:
    """on an EditModel, as its update_selection: selected = mouse-down copy, plus or minus the hits"""
    assert mask.shape == (int(P.screen_h), int(P.screen_w))
    model._ensure()
    hw = EM.pack_bits(mask_hit_flags(model.clip_positions(P), model.cut, mask), model.nw)
    model.sel = (model.md & ~hw) if subtract else (model.md | hw)


def select_surface_mask(records: np.ndarray, selected: np.ndarray, mask: np.ndarray, tag: int, n: int, deleted=None, cut=None, subtract: bool = False) -> np.ndarray:
    """pick_model.select_surface with the pixels of the mask in place of the rectangle's"""
    assert records.shape == mask.shape
    sel = np.ascontiguousarray(selected, np.uint32).copy()
    r = records[np.asarray(mask, bool)]
    s = r["splat"][(r["tag"] == tag) & (r["splat"] < n)].astype(np.int64)
    if deleted is not None:
        s = s[((np.asarray(deleted, np.uint32)[s >> 5] >> (s & 31).astype(np.uint32)) & 1) == 0]
    if cut is not None:
        s = s[~np.asarray(cut, bool)[s]]
    s = np.unique(s)
    bits = np.zeros(len(sel), np.uint32)
    np.bitwise_or.at(bits, s >> 5, (np.uint32(1) << (s & 31).astype(np.uint32)))
    return (sel & ~bits) if subtract else (sel | bits)


def rect_of_mask_box(x0: int, y0: int, x1: int, y1: int, H: int):
    """the rectangle of gs_renderer_edit_update_selection that hits what a mask with exactly the pixels [x0, x1] x [y0, y1] (y down) set hits, for finite
    pixel positions: px in [x0, x1 + 1), py in [H - 1 - y1, H - y0)"""
    return (f32(x0), f32(H - 1 - y1), np.nextafter(f32(x1 + 1), f32(-np.inf)), np.nextafter(f32(H - y0), f32(-np.inf)))


# ---- shared cases ---------------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (31, 3), (32, 2), (33, 2), (257, 65)]
BIG = (1200, 797)
EDGE_BATCH = 256                                                   # gs_mask.hip's kMaskEdgeBatch


def scaled(shape, w: int, h: int) -> np.ndarray:
    """a unit-square shape (points in [0, 1]^2) laid over the screen with a margin"""
    s = np.asarray(shape, np.float64)
    return (s * [w * 0.8, h * 0.8] + [w * 0.1 + 0.13, h * 0.1 + 0.29]).astype(f32)


TRIANGLE = [(0.1, 0.05), (0.95, 0.4), (0.3, 1.0)]
CONCAVE_L = [(0, 0), (1, 0), (1, 0.35), (0.4, 0.35), (0.4, 1), (0, 1)]
BOW_TIE = [(0, 0), (1, 1), (1, 0), (0, 1)]
PENTAGRAM = [(0.5 + 0.5 * np.sin(2 * np.pi * (2 * k) / 5), 0.5 - 0.5 * np.cos(2 * np.pi * (2 * k) / 5)) for k in range(5)]


def radial_lasso(w: int, h: int, count: int, seed: int) -> np.ndarray:
    """a seeded star-shaped outline around the screen centre, partly off screen"""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.random(count)) * 2 * np.pi
    rad = 0.15 + 0.45 * rng.random(count)
    return np.stack([w * (0.5 + rad * np.cos(ang) * 1.1), h * (0.5 + rad * np.sin(ang) * 1.1)], axis=1).astype(f32)


def random_stroke(w: int, h: int, points: int, seed: int) -> np.ndarray:
    """a seeded random walk that stays near the screen, with a few repeated points (zero-length segments)"""
    rng = np.random.default_rng(seed)
    step = rng.normal(0.0, max(w, h) / 40.0, (points, 2))
    p = np.cumsum(step, axis=0) + [w / 2, h / 2]
    p = np.stack([np.abs((p[:, 0] + w * 0.2) % (2.8 * w) - 1.4 * w) - 0.2 * w, np.abs((p[:, 1] + h * 0.2) % (2.8 * h) - 1.4 * h) - 0.2 * h], axis=1)
    p[5::97] = p[4::97][:len(p[5::97])]
    return p.astype(f32)


def polygon_cases(w: int, h: int):
    """(name, points) for a w x h screen"""
    out = [("triangle", scaled(TRIANGLE, w, h)), ("concave L", scaled(CONCAVE_L, w, h)), ("bow-tie", scaled(BOW_TIE, w, h)), ("pentagram", scaled(PENTAGRAM, w, h)),
           ("on pixel centres", np.array([(0.5, 0.5), (w - 0.5, 0.5), (w - 0.5, h - 0.5), (w // 2 + 0.5, h // 2 + 0.5), (0.5, h - 0.5)], f32)),
           ("on row centres", np.array([(-3.25, 0.5), (w + 2.75, 1.5), (w / 3, h - 0.5), (w / 5, h / 2 + 0.5)], f32)),
           ("off screen", np.array([(w + 5, h + 5), (w + 50, h + 9), (w + 20, h + 70)], f32)),
           ("off screen to the left", np.array([(-50, -3), (-2, h / 2), (-40, h + 8)], f32)),
           ("around the screen", np.array([(-10, -10), (w + 10, -10), (w + 10, h + 10), (-10, h + 10)], f32)),
           ("at the coordinate limit", np.array([(-65536, -65536), (65536, -60000), (65536, 65536), (-100, 65536)], f32))]
    for count in (3, EDGE_BATCH - 1, EDGE_BATCH, EDGE_BATCH + 1, 4097):
        out.append((f"radial lasso {count}", radial_lasso(w, h, count, 100 + count)))
    return out


def stroke_cases(w: int, h: int):
    """(name, points, radius)"""
    cx, cy = w // 2 + 0.5, h // 2 + 0.5
    big = 2.0 * max(w, h)
    return [("one point, radius 0.5", np.array([(cx, cy)], f32), 0.5),
            ("one point off screen", np.array([(-40.0, -40.0)], f32), 7.0),
            ("one point between centres", np.array([(cx + 0.5, cy + 0.5)], f32), 0.70710678),
            ("zero-length segments", np.array([(2.2, 1.1), (2.2, 1.1), (w - 1.7, h - 0.6), (w - 1.7, h - 0.6), (w / 2, 0.3)], f32), 1.3),
            ("radius larger than the screen", np.array([(w / 3, h / 3), (w / 2, h / 2)], f32), big),
            ("far away, radius reaches", np.array([(-3.0 * big, h / 2), (-2.5 * big, h / 3)], f32), 2.5 * big + 3.3),
            ("clipped left", np.array([(-6.5, h * 0.25), (3.0, h * 0.75)], f32), 2.6),
            ("clipped right", np.array([(w - 2.5, h * 0.2), (w + 8.0, h * 0.9)], f32), 3.1),
            ("clipped top", np.array([(w * 0.2, -5.0), (w * 0.8, 1.5)], f32), 2.2),
            ("clipped bottom", np.array([(w * 0.1, h + 4.0), (w * 0.7, h - 1.5)], f32), 2.9),
            ("tiny radius", np.array([(cx, cy), (cx + 3.0, cy)], f32), 1.0e-30)]
