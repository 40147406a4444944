"""The cases of the attribute suites (helper, not a test): a builder of a VeryHigh chunk-less asset from arbitrary per-splat arrays -- its decode is the
identity on every field -- the adversarial family of values, and the raw C calls the refusal tests make.  Imports without a GPU; nothing here makes
a context."""
import ctypes as C
import functools

import numpy as np

import attribute_model as AM
from unitygaussiansplatting_amd import _abi, asset as A, creator

f32 = np.float32
HIST_LO, HIST_HI = 0.125, 0.875                                    # the range the family's bin edges are laid on
FAMILY_BINS = (1, 2, 3, 64, 255, 256, 1000, 4096)
POINT = (0.25, -0.5, 0.125)                                        # q of GS_ATTR_DIST2 in the suites


def attribute_asset(pos, scale, opacity, col):
    """All-fp32, chunk-less asset: position, linear scale, linear opacity and DC colour decode to exactly the arrays given (no chunk, so no
    de-normalisation, no squarings, no InvSquareCentered01).  Colour texels go at creator.SplatIndexToTextureIndex"""
    pos, scale, col = (np.ascontiguousarray(x, f32).reshape(-1, 3) for x in (pos, scale, col))
    opacity = np.ascontiguousarray(opacity, f32).reshape(-1)
    n = len(pos)
    assert len(scale) == len(col) == len(opacity) == n
    other = np.zeros((n, 4), np.uint32)
    other[:, 0] = (511 | (511 << 10) | (511 << 20) | (3 << 30))        # ~identity rotation
    other[:, 1:4] = scale.view(np.uint32)
    w, h = A.CalcTextureSize(n)
    texels = np.zeros((w * h, 4), f32)
    at = creator.SplatIndexToTextureIndex(np.arange(n, dtype=np.uint32))
    texels[at, 0:3] = col
    texels[at, 3] = opacity
    return A.GaussianSplatAsset(splatCount=n, posFormat=A.VectorFormat.Float32, scaleFormat=A.VectorFormat.Float32, shFormat=A.SHFormat.Float32,
                                colorFormat=A.ColorFormat.Float32x4, posData=pos.view(np.uint8).reshape(-1).copy(), otherData=other.view(np.uint8).reshape(-1).copy(),
                                colorData=texels.view(np.uint8).reshape(-1).copy(), shData=np.zeros(n * 192, np.uint8))


def fields_of(pos, scale, opacity, col) -> np.ndarray:
    """the arrays as the columns of Oracle.decode_all() that attribute_model.values reads (the rest zero)"""
    n = len(opacity)
    dec = np.zeros((n, 59), f32)
    dec[:, 0:3], dec[:, 7:10], dec[:, 10], dec[:, 11:14] = pos, scale, opacity, col
    return dec


def plain(n: int, seed: int):
    """(pos, scale, opacity, col) of an ordinary scene: a Gaussian cloud, log-normal scales, opacities piled up at 0 and 1, colours on 256 levels"""
    rng = np.random.default_rng(seed)
    pos = rng.standard_normal((n, 3)).astype(f32)
    scale = np.exp(rng.normal(-4.0, 0.8, (n, 3))).astype(f32)
    opacity = np.clip(rng.normal(0.5, 0.6, n), 0.0, 1.0).astype(f32)
    col = (rng.integers(0, 256, (n, 3)).astype(f32) * f32(1.0 / 255.0)).astype(f32)
    return pos, scale, opacity, col


def bin_edge_values(lo=HIST_LO, hi=HIST_HI, bins_list=FAMILY_BINS, per_bins: int = 12, seed: int = 1) -> np.ndarray:
    """exactly lo and hi, and for every bin count a sample of its edges lo + k (hi - lo) / bins with the floats up to three ulp either side"""
    rng = np.random.default_rng(seed)
    out = [f32(lo), f32(hi)]
    for bins in bins_list:
        ks = {0, 1, bins - 1, bins} | set(int(k) for k in rng.integers(0, bins + 1, per_bins))
        for k in sorted(ks):
            e = f32(lo + k * (hi - lo) / bins)
            down = up = e
            out.append(e)
            for _ in range(3):
                down, up = np.nextafter(down, f32(-np.inf)), np.nextafter(up, f32(np.inf))
                out += [down, up]
    return np.array(out, f32)


SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, -1.0, -0.25, 1e-20, -1e-20, 1e20, -1e20, 3e38, 1e-13, 1e13, 1.0, 0.5], f32)


@functools.lru_cache(maxsize=None)
def adversarial(n: int = 1500, seed: int = 3):
    """(pos, scale, opacity, col): an ordinary scene with, in every field, NaN, +-inf, +-0, denormals, negatives, values whose product under- and
    overflows (1e-20 and 1e20 cubed, 3e38 x 3e38), the bin-edge values of bin_edge_values() and the triples that tell a fused sum from a rounded one;
    scale triples that are all NaN, all -0 / +0 in both orders, and NaN beside a number.  Shared and left unchanged"""
    rng = np.random.default_rng(seed)
    pos, scale, opacity, col = plain(n, seed)
    edges = bin_edge_values()
    pick = lambda shape: np.where(rng.random(shape) < 0.5, rng.choice(SPECIALS, shape), rng.choice(edges, shape)).astype(f32)      # half specials, half edge values
    m = rng.random(n) < 0.45; opacity[m] = pick(int(m.sum()))
    m = rng.random(n) < 0.35; scale[m] = pick((int(m.sum()), 3))
    m = rng.random(n) < 0.35; col[m] = pick((int(m.sum()), 3))
    m = rng.random(n) < 0.25; pos[m] = pick((int(m.sum()), 3))
    crafted = np.array([[np.nan, np.nan, np.nan], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [-0.0, -0.0, 0.0], [np.nan, 2.0, np.nan], [2.0, np.nan, 3.0], [np.nan, np.nan, -1.0],
                        [1e-20, 1e-20, 1e-20], [1e20, 1e20, 1e20], [3e38, 3e38, 1e-38], [1e-30, 1e-30, 1e38], [np.inf, 0.0, 1.0], [-np.inf, np.inf, 1.0],
                        [1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -22], [0.1, 0.7, 0.3], [1e-13, 1e-13, 1e-13], [np.inf, np.inf, np.inf], [np.inf, np.nan, np.inf],
                        [-np.inf, -np.inf, -np.inf]], f32)
    k = len(crafted)
    assert n >= 4 * k + len(edges)
    scale[:k], col[k:2 * k], pos[2 * k:3 * k] = crafted, crafted, crafted
    opacity[3 * k:3 * k + len(edges)] = edges                      # every edge value at least once
    for x in (pos, scale, opacity, col):
        x.setflags(write=False)
    return pos, scale, opacity, col


def all_equal(n: int, value: float = 0.375):
    """every field of every splat the same value: one bin takes everything"""
    return np.full((n, 3), value, f32), np.full((n, 3), value, f32), np.full(n, value, f32), np.full((n, 3), value, f32)


# ---- driving a renderer: the C calls themselves (for the refusals); pointers may be None -----------------------------------------------------------------
def _h(r):
    return r._r_h if r is not None else None


def _a(x):
    return x.ctypes.data if x is not None else None


def raw_values(lib, r, attr, point, out, count) -> int:
    return lib.gs_renderer_edit_attribute_values(_h(r), attr, _a(point), _a(out), count)


def raw_select(lib, r, attr, point, lo, hi, subtract=0) -> int:
    return lib.gs_renderer_edit_select_range(_h(r), attr, _a(point), C.c_float(lo), C.c_float(hi), subtract)


def raw_stats(lib, r, attr, point, scope, out) -> int:
    return lib.gs_renderer_edit_attribute_stats(_h(r), attr, _a(point), scope, C.byref(out) if out is not None else None)


def raw_histogram(lib, r, attr, point, scope, lo, hi, bins, out, count) -> int:
    return lib.gs_renderer_edit_attribute_histogram(_h(r), attr, _a(point), scope, C.c_float(lo), C.c_float(hi), bins, _a(out), count)


def raw_ranks(lib, r, attr, point, scope, ranks, rank_count, out, population) -> int:
    return lib.gs_renderer_edit_attribute_ranks(_h(r), attr, _a(point), scope, _a(ranks), rank_count, _a(out), C.byref(population) if population is not None else None)


def stats_tuple(s: _abi.gs_attribute_stats):
    """(members, nans, vmin bits, vmax bits): the form attribute_model.stats gives"""
    return int(s.members), int(s.nans), int(f32(s.vmin).view(np.uint32)), int(f32(s.vmax).view(np.uint32))
