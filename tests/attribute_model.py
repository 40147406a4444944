"""The numpy twin of the attribute tools -- gs_renderer_edit_attribute_values / _select_range / _attribute_stats / _attribute_histogram / _attribute_ranks
(helper, not a test): the contract of DESIGN.md section 4.19 restated operation by operation in fp32 numpy, so that it gives the same bits and integers
as the kernels.  The fields are the columns of Oracle.decode_all(): pos 0:3, scale 7:10, opacity 10, col 11:14 (builders.decode_of shares the decodes).

Alive is the rule of the existing models (neighbour_model.alive_flags): index < N, not deleted, not cut."""
from __future__ import annotations

import numpy as np

f32 = np.float32
NOT_ALIVE = 0xFFFFFFFF
OPACITY, SCALE_MAX, SCALE_MIN, VOLUME, POS_X, POS_Y, POS_Z, DIST2, COLOR_R, COLOR_G, COLOR_B, LUMA = range(12)
ATTRS = tuple(range(12))
CLASS_OF = {OPACITY: "opacity", SCALE_MAX: "scale", SCALE_MIN: "scale", VOLUME: "scale", POS_X: "pos", POS_Y: "pos", POS_Z: "pos", DIST2: "pos",
            COLOR_R: "colour", COLOR_G: "colour", COLOR_B: "colour", LUMA: "colour"}
ONE_PER_CLASS = (OPACITY, VOLUME, DIST2, LUMA)
MAX_BINS = MAX_RANKS = 4096


def fmax(a, b):
    """fmaxf with the +-0 tie pinned to the first operand: a NaN operand is ignored, NaN if both are (np.fmax wherever the operands are not +0 and -0)"""
    with np.errstate(invalid="ignore"):
        return np.where((a >= b) | np.isnan(b), a, b).astype(f32)


def fmin(a, b):
    with np.errstate(invalid="ignore"):
        return np.where((a <= b) | np.isnan(b), a, b).astype(f32)


def values(dec, attr: int, point=None) -> np.ndarray:
    """value(i, attr) of every splat from the decoded fields, fp32, one rounding per operation, nothing fused"""
    dec = np.asarray(dec, f32)
    p, s, o, c = dec[:, 0:3], dec[:, 7:10], dec[:, 10], dec[:, 11:14]
    with np.errstate(all="ignore"):
        if attr == OPACITY:
            return o.copy()
        if attr == SCALE_MAX:
            return fmax(fmax(s[:, 0], s[:, 1]), s[:, 2])
        if attr == SCALE_MIN:
            return fmin(fmin(s[:, 0], s[:, 1]), s[:, 2])
        if attr == VOLUME:
            return ((s[:, 0] * s[:, 1]).astype(f32) * s[:, 2]).astype(f32)
        if attr in (POS_X, POS_Y, POS_Z):
            return p[:, attr - POS_X].copy()
        if attr == DIST2:
            q = np.asarray(point, f32).reshape(3)
            dx, dy, dz = (p[:, 0] - q[0]).astype(f32), (p[:, 1] - q[1]).astype(f32), (p[:, 2] - q[2]).astype(f32)
            return (((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)).astype(f32)
        if attr in (COLOR_R, COLOR_G, COLOR_B):
            return c[:, attr - COLOR_R].copy()
        if attr == LUMA:
            return (((f32(0.299) * c[:, 0]).astype(f32) + (f32(0.587) * c[:, 1]).astype(f32)).astype(f32) + (f32(0.114) * c[:, 2]).astype(f32)).astype(f32)
    raise ValueError(attr)


def value_words(v, alive) -> np.ndarray:
    """what gs_renderer_edit_attribute_values writes: the value's bits for an alive splat, 0xFFFFFFFF for every other one"""
    out = np.ascontiguousarray(v, f32).view(np.uint32).copy()
    out[~np.asarray(alive, bool)] = NOT_ALIVE
    return out


def same_words(got, want) -> np.ndarray:
    """per word: the same bits -- or a NaN value on both sides (its sign and payload carry no meaning), which the all-ones word never stands for"""
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    both_nan = np.isnan(g.view(f32)) & np.isnan(w.view(f32)) & (g != NOT_ALIVE) & (w != NOT_ALIVE)
    return (g == w) | both_nan


def keys(v) -> np.ndarray:
    """KEY = FloatToSortableUint(value): a total order, -0 before +0"""
    u = np.ascontiguousarray(v, f32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_values(k) -> np.ndarray:
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(f32)


def scope_flags(alive, selected_words=None, selected_only: bool = False) -> np.ndarray:
    """the members: the alive splats, or those of them whose selected bit is set (bits at or beyond N never count; no words: nobody)"""
    alive = np.asarray(alive, bool)
    if not selected_only:
        return alive.copy()
    if selected_words is None:
        return np.zeros(len(alive), bool)
    sel = np.unpackbits(np.ascontiguousarray(selected_words, np.uint32).view(np.uint8), bitorder="little")[:len(alive)].astype(bool)
    return alive & sel


def in_range(v, lo, hi) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (f32(lo) <= v) & (v <= f32(hi))


def pack_bits(flags, n_words: int) -> np.ndarray:
    m = np.zeros(n_words * 32, np.uint8)
    m[:len(flags)] = np.asarray(flags, bool)
    return np.packbits(m, bitorder="little").view(np.uint32).copy()


def select_range(selected_words, v, alive, lo, hi, subtract: bool = False) -> np.ndarray:
    """the selection words after gs_renderer_edit_select_range: |= in, or &= ~in; no bit at or beyond N comes from it"""
    sel = np.ascontiguousarray(selected_words, np.uint32).copy()
    w = pack_bits(np.asarray(alive, bool) & in_range(v, lo, hi), len(sel))
    return (sel & ~w) if subtract else (sel | w)


def stats(v, members):
    """(members, nans, vmin bits, vmax bits): the non-NaN members of smallest / largest KEY; +inf / -inf if there is none"""
    v = np.ascontiguousarray(v, f32)[np.asarray(members, bool)]
    nan = np.isnan(v)
    k = keys(v[~nan])
    if len(k) == 0:
        return len(v), int(nan.sum()), int(f32(np.inf).view(np.uint32)), int(f32(-np.inf).view(np.uint32))
    return len(v), int(nan.sum()), int(key_values(k.min()).view(np.uint32)), int(key_values(k.max()).view(np.uint32))


def hist_scale(lo, hi, bins: int):
    """s = (float) bins / (hi - lo) in fp32, or None where the call is refused"""
    lo, hi = f32(lo), f32(hi)
    if not (1 <= int(bins) <= MAX_BINS) or not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        return None
    with np.errstate(all="ignore"):
        w = f32(hi - lo)
        if not np.isfinite(w):
            return None
        s = f32(f32(bins) / w)
    return s if np.isfinite(s) else None


def bin_of(v, lo, hi, bins: int) -> np.ndarray:
    """the word of the bins + 3 a value is counted in: NaN -> bins + 2, v < lo -> bins, v > hi -> bins + 1, else min(bins - 1, (uint32)((v - lo) * s))"""
    v = np.ascontiguousarray(v, f32)
    lo, hi, s = f32(lo), f32(hi), hist_scale(lo, hi, bins)
    assert s is not None
    out = np.zeros(len(v), np.int64)
    with np.errstate(invalid="ignore"):
        nan, below, above = np.isnan(v), v < lo, v > hi
    inside = ~(nan | below | above)
    t = ((v[inside] - lo).astype(f32) * s).astype(f32)
    out[inside] = np.minimum(t.astype(np.uint32).astype(np.int64), bins - 1)
    out[nan], out[below], out[above] = bins + 2, bins, bins + 1
    return out


def histogram(v, members, lo, hi, bins: int) -> np.ndarray:
    return np.bincount(bin_of(np.ascontiguousarray(v, f32)[np.asarray(members, bool)], lo, hi, bins), minlength=bins + 3).astype(np.uint32)


def population_keys(v, members) -> np.ndarray:
    """the sorted KEYs of the members whose value is not NaN"""
    v = np.ascontiguousarray(v, f32)[np.asarray(members, bool)]
    return np.sort(keys(v[~np.isnan(v)]))


def ranks(v, members, rank_list):
    """(the words of values_out, the population)"""
    k = population_keys(v, members)
    r = np.asarray(rank_list, np.int64).reshape(-1)
    out = np.full(len(r), NOT_ALIVE, np.uint32)
    ok = r < len(k)
    out[ok] = key_values(k[r[ok]]).view(np.uint32)
    return out, len(k)


def quantile_ranks(fractions, population: int) -> np.ndarray:
    return np.minimum(population - 1, np.floor(np.asarray(fractions, np.float64) * np.float64(population))).astype(np.uint32)
