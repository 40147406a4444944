"""Inputs and the strict numpy restatement for the nearest-mean assignment of the importer's Cluster* SH palette
(gs_import_assign_clusters; csrc/gs_import.cpp assign_clusters on the host, csrc/gs_cluster.hip on the GPU).  Shared by
tests/test_import_cluster.py (CPU) and tests/test_gpu_import_cluster.py (-m gpu)."""
from __future__ import annotations

import numpy as np

f32 = np.float32
DIM = 45


def reference_assign(x: np.ndarray, m: np.ndarray) -> np.ndarray:
    """The contract, restated: dot accumulated term by term in float64 (product rounded, then the sum; no matrix product, whose
    summation order is the BLAS's), c2 the same sequential sum of m*m, d = c2 - 2 dot; index 0 if d_0 is NaN, else the smallest j
    attaining the minimum over the non-NaN d_j -- what the scan `best = 0; bd = d_0; for j >= 1: if d_j < bd: take j` gives."""
    x64, m64 = np.asarray(x, f32).astype(np.float64), np.asarray(m, f32).astype(np.float64)
    dot = np.zeros((len(x64), len(m64)), np.float64)
    c2 = np.zeros(len(m64), np.float64)
    with np.errstate(all="ignore"):
        for k in range(DIM):
            dot += x64[:, k, None] * m64[None, :, k]
            c2 += m64[:, k] * m64[:, k]
        d = c2[None, :] - 2.0 * dot
    first_min = np.where(np.isnan(d), np.inf, d).argmin(axis=1)          # argmin: the first of equal minima
    return np.where(np.isnan(d[:, 0]), 0, first_min).astype(np.uint32)


def random_case(n: int, k: int, seed: int):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, DIM)).astype(f32), rng.standard_normal((k, DIM)).astype(f32)


def points_near_means(m: np.ndarray, n: int, seed: int, noise: float = 0.05) -> np.ndarray:
    """n points, each a mean of m (cycled through a shuffled order, so every tile of means is some point's answer) plus a little noise."""
    rng = np.random.default_rng(seed)
    pick = rng.permutation(len(m))[np.arange(n) % len(m)]
    return (m[pick] + noise * rng.standard_normal((n, DIM))).astype(f32)


def special_cases():
    """name -> (x, means): the inputs whose distances are not ordinary numbers.  Small: every one is checked against reference_assign."""
    out = {}
    x, m = random_case(257, 63, 11)
    mm = m.copy()
    mm[[5, 17, 40, 62]] = m[[2, 2, 39, 0]]                               # duplicated means: the lower row must win
    out["duplicated_means"] = (points_near_means(mm, 257, 12), mm)
    xx = x.copy()
    xx[::7, 3] = np.nan                                                  # every d of such a point is NaN: index 0
    xx[5, 44] = np.nan
    out["nan_in_x"] = (xx, m)
    mm = m.copy()
    mm[[1, 7, 33, 62], [0, 44, 20, 9]] = np.nan                          # those means can never win; the rest compete as usual
    out["nan_in_means"] = (points_near_means(m, 257, 13), mm)
    mm = m.copy()
    mm[0, 10] = np.nan                                                   # d_0 is NaN for every point: the scan never leaves 0
    out["nan_in_row0"] = (points_near_means(m, 257, 14), mm)
    mm = m.copy()
    mm[1:, 2] = np.nan                                                   # only d_0 is a number
    out["nan_everywhere_but_row0"] = (x, mm)
    xx = x.copy()
    xx[::5, 7] = np.inf                                                  # dot = +-inf: d = -+inf, so the winner is the first mean with the right sign in column 7
    xx[1::5, 30] = -np.inf
    xx[2::25, 8] = np.inf                                                # together with column 7 at rows 2, 27, ...: inf - inf inside the sum -> NaN
    out["inf_in_x"] = (xx, m)
    mm = m.copy()
    mm[[4, 9], [1, 2]] = [np.inf, -np.inf]                               # c2 = inf, dot = +-inf: d = NaN or +inf
    mm[20, 5] = np.inf
    out["inf_in_means"] = (x, mm)
    mm = m.copy()
    mm[0, 1] = np.inf                                                    # d_0 = +inf or NaN by the sign of x[:, 1]
    out["inf_in_row0"] = (x, mm)
    xx = x.copy()
    xx[::3] = np.inf                                                     # every product infinite
    out["all_inf_points"] = (xx, np.abs(m))                              # |m|: dot = +inf, d = -inf for every mean: an all-way tie at -inf, index 0
    tiny = f32(1e-40)                                                    # fp32 denormal scale (min normal 1.18e-38)
    out["denormal_points"] = ((points_near_means(m, 257, 15) * tiny).astype(f32), m)
    out["denormal_means"] = (x, (m * tiny).astype(f32))
    out["denormal_both"] = ((points_near_means(m, 257, 16) * tiny).astype(f32), (m * tiny).astype(f32))
    for name, (a, b) in out.items():
        assert a.dtype == f32 and b.dtype == f32 and a.shape[1] == DIM and b.shape[1] == DIM, name
    assert np.any((np.abs(out["denormal_both"][1]) > 0) & (np.abs(out["denormal_both"][1]) < np.finfo(f32).tiny))
    return out
