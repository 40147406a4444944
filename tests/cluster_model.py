"""The Lloyd loop of the Cluster* SH palette in numpy (helper, not a test): the contract of gs_import_cluster_shs restated without any of the code it
checks.  The nearest-mean assignment goes through gs_import_assign_clusters(NULL, ...) -- the host loop tests/test_import_cluster.py holds to a
term-by-term restatement -- or through any function handed in its place; the sums are np.add.at in float64, which adds strictly in point order.
Shared by tests/test_cluster_shs.py (CPU) and tests/test_gpu_cluster_shs.py (-m gpu)."""
from __future__ import annotations

import numpy as np

from unitygaussiansplatting_amd import creator

f32 = np.float32
DIM = 45
SUBSET = 200_000
PASSES = 4


def seeds(x: np.ndarray, k: int) -> np.ndarray:
    """means[j] = x[(j n) / k], 64-bit product"""
    return x[(np.arange(k, dtype=np.int64) * len(x)) // k].copy()


def subset(x: np.ndarray) -> np.ndarray:
    return x if len(x) <= SUBSET else x[(np.arange(SUBSET, dtype=np.int64) * len(x)) // SUBSET]


def mean_update(sub: np.ndarray, idx: np.ndarray, means: np.ndarray) -> np.ndarray:
    """for every cluster with points: sum = 0.0, then sum = sum + (double)sub[p] over its points in ascending p, mean = (float)(sum / (double)count);
    a cluster without points keeps its mean"""
    k = len(means)
    sums = np.zeros((k, DIM), np.float64)
    np.add.at(sums, idx.astype(np.int64), sub.astype(np.float64))        # unbuffered: one add per point, in point order
    cnt = np.bincount(idx.astype(np.int64), minlength=k)
    out = means.copy()
    nz = cnt > 0
    out[nz] = (sums[nz] / cnt[nz, None].astype(np.float64)).astype(f32)
    return out


def lloyd(x, k: int, assign=creator.AssignClusters):
    """(means [k, 45] float32, index [n] uint32, the cluster sizes of every Lloyd pass [4, k])"""
    x = np.ascontiguousarray(x, f32).reshape(-1, DIM)
    assert np.isfinite(x).all()                                         # the byte contract holds for finite values only
    means = seeds(x, k)
    sub = subset(x)
    cnt = []
    for _ in range(PASSES):
        idx = assign(sub, means)
        cnt.append(np.bincount(idx.astype(np.int64), minlength=k))
        means = mean_update(sub, idx, means)
    return means, np.asarray(assign(x, means), np.uint32), np.stack(cnt)


def random_points(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((n, DIM)).astype(f32)


def clumped_points(n: int, seed: int, big: float = 0.4, small: float = 0.1) -> np.ndarray:
    """random points in which a contiguous run of big * n rows repeats one row and a strided set of small * n rows another: the stride-sampled seeds
    inside the run are equal, the lowest of them wins every tie, so the others' clusters are empty and one cluster holds the whole run"""
    x = random_points(n, seed)
    a, b = int(n * 0.1), int(n * 0.1) + int(n * big)
    x[a:b] = x[a]
    rows = b + 3 * np.arange(int(n * small))
    rows = rows[rows < n]
    x[rows] = x[n - 1]
    return x


def crafted_decode(n: int = 6000, big: int = 2500, small: int = 500, seed: int = 17) -> np.ndarray:
    """the oracle's decode [n, 59] of small_asset(n, 5, "VeryHigh") with the SH (columns 14:59) of `big` randomly placed rows replaced by one row's and
    of `small` others by another's: with K = 4,096 the stride-sampled seeds repeat, about two thousand clusters never get a point and one holds `big`"""
    import copy_model
    from common import small_asset
    dec = copy_model.decode(small_asset(n, 5, "VeryHigh")).copy()
    rows = np.random.default_rng(seed).permutation(n)
    dec[rows[:big], 14:59] = dec[rows[0], 14:59]
    dec[rows[big:big + small], 14:59] = dec[rows[big], 14:59]
    return dec
