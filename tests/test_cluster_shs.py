"""gs_import_cluster_shs(NULL, ...) -- cluster_shs of csrc/gs_import.cpp, the importer's whole SH palette, exposed as it is -- against the numpy Lloyd
loop of tests/cluster_model.py: means and indices bit for bit.  The sizes straddle the assignment's tiles of 64 and include n <= k (the seeds repeat);
200,001 points take the stride-sampled training subset; the clumped case reaches the empty clusters and one long cluster, which random points never
do.  CPU only; the same shapes run on the GPU in tests/test_gpu_cluster_shs.py."""
import numpy as np
import pytest

import cluster_model as CM
from common import same_bits
from unitygaussiansplatting_amd import _abi, _lib, creator

f32 = np.float32


def check(x, k):
    want_means, want_index, cnt = CM.lloyd(x, k)
    means, index = creator.ClusterSHsNative(x, k)
    assert means.shape == (k, 45) and means.dtype == f32 and index.shape == (len(x),) and index.dtype == np.uint32
    assert same_bits(means, want_means, dtype=None), np.flatnonzero((means.view(np.uint32) != want_means.view(np.uint32)).any(axis=1))[:8]
    assert np.array_equal(index, want_index)
    return cnt


@pytest.mark.parametrize("k", [1, 2, 63, 65])
@pytest.mark.parametrize("n", [1, 63, 257, 1_037])
def test_host_route_equals_the_model(n, k):
    check(CM.random_points(n, 100 * n + k), k)


def test_host_route_takes_the_training_subset():
    x = CM.random_points(200_001, 7)
    assert len(CM.subset(x)) == 200_000 and same_bits(CM.subset(x)[-1], x[199_999], dtype=None) and same_bits(CM.subset(x)[100_000], x[100_000], dtype=None)
    check(x, 64)


def test_host_route_empty_and_long_clusters():
    """a run of equal rows: the seeds inside it tie, the lowest takes every one of its points, the others' clusters stay empty and keep their means"""
    n, k = 1_037, 65
    x = CM.clumped_points(n, 3)
    cnt = check(x, k)
    assert ((cnt == 0).sum(axis=1) >= 20).all() and (cnt.max(axis=1) >= int(n * 0.4)).all()
    means, _ = creator.ClusterSHsNative(x, k)
    empty = np.flatnonzero((cnt == 0).all(axis=0))
    assert len(empty) >= 20 and same_bits(means[empty], CM.seeds(x, k)[empty], dtype=None)     # empty in all four passes: still its seed


def test_host_route_crafted_scene():
    """the SH rows of the crafted scene the GPU bake is tested on (tests/test_gpu_bake_cluster.py), K = 4,096: thousands of empty clusters, one of 2,500"""
    x = np.ascontiguousarray(CM.crafted_decode()[:, 14:59], f32)
    cnt = check(x, 4_096)
    assert ((cnt == 0).sum(axis=1) >= 1_500).all() and (cnt.max(axis=1) >= 2_500).all()


def test_argument_validation_without_a_device():
    lib = _lib.lib()
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    x = CM.random_points(4, 1)
    means, index = np.zeros((3, 45), f32), np.zeros(4, np.uint32)
    px, pm, pi = x.ctypes.data, means.ctypes.data, index.ctypes.data
    assert lib.gs_import_cluster_shs(None, None, 4, 3, pm, pi) == bad
    assert lib.gs_import_cluster_shs(None, px, 4, 3, None, pi) == bad
    assert lib.gs_import_cluster_shs(None, px, 4, 3, pm, None) == bad
    assert lib.gs_import_cluster_shs(None, px, 0, 3, pm, pi) == bad
    assert lib.gs_import_cluster_shs(None, px, 4, 0, pm, pi) == bad
    assert lib.gs_import_cluster_shs(None, px, 4, 65_537, pm, pi) == bad
    assert not means.any() and not index.any()                          # a refusal writes nothing
    assert lib.gs_import_cluster_shs(None, px, 4, 3, pm, pi) == 0
    assert same_bits(means, CM.lloyd(x, 3)[0], dtype=None)
    assert lib.gs_abi_version() == 9                                    # an addition to ABI 9
