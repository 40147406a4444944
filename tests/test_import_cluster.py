"""gs_import_assign_clusters(NULL, ...) -- the host loop the Cluster* SH palette is assigned with (csrc/gs_import.cpp
assign_clusters), exposed so that the GPU kernel of csrc/gs_cluster.hip can be held to it index for index -- against a strict
numpy restatement of its contract (cluster_cases.reference_assign), and gs_import_encode_on(NULL, ...) against gs_import_encode.
No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as CC
from unitygaussiansplatting_amd import _abi, _lib, creator, scenes

SPECIAL = CC.special_cases()


def _check(x, m):
    got = creator.AssignClusters(x, m)
    want = CC.reference_assign(x, m)
    bad = np.flatnonzero(got != want)
    assert got.dtype == np.uint32 and len(bad) == 0, f"{len(bad)} of {len(x)} indices differ, first at {bad[:5]}: {got[bad[:5]]} != {want[bad[:5]]}"
    return got


@pytest.mark.parametrize("k", [63, 4_097])
def test_host_assignment_matches_the_restated_contract_random(k):
    x, m = CC.random_case(257, k, 100 + k)
    got = _check(x, m)
    assert len(np.unique(got)) > 40                                     # a real competition, not one winner
    got = _check(CC.points_near_means(m, 257, 7), m)
    assert len(np.unique(got)) > 60 and got.max() > k - k // 8


@pytest.mark.parametrize("name", sorted(SPECIAL))
def test_host_assignment_special_values(name):
    x, m = SPECIAL[name]
    got = _check(x, m)
    if name == "duplicated_means":
        assert not np.isin(got, [5, 17, 40, 62]).any() and np.isin([0, 2, 39], got).all()      # the copies never win, their originals do
    if name == "nan_in_row0":
        assert not got.any()
    if name == "all_inf_points":
        assert not got[::3].any() and got.any()
    if name == "nan_in_x":
        assert not got[::7].any() and got[5] == 0 and got.any()
    if name == "nan_in_means":
        assert not np.isin(got, [1, 7, 33, 62]).any()
    if name == "nan_everywhere_but_row0":
        assert not got.any()
    if name in ("denormal_means", "denormal_both"):                      # (denormal points against ordinary means: |c|^2 alone decides)
        assert len(np.unique(got)) > 20                                  # nothing was flushed to zero (all-zero distances would all give 0)


def test_assignment_argument_validation():
    lib = _lib.lib()
    x, m = CC.random_case(4, 3, 1)
    out = np.zeros(4, np.uint32)
    px, pm, po = x.ctypes.data, m.ctypes.data, out.ctypes.data
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    assert lib.gs_import_assign_clusters(None, None, 4, pm, 3, po) == bad
    assert lib.gs_import_assign_clusters(None, px, 4, None, 3, po) == bad
    assert lib.gs_import_assign_clusters(None, px, 4, pm, 3, None) == bad
    assert lib.gs_import_assign_clusters(None, px, 0, pm, 3, po) == bad
    assert lib.gs_import_assign_clusters(None, px, 4, pm, 0, po) == bad
    assert lib.gs_import_assign_clusters(None, px, 4, pm, 3, po) == 0
    assert np.array_equal(out, CC.reference_assign(x, m))
    assert lib.gs_import_assign_clusters(None, px, 1, pm, 1, po) == 0 and out[0] == 0            # one point, one mean
    sizes = (C.c_uint64 * 5)()
    ok = _abi.gs_import_formats(2, 2, 2, 3, 1, 1)
    assert lib.gs_import_encode_on(None, None, C.byref(ok), (C.c_void_p * 5)(), sizes, None, None) == bad


def _encode(fn, raw, fmt, *ctx):
    n = len(raw)
    arrs = [np.ascontiguousarray(a, np.float32) for a in (raw.pos, raw.dc0, raw.sh.reshape(n, 45), raw.opacity, raw.scale, raw.rot)]
    inp = _abi.gs_import_input(n, *[a.ctypes.data for a in arrs])
    sizes = (C.c_uint64 * 5)()
    assert _lib.lib().gs_import_blob_sizes(n, C.byref(fmt), sizes) == 0
    blobs = [np.full(int(s), 0xA5, np.uint8) for s in sizes]
    ptrs = (C.c_void_p * 5)(*[b.ctypes.data if len(b) else None for b in blobs])
    bmin, bmax = (C.c_float * 3)(), (C.c_float * 3)()
    assert fn(*ctx, C.byref(inp), C.byref(fmt), ptrs, sizes, bmin, bmax) == 0
    return blobs, tuple(bmin), tuple(bmax)


def test_encode_on_without_a_context_is_encode():
    """VeryLow (Cluster4k palette, BC7 colour) at n = 4,500: the same five blobs and bounds from the two entry points."""
    from unitygaussiansplatting_amd.creator import QUALITY
    raw = scenes.make_splats(4_500, 4_700, 3.0)
    fp, fs, fc, fsh = QUALITY["VeryLow"]
    fmt = _abi.gs_import_formats(int(fp), int(fs), int(fc), int(fsh), 1, 1)
    lib = _lib.lib()
    a, amin, amax = _encode(lib.gs_import_encode, raw, fmt)
    b, bmin, bmax = _encode(lib.gs_import_encode_on, raw, fmt, None)
    assert int(fsh) == 8                                                # GS_SH_CLUSTER4K
    for k in range(5):
        assert np.array_equal(a[k], b[k]), f"blob {k} differs"
    assert amin == bmin and amax == bmax
    idx = np.frombuffer(a[1][:4_500 * 8].tobytes(), "<u2").reshape(4_500, 4)[:, 3]
    assert len(np.unique(idx)) > 512                                    # the palette is in use
