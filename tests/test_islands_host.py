"""CPU: gsm::NeighbourForEach (csrc/gs_device_math.h) compiled for the host with tests/harness.py's line and run serially by tests/islands_host_harness.cpp
the way the kernels of gs_neighbours.hip run it -- keys, a stable sort, nine runs, the edges to earlier sorted positions into a union-find, the minimum
and the size per root -- held to the numpy twin of tests/islands_model.py integer for integer on the families of tests/neighbour_rig.py and the new ones;
and the same program under the host sanitizers."""
import subprocess

import numpy as np
import pytest

import islands_model as IM
import neighbour_rig as NR
from harness import build_harness, run_under_sanitizers

f32 = np.float32


@pytest.fixture(scope="module")
def cc_harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("islands"), "islands_host_harness.cpp", exe=True)


def host_components(exe, tmp_path, pos, alive, radius):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    with open(src, "wb") as f:
        f.write(np.uint32(len(pos)).tobytes() + f32(radius).tobytes() + pos.tobytes() + np.asarray(alive, np.uint8).tobytes())
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    words = np.fromfile(dst, np.uint32)
    return words[:len(pos)], words[len(pos):]


def check(exe, tmp_path, pos, alive, radius, what):
    labels, sizes = host_components(exe, tmp_path, pos, alive, radius)
    want = IM.components(pos, alive, radius)
    assert np.array_equal(labels, want[0]) and np.array_equal(sizes, want[1]), (what, radius, np.flatnonzero(labels != want[0])[:8])
    return labels, sizes


@pytest.mark.parametrize("seed", (1, 2))
def test_host_components_equal_the_twin(cc_harness, tmp_path, seed):
    rng = np.random.default_rng(seed)
    for name, pos, radius in NR.adversarial(1500, seed) + IM.new_families(seed, 1500) + [("identical",) + NR.identical(300)]:
        for alive in (np.ones(len(pos), bool), rng.random(len(pos)) < 0.6):
            check(cc_harness, tmp_path, pos, alive, radius, (name, seed))


@pytest.mark.parametrize("n", [1, 2, 33, 257])
def test_host_components_at_small_sizes_and_extreme_radii(cc_harness, tmp_path, n):
    pos, radius = NR.gaussian(n, n)
    alive = np.ones(n, bool)
    for r in (NR.isolating_radius(pos), radius, NR.one_cell_radius(pos), 1.0e-15, 1.0e15):
        check(cc_harness, tmp_path, pos, alive, r, n)
    labels, sizes = check(cc_harness, tmp_path, pos, alive, NR.one_cell_radius(pos), n)
    assert not labels.any() and (sizes == n).all()
    labels, sizes = host_components(cc_harness, tmp_path, pos, np.zeros(n, bool), radius)
    assert (labels == IM.NOT_ALIVE).all() and not sizes.any()


def test_host_components_of_the_long_chains_and_the_ring(cc_harness, tmp_path):
    n = 4097
    alive = np.ones(n, bool)
    for axis in range(3):
        pos, radius, _ = IM.chain(n, 4 + axis, axis)
        labels, sizes = check(cc_harness, tmp_path, pos, alive, radius, ("chain", axis))
        assert not labels.any() and (sizes == n).all()
    pos, radius, where, want = IM.broken_chain(n, 5, (0, 255, 256, 1000, 2047, 4000, 4094))
    labels, sizes = check(cc_harness, tmp_path, pos, alive, radius, "broken chain")
    assert sorted(np.unique(sizes).tolist()) == sorted(set(want.tolist())) and len(np.unique(labels)) == len(want)
    pos, radius, _ = IM.ring(n, 7)
    labels, sizes = check(cc_harness, tmp_path, pos, alive, radius, "ring")
    assert not labels.any() and (sizes == n).all()


def test_the_label_is_the_minimum_and_not_the_root(tmp_path):
    """the harness built with the mutation ISLANDS_LABEL_IS_ROOT gives other labels on a shuffled chain (and the same sizes)"""
    exe = build_harness(tmp_path, "islands_host_harness.cpp", defines=["ISLANDS_LABEL_IS_ROOT"], exe=True)
    pos, radius, where = IM.chain(257, 6)
    alive = np.ones(257, bool)
    labels, sizes = host_components(exe, tmp_path, pos, alive, radius)
    want = IM.components(pos, alive, radius)
    first = (where[0], where[1])                                   # the line's first two points share the grid's first cell: either can be sorted position 0
    assert 0 not in first and not want[0].any()
    assert np.array_equal(sizes, want[1]) and (labels == labels[0]).all() and labels[0] in first


def test_host_harness_under_the_sanitizers(tmp_path):
    """the stand-alone program over its own input (a lattice at the radius with a corner cut off, a far pair in a clamped cell, a NaN, dead splats),
    built with ASan and UBSan"""
    out = run_under_sanitizers(tmp_path, "islands_host_harness.cpp", "ISLANDS_HARNESS_SANITIZED")
    assert out.returncode == 0 and "islands_host_harness ok" in out.stdout, out.stderr[-2000:]
