"""CPU: gsm::Neighbour* (csrc/gs_device_math.h) compiled for the host with tests/harness.py's line and run serially by tests/neighbour_host_harness.cpp the
way the kernels of gs_neighbours.hip run it -- keys, a stable sort, nine runs, the walk -- held to the numpy twin integer for integer on the families of
tests/neighbour_rig.py; and the same program under the host sanitizers."""
import subprocess

import numpy as np
import pytest

import neighbour_model as NM
import neighbour_rig as NR
from harness import build_harness, run_under_sanitizers

f32 = np.float32


@pytest.fixture(scope="module")
def nb_harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("neighbours"), "neighbour_host_harness.cpp", exe=True)


def host_counts(exe, tmp_path, pos, alive, radius, limit) -> np.ndarray:
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    with open(src, "wb") as f:
        f.write(np.uint32(len(pos)).tobytes() + f32(radius).tobytes() + np.uint32(limit).tobytes() + pos.tobytes() + np.asarray(alive, np.uint8).tobytes())
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return np.fromfile(dst, np.uint32)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_host_counts_equal_the_twin(nb_harness, tmp_path, seed):
    rng = np.random.default_rng(seed)
    cases = NR.adversarial(1500, seed) + [("identical",) + NR.identical(300)]
    for name, pos, radius in cases:
        for alive in (np.ones(len(pos), bool), rng.random(len(pos)) < 0.6):
            counts = NM.brute_counts(pos, alive, radius)
            for limit in (65535, 4, 1):
                got = host_counts(nb_harness, tmp_path, pos, alive, radius, limit)
                assert np.array_equal(got, NM.counts_words(counts, alive, limit)), (name, seed, limit)


@pytest.mark.parametrize("n", [1, 2, 33, 257])
def test_host_counts_at_small_sizes_and_extreme_radii(nb_harness, tmp_path, n):
    pos, radius = NR.gaussian(n, n)
    alive = np.ones(n, bool)
    for r in (NR.isolating_radius(pos), radius, NR.one_cell_radius(pos), 1.0e-15, 1.0e15):
        want = NM.counts_words(NM.brute_counts(pos, alive, r), alive, 65535)
        assert np.array_equal(host_counts(nb_harness, tmp_path, pos, alive, r, 65535), want), (n, r)
    assert np.array_equal(host_counts(nb_harness, tmp_path, pos, alive, NR.one_cell_radius(pos), 65535), np.full(n, n - 1, np.uint32))
    nobody = np.zeros(n, bool)
    assert np.array_equal(host_counts(nb_harness, tmp_path, pos, nobody, radius, 65535), np.full(n, NM.NOT_ALIVE, np.uint32))


def test_host_harness_under_the_sanitizers(tmp_path):
    """the stand-alone program over its own input (a lattice at the radius, a far pair in a clamped cell, a NaN, a dead splat), built with ASan and UBSan"""
    out = run_under_sanitizers(tmp_path, "neighbour_host_harness.cpp", "NEIGHBOUR_HARNESS_SANITIZED")
    assert out.returncode == 0 and "neighbour_host_harness ok" in out.stdout, out.stderr[-2000:]
