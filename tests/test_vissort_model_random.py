"""CPU suite: the specification GS_SORT_VISIBLE is built to -- "the visible splats sorted by the chain (key under the most recent matrix, ..., key under the
oldest, rank in the base order)" with consolidations "one stable sort of the base by the most recent matrix + the chain fix-up" -- against the ORACLE's
sequential stable sort of all N through the previous order on every SortPoints (GaussianSplatRenderer.cs:612-639, SplatUtilities.compute:69-82,
GpuSorting.cs:142-198), on seeded random sequences: tie-heavy and plain scenes, 6 to 40 sorts drawn from a small pool of cameras (so matrices recur in
any order: a recurring row moves to the front of the history), yaw-only / pitched / dolly cameras mixed, consolidations at random times, uploaded
(random permutation) and reset base orders in between, arbitrary visibility sets.  Twelve seeds in the suite; GSPLAT_VISMODEL_SEEDS=n adds n more
(1,500 were run once: all passed)."""
import os

import numpy as np
import pytest

import oracle_lib as O
from builders import tie_heavy_asset
from unitygaussiansplatting_amd import camera, scenes
from vissort_model import VisibleSortModel

_SEEDS = list(range(1, 13)) + [100 + k for k in range(int(os.environ.get("GSPLAT_VISMODEL_SEEDS", "0")))]


@pytest.mark.parametrize("seed", _SEEDS)
def test_chain_sort_and_consolidation_on_a_random_sequence(seed):
    rng = np.random.default_rng(71_000 + seed)
    kind = str(rng.choice(["lattice", "planes", "duplicates", "colocated", "random"]))
    a = tie_heavy_asset(kind, n=int(rng.choice([1500, 3000])), seed=int(rng.integers(1, 50)), quality=str(rng.choice(["VeryHigh", "Medium"])))
    n = a.splatCount
    orc = O.Oracle(a)
    model = VisibleSortModel(a, depth=10 ** 9)
    l2w = np.eye(4, dtype=np.float32)
    mk = lambda eye, target=(0.0, 0.0, 0.0): camera.Camera(position=eye, target=target, pixelWidth=320, pixelHeight=200)
    pool = [mk(scenes.orbit_eye(6.0, 0.0, float(rng.uniform(0, 360)))) for _ in range(3)]                   # yaw only: lattice columns tie
    pool += [mk(scenes.orbit_eye(6.0, float(rng.uniform(-40, 40)), float(rng.uniform(0, 360)))) for _ in range(3)]
    pool += [mk((0.0, 0.0, 6.0 + 0.5 * k), (0.0, 0.0, -100.0)) for k in range(3)]                            # a dolly: one direction row, another offset
    for k in range(int(rng.integers(6, 41))):
        u = rng.random()
        if u < 0.06:
            perm = rng.permutation(n).astype(np.uint32)        # gs_renderer_upload_order: the uploaded order is the new base
            orc.order[:] = perm
            model.reset(); model.base = perm.copy()
            model.rank = np.empty_like(perm); model.rank[perm] = np.arange(n, dtype=np.uint32)
        elif u < 0.10:
            orc.reset_order(); model.reset()                   # CSSetIndices
        cam = pool[int(rng.integers(len(pool)))]
        m = camera.sort_matrix(cam, l2w)
        orc.sort(m)
        model.push(m)
        if rng.random() < 0.2:
            model.consolidate()
            assert np.array_equal(model.base, orc.order), f"seed {seed} ({kind}): consolidation at sort {k}"
        for visible in (rng.random(n) < float(rng.uniform(0.05, 0.9)), np.ones(n, bool)):
            assert np.array_equal(model.visible_order(visible), orc.order[visible[orc.order]]), f"seed {seed} ({kind}): after sort {k}"
