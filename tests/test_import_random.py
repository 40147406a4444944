"""CPU suite: the native importer (csrc/gs_import.cpp: gs_import_encode) against the numpy importer (creator.py) on a seeded random walk -- splat counts around the
chunk (256) and texture-tile boundaries, every position / scale / colour / SH format, Morton and LinearizeData on and off, and inputs made adversarial on
purpose: coincident positions (empty chunk bounds), scales and opacity logits at the ends of the exp / sigmoid ranges, un-normalised and tied quaternion
components, SH coefficients far outside the clamp, denormals and signed zeros.  The bar is test_import.py's: all five blobs, the bounds and the data hash
identical byte for byte (GaussianSplatAssetCreator.cs:247-340, 576-1066; GaussianUtils.cs).  Eight seeds in the suite; GSPLAT_IMPORT_SEEDS=n adds n more
(3,000 were run once: all passed)."""
import os

import numpy as np
import pytest

from builders import _same, adversarial_splats
from unitygaussiansplatting_amd import asset as A
from unitygaussiansplatting_amd import creator, scenes

_SEEDS = list(range(1, 9)) + [100 + k for k in range(int(os.environ.get("GSPLAT_IMPORT_SEEDS", "0")))]
_VEC = [A.VectorFormat.Float32, A.VectorFormat.Norm16, A.VectorFormat.Norm11, A.VectorFormat.Norm6]
_COL = [A.ColorFormat.Float32x4, A.ColorFormat.Float16x4, A.ColorFormat.Norm8x4]          # (BC7 / Cluster*: test_import.py's preset cases -- minutes of k-means in numpy)
_SH = [A.SHFormat.Float32, A.SHFormat.Float16, A.SHFormat.Norm11, A.SHFormat.Norm6]


@pytest.mark.parametrize("seed", _SEEDS)
def test_native_importer_is_the_numpy_importer_on_a_random_case(seed):
    rng = np.random.default_rng(31_000 + seed)
    n = int(rng.choice([1, 2, 255, 256, 257, 511, 513, 2_047, 2_049, 4_099, 12_345]))
    raw = scenes.make_splats(n, int(rng.integers(1, 1000)), float(rng.choice([0.01, 1.0, 50.0])))
    if rng.random() < 0.7:
        raw = adversarial_splats(raw, rng, negative_zero=True)
    morton = bool(rng.random() < 0.6)
    linearize = bool(rng.random() < 0.8)
    if not linearize:
        raw = creator.LinearizeData(raw)
    fmt = dict(formatPos=_VEC[int(rng.integers(4))], formatScale=_VEC[int(rng.integers(4))], formatColor=_COL[int(rng.integers(3))], formatSH=_SH[int(rng.integers(4))])
    a = creator.CreateAssetFromSplats(raw, "Medium", morton=morton, linearize=linearize, **fmt)
    b = creator.CreateAssetFromSplatsNative(raw, "Medium", morton=morton, linearize=linearize, **fmt)
    _same(a, b)
