"""-m gpu: a seeded random walk over what the fixed-case parity tests pin one at a time -- asset preset and size, scene extent, camera (outside, inside
the cloud, grazing, narrow / wide field of view), target size (odd, tiny, tall, wide), object transform (rotated, non-uniformly scaled, mirrored),
_SplatScale / _SplatOpacityScale / _SHOrder / _SHOnly, sort mode, tile shape, cutouts, deleted bits, blend mode -- each case through the C-ABI and through the oracle:

    order buffer              bit-exact (CSCalcDistances + the stable sort, SplatUtilities.compute:69-82, GpuSorting.cs:142-198)
    40-byte SplatViewData     bit-exact (CSCalcViewData, SplatUtilities.compute:189-252)
    (tile, splat) pairs, visible count   equal
    RGBA16F target            <= 2^-9 relative to max(1, |c|), every pixel; the fast blend mode <= 4e-3

Three seeds run in the suite; GSPLAT_PARITY_SEEDS=n (from GSPLAT_PARITY_SEED0, default 100) adds a campaign of n more (scripts/r06_call27.sh ran 150 once,
scripts/r06_call31.sh 230 others, scripts/r06_call33.sh 85 more)."""
import os

import numpy as np
import pytest

import oracle_lib as O
from common import RT_TOL, rt_err, views_equal
from builders import CUTOUT_SETS, _case
from unitygaussiansplatting_amd import camera, creator, scenes
from unitygaussiansplatting_amd._lib import GsError
from unitygaussiansplatting_amd.cutout import shader_data_array
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, RenderTarget

pytestmark = pytest.mark.gpu

_SEEDS = [1, 2, 3] + [int(os.environ.get("GSPLAT_PARITY_SEED0", "100")) + k for k in range(int(os.environ.get("GSPLAT_PARITY_SEEDS", "0")))]
@pytest.mark.parametrize("seed", _SEEDS)
def test_random_case_against_the_oracle(gpu_ctx, seed):
    c = _case(seed)
    what = {k: c[k] for k in ("n", "quality", "extent", "kind", "fields", "mode", "tile", "cut", "bits_seed", "blend")} | {"size": (c["cam"].pixelWidth, c["cam"].pixelHeight), "transform": c["tr"]}
    raw = scenes.make_splats(c["n"], c["asset_seed"], c["extent"])
    a = creator.CreateAssetFromSplatsNative(raw, c["quality"], name=f"rnd{seed}")
    r = GaussianSplatRenderer(gpu_ctx, a, c["tr"])
    for k, v in c["fields"].items():
        setattr(r, k, v)
    r.sortMode = c["mode"]
    r.OnEnable()
    r.SetTileShape(*c["tile"])
    r.blendMode = c["blend"]
    r.m_Cutouts = CUTOUT_SETS[c["cut"]] if c["cut"] else None
    bits = None
    if c["bits_seed"] is not None:
        g = np.random.default_rng(c["bits_seed"])
        bits = (g.integers(0, 2 ** 32, (a.splatCount + 31) // 32, dtype=np.uint64) & g.integers(0, 2 ** 32, (a.splatCount + 31) // 32, dtype=np.uint64)).astype(np.uint32)
    r.SetDeletedBits(bits)
    cam = c["cam"]
    rt = RenderTarget(gpu_ctx, cam.pixelWidth, cam.pixelHeight)
    orc = O.Oracle(a)
    cams = [cam, camera.Camera(position=tuple(np.asarray(cam.position) * 1.03), pixelWidth=cam.pixelWidth, pixelHeight=cam.pixelHeight, fieldOfView=cam.fieldOfView)]
    for k, cm in enumerate(cams):                               # two frames: the second sort goes through the first one's order
        r.SortPoints(cm)
        orc.sort(camera.sort_matrix(cm, r.transform.localToWorldMatrix))
        r.CalcViewData(cm); rt.Clear(); r.Draw(cm, rt)
        try:
            st = r.FrameStats()
        except GsError as ex:                                   # the documented protocol (gsplat_c.h: GS_ERR_PAIR_OVERFLOW): the frame outgrew the pair buffer,
            assert ex.code == -6, ex                            # the library has grown it, the host draws the frame again (seed 1086: 60 k splats of a 0.5-unit scene at
            rt.Clear(); r.Draw(cm, rt)                          # _SplatScale 2 from a grazing camera, 1280x720 in 16x16 tiles: more than the initial 4 M pairs)
            st = r.FrameStats()
        P = r.FrameParams(cm)
        arr, ncut = shader_data_array(r.m_Cutouts, r.transform.localToWorldMatrix)
        want_view = orc.calc_view(P, arr, ncut, bits)
        assert views_equal(r.DownloadView(), want_view), f"seed {seed} frame {k}: view records differ; {what}"
        pairs = orc.pairs(P, st)                                # (for the tile shape the draw reports; also sets orc.visible)
        assert st.visible_splats == orc.visible, f"seed {seed} frame {k}: visible {st.visible_splats} vs {orc.visible}; {what}"
        assert st.tile_pairs == pairs, f"seed {seed} frame {k}: pairs {st.tile_pairs} vs {pairs}; {what}"
        ref = orc.draw(P, c["blend"])
        e = rt_err(rt.Download(), ref)
        assert e <= (RT_TOL if c["blend"] == 0 else 4e-3), f"seed {seed} frame {k}: target off by {e}; {what}"
        assert np.array_equal(r.DownloadOrder(), orc.order), f"seed {seed} frame {k}: order differs; {what}"
    r.OnDisable()
    rt.Dispose()
