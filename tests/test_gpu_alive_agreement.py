"""-m gpu: every consumer of the alive set -- the compacted export, the bake, the SPZ export, the attribute statistics, the neighbour counts, the
components -- sees ONE set, the one the host models give: alive = index < N, not deleted, not cut (export_model.ExportModel.alive), listed = alive and
every component of the position finite (neighbour_model.listed_flags).  The consumers share their compaction kernels (csrc/gs_compact.hip), and those
that do not (the attribute kernels) restate the test: this module is what ties them together.

An all-fp32 (VeryHigh) asset, so that non-finite positions exist.  N = 257 and 513: two and three chunks, a last selection word with tail bits, and
a fifth wave -- at 257 it holds splat 256 alone, which is deleted, so the wave lists nothing; at 513 it holds alive splats.  Deleted: 0, 255, 256 (a
chunk's first and last splat, the next chunk's first) and a few more; one inverted ellipsoid cuts the five splats placed inside it; among the alive,
splat 64 has a NaN component and splat N - 3 a +inf one.  Every case also runs without the cutout, where the attribute kernels of three classes skip
the position load."""
import functools

import numpy as np
import pytest

import edit_model as EM
import export_model as XM
import neighbour_model as NM
from builders import fp32_point_asset
from common import same_bits
from gpu_rig import pinned_renderer
from unitygaussiansplatting_amd import camera
from unitygaussiansplatting_amd.cutout import GaussianCutout, Type
from unitygaussiansplatting_amd.renderer import SplatAttribute

pytestmark = pytest.mark.gpu
f32 = np.float32
NOT_ALIVE = 0xFFFFFFFF
RADIUS = 1000.0                                                    # every listed splat is every other one's neighbour
NAN_AT, CUT_AT = 64, (10, 70, 130, 200, 250)                       # (a wave's first lane; one splat of each wave of the first chunk)
CENTRE = (5.0, 5.0, 5.0)


def cutouts():
    """inverted: what lies INSIDE is cut.  A NaN is inside nothing, +inf is outside"""
    return [GaussianCutout(Type.Ellipsoid, True, camera.Transform(position=CENTRE, scale=(0.5, 0.5, 0.5)))]


@functools.lru_cache(maxsize=None)
def scene(n: int):
    """(asset, positions, deleted words): distinct positions without a zero component, so that bits identify a splat and no bound is a signed zero"""
    rng = np.random.default_rng(n)
    pos = (rng.uniform(0.25, 2.0, (n, 3)) * rng.choice((-1.0, 1.0), (n, 3))).astype(f32)
    pos[list(CUT_AT)] = (np.asarray(CENTRE) + rng.uniform(0.01, 0.1, (len(CUT_AT), 3))).astype(f32)
    pos[NAN_AT, 0] = np.nan
    pos[n - 3, 2] = np.inf
    deleted = np.zeros(n, bool)
    deleted[[0, 255, 256, 31, 32, 100]] = True
    pos.setflags(write=False)
    return fp32_point_asset(pos), pos, EM.pack_bits(deleted, (n + 31) // 32)


@functools.lru_cache(maxsize=None)
def expected(n: int, cut: bool):
    """(alive, listed) flags of the host models, computed once per case and left unchanged"""
    asset, pos, words = scene(n)
    m = XM.ExportModel(asset)
    m.edit.set_deleted_bits(words)
    m.edit.set_cutouts(cutouts() if cut else None, camera.Transform().localToWorldMatrix)
    alive = m.alive()
    listed = NM.listed_flags(pos, alive)
    # the scene is what the docstring says it is
    assert not alive[[0, 255, 256]].any() and alive[NAN_AT] and alive[n - 3]
    assert np.array_equal(np.flatnonzero(m.edit.cut), CUT_AT if cut else ())
    assert np.array_equal(np.flatnonzero(alive & ~listed), (NAN_AT, n - 3))
    alive.setflags(write=False)
    listed.setflags(write=False)
    return alive, listed


@pytest.mark.parametrize("cut", [True, False], ids=["one cutout", "no cutout"])
@pytest.mark.parametrize("n", [257, 513])
def test_every_consumer_sees_the_models_alive_set(gpu_ctx, n, cut):
    asset, pos, words = scene(n)
    alive, listed = expected(n, cut)
    count, m = int(alive.sum()), int(listed.sum())
    r = pinned_renderer(gpu_ctx, asset)
    try:
        r.SetDeletedBits(words)
        r.m_Cutouts = cutouts() if cut else None
        r.UpdateCutoutsBuffer()
        # the compacted export: the alive records in index order (a position's bits name its splat)
        rows = r.ExportAlive()
        assert len(rows) == count and same_bits(rows[:, 0:3], pos[alive])
        # the bake: the count, and the bounds fminf / fmaxf leave of the alive positions (a NaN is skipped, +inf is the maximum)
        baked = r.EditBakeAsset("VeryHigh")
        try:
            assert baked.splatCount == count
            assert same_bits(baked.boundsMin, np.fmin.reduce(pos[alive], axis=0)) and same_bits(baked.boundsMax, np.fmax.reduce(pos[alive], axis=0))
            assert baked.boundsMax[2] == np.inf
        finally:
            baked.Dispose()
        # the SPZ export
        assert r.ExportSpzBody()[1] == count
        # the attribute kernels, one attribute of each class: opacity, scale, position, colour
        for attr in (SplatAttribute.Opacity, SplatAttribute.ScaleMax, SplatAttribute.PosX, SplatAttribute.Luma):
            assert r.EditAttributeStats(attr).members == count, attr
        # the neighbour grid: a count for exactly the alive splats; the listed ones see each other, the two non-finite ones nobody
        counts = r.EditNeighbourCounts(RADIUS)
        assert np.array_equal(np.flatnonzero(counts != NOT_ALIVE), np.flatnonzero(alive))
        assert (counts[listed] == m - 1).all() and not counts[alive & ~listed].any()
        # the components: a label for exactly the alive splats; the listed ones are one component, the two non-finite ones components of their own
        labels, sizes = r.EditComponents(RADIUS)
        assert np.array_equal(np.flatnonzero(labels != NOT_ALIVE), np.flatnonzero(alive)) and not sizes[~alive].any()
        assert (labels[listed] == np.flatnonzero(listed)[0]).all() and (sizes[listed] == m).all()
        lonely = np.flatnonzero(alive & ~listed)
        assert np.array_equal(labels[lonely], lonely) and (sizes[lonely] == 1).all()
    finally:
        r.DisposeResourcesForAsset()
