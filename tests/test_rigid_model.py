"""The rigid rotate / scale of the selection on the CPU box: the host build of the shipped lines (csrc/gs_params.h's
edit_rigid_rotate_of and the per-splat functions of csrc/gs_device_math.h, through tests/rigid_host_harness.cpp) against the numpy twin
(tests/rigid_model.py) bit for bit; the twin against the shipped merge (BakeSplatTransform); the physics of the float64 form; the rewritten blobs drawn by
the CPU oracle against the original frame; and the interface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import edit_model as EM
import export_model as XM
import oracle_lib as O
import rigid_model as RM
import transform_model as TM
from common import _p, default_camera, rt_err, small_asset
from harness import build_harness
from unitygaussiansplatting_amd import _abi, _lib, camera
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=f32)


@pytest.fixture(scope="module")
def rh(tmp_path_factory):
    lib = C.CDLL(build_harness(tmp_path_factory.mktemp("rh"), "rigid_host_harness.cpp"))
    for name in ("rh_xform", "rh_rotate", "rh_bake", "rh_scale"):
        getattr(lib, name).restype = C.c_int
    return lib


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_floats(a, b) -> bool:
    """bit for bit, a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def unit(v):
    v = np.asarray(v, f64)
    return v / np.linalg.norm(v)


def axis_angle(axis, angle):
    a = unit(axis)
    return np.concatenate([a * np.sin(angle / 2.0), [np.cos(angle / 2.0)]])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def tool_frames(rng):
    """(o2w, w2o) pairs as float32 4x4: identity, rotations, similarities, non-uniformly scaled and mirrored frames (w2o = the float32 inverse)"""
    out = [(EYE, EYE)]
    for k in range(40):
        q = unit(rng.standard_normal(4))
        s = [(1.0, 1.0, 1.0), (2.5, 2.5, 2.5), tuple(rng.uniform(0.2, 4.0, 3)), tuple(rng.uniform(0.2, 4.0, 3) * rng.choice([-1.0, 1.0], 3)), (-1.0, 1.0, 1.0)][k % 5]
        tr = camera.Transform(position=tuple(rng.standard_normal(3)), rotation=tuple(q), scale=s)
        out.append((tr.localToWorldMatrix, tr.worldToLocalMatrix))
    return out


def branch_deltas(rng):
    """delta quaternions (with O2W = I, L = R(delta)) at the seams of the quaternion extraction: the trace 1 + 2 cos(angle) changes sign at 120 degrees;
    about (1, 1, 1) the diagonal entries are equal as well; half turns about the axes and about random axes take the three diagonal branches"""
    out = []
    third = 2.0 * np.pi / 3.0
    for eps in (0.0, 1e-8, -1e-8, 1e-7, -1e-7, 1e-4, -1e-4):
        out.append(axis_angle((1, 1, 1), third + eps))
        out.append(axis_angle((1, -1, 1), third + eps))
        for _ in range(4):
            out.append(axis_angle(rng.standard_normal(3), third + eps))
    for axis in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        for eps in (0.0, 1e-7, -1e-7):
            out.append(axis_angle(axis, np.pi + eps))
    for _ in range(30):
        out.append(axis_angle(rng.standard_normal(3), np.pi - abs(rng.normal()) * 1e-3))
    return [np.asarray(q, f32) for q in out]


def random_splats(rng, n):
    """rotation words of random unit quaternions and [n, 48] SH records; the last three floats of a record are a marker"""
    q = rng.standard_normal((n, 4))
    words = TM.encode_quat_norm10(TM.pack_smallest3((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)))
    sh = np.zeros((n, 48), f32)
    sh[:, :45] = (rng.standard_normal((n, 45)) * 0.3).astype(f32)
    sh[:, 45:] = np.array([7.0, 8.0, 9.0], f32)
    return words.astype(np.uint32), sh


def extreme_sh(rng, n):
    """denormal, huge (the sums overflow), zero and signed-zero coefficients"""
    sh = np.zeros((n, 48), f32)
    kinds = [1.0e-40, 3.0e-39, 1.0e-45, 3.0e38, 1.0e30, 0.0]
    for k in range(n):
        mag = np.array([kinds[j] for j in rng.integers(0, len(kinds), 45)], f64)
        sh[k, :45] = (mag * rng.choice([-1.0, 1.0], 45) * rng.uniform(0.5, 1.0, 45)).astype(f32)
    return sh


def harness_xform(rh, o2w, w2o, delta):
    o2w, w2o, delta = (np.ascontiguousarray(v, f32) for v in (o2w, w2o, delta))
    L, q, bands = np.zeros(9, f32), np.zeros(4, f32), np.zeros(83, f32)
    rc = rh.rh_xform(_p(o2w), _p(w2o), _p(delta), _p(L), _p(q), _p(bands))
    return rc, L.reshape(3, 3), q, bands


def harness_rotate(rh, fn, o2w, w2o, delta, words, sh):
    o2w, w2o, delta = (np.ascontiguousarray(v, f32) for v in (o2w, w2o, delta))
    words, sh = np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(sh, f32)
    n = len(words)
    if fn == "rh_rotate":
        outW, outSH = np.zeros(n, np.uint32), sh.copy()
        assert rh.rh_rotate(_p(o2w), _p(w2o), _p(delta), _p(words), _p(sh), C.c_uint32(n), _p(outW), _p(outSH)) == 0
        return outW, outSH
    outQ, outW, outSH = np.zeros((n, 4), f32), np.zeros(n, np.uint32), np.zeros((n, 45), f32)
    assert rh.rh_bake(_p(o2w), _p(w2o), _p(delta), _p(words), _p(sh), C.c_uint32(n), _p(outQ), _p(outW), _p(outSH)) == 0
    return outQ, outW, outSH


def cases(rng):
    frames = tool_frames(rng)
    out = []
    for k, (o2w, w2o) in enumerate(frames):
        d = rng.standard_normal(4) * [1.0, 1.0e-3, 37.0, 1.0][k % 4]          # non-unit deltas
        out.append((o2w, w2o, np.asarray(d, f32)))
    out += [(EYE, EYE, d) for d in branch_deltas(rng)]
    return out


# ---- 1. the host build of the shipped lines against the twin, bit for bit ------------------------------------------------------------------------
def test_harness_equals_the_twin(rh):
    rng = np.random.default_rng(415)
    words, sh = random_splats(rng, 64)
    wild = extreme_sh(rng, 32)
    branches = set()
    for k, (o2w, w2o, d) in enumerate(cases(rng)):
        G = RM.rigid_rotate_of(o2w, w2o, d)
        rc, L, q, bands = harness_xform(rh, o2w, w2o, d)
        assert rc == 0
        assert same_floats(L, G.L), (k, "L")
        assert same_floats(q, G.q), (k, "q_L", q, G.q)
        assert same_floats(bands, np.concatenate([b.reshape(-1) for b in G.bands])), (k, "bands")
        L4 = np.zeros((4, 4), f32); L4[:3, :3] = G.L
        branches.add(RM.quat_branch(XM.sh_rot_matrix(L4, f32)))
        gw, gsh = harness_rotate(rh, "rh_rotate", o2w, w2o, d, words, sh)
        assert np.array_equal(gw, RM.rotate_words(words, G.q)), (k, "words")
        assert same_floats(gsh, RM.rotate_sh_records(sh, G.bands)), (k, "sh")
        assert np.array_equal(bits(gsh[:, 45:]), bits(sh[:, 45:]))             # the last 12 bytes of a record are not written
        if k % 8 == 0:
            _, xsh = harness_rotate(rh, "rh_rotate", o2w, w2o, d, words[:32], wild)
            assert same_floats(xsh, RM.rotate_sh_records(wild, G.bands)), (k, "denormal / huge sh")
    assert branches == {0, 1, 2, 3}, branches                                  # premise: every branch of the extraction was taken
    # the uniform scale
    scales = np.concatenate([rng.uniform(1.0e-3, 2.0, (64, 3)), [[1.0e-40, 3.0e38, 0.0], [-0.0, np.inf, 1.0]]]).astype(f32)
    for s in (2.0, 0.5, -3.0, 0.0, 1.0e-30, 1.0 / 3.0):
        d3 = np.full(3, s, f32)
        out = np.zeros_like(scales)
        assert rh.rh_scale(_p(d3), _p(scales), C.c_uint32(len(scales)), _p(out)) == 1 and RM.is_uniform(d3)
        assert same_floats(out, RM.scale_scales(scales, d3[0])), s
    for d3 in ((2.0, 2.0, 2.5), (1.0, -1.0, 1.0), (np.nan, np.nan, np.nan)):   # not uniform: -x is not x, a NaN equals nothing
        d3 = np.asarray(d3, f32)
        assert rh.rh_scale(_p(d3), _p(scales), C.c_uint32(len(scales)), _p(np.zeros_like(scales))) == 0 and not RM.is_uniform(d3)


def test_refused_arguments(rh):
    bad_deltas = [(0, 0, 0, 0), (np.nan, 0, 0, 1), (np.inf, 0, 0, 1), (3.0e38, 3.0e38, 3.0e38, 3.0e38)]       # the last: finite components, a norm that is finite in fp64
    for k, d in enumerate(bad_deltas):
        refused = k < 3
        assert (harness_xform(rh, EYE, EYE, d)[0] == 1) == refused, d
        if refused:
            with pytest.raises(RM.Refused):
                RM.rigid_rotate_of(EYE, EYE, d)
        else:
            RM.rigid_rotate_of(EYE, EYE, d)
    for row in range(3):
        for v in (0.0, np.nan, np.inf):
            m = EYE.copy(); m[row, :3] = (v, 0.0, 0.0) if v != 0.0 else 0.0
            assert harness_xform(rh, m, EYE, (0, 0, 0, 1))[0] == 1
            with pytest.raises(RM.Refused):
                RM.rigid_rotate_of(m, EYE, (0, 0, 0, 1))


# ---- 2. against the shipped merge ------------------------------------------------------------------------------------------------------------------
def test_rigid_rotate_is_the_merge_of_the_same_transform(rh):
    """(rot, SH) of a rigidly rotated splat = BakeSplatTransform(m = L, rot = q_L, scale = 1) of it, and the word is the encoder's word: no new tolerance"""
    rng = np.random.default_rng(416)
    words, sh = random_splats(rng, 128)
    for k, (o2w, w2o, d) in enumerate(cases(rng)):
        gw, gsh = harness_rotate(rh, "rh_rotate", o2w, w2o, d, words, sh)
        bq, bw, bsh = harness_rotate(rh, "rh_bake", o2w, w2o, d, words, sh)
        assert np.array_equal(gw, bw), (k, "word")
        assert same_floats(gsh[:, :45], bsh), (k, "sh")
        # ... and the numpy merge (tests/copy_model.py's arithmetic) over the twin's L and q_L says the same
        G = RM.rigid_rotate_of(o2w, w2o, d)
        L4 = np.eye(4, dtype=f32); L4[:3, :3] = G.L
        assert same_floats(bq, XM.quat_mul(G.q, TM.decode_rotation(words))), (k, "quaternion")
        assert same_floats(bsh, XM.rotate_sh(sh[:, :45].reshape(-1, 15, 3), XM.sh_bands(L4, f32), f32).reshape(-1, 45)), (k, "sh model")


# ---- 3. physics, in float64 ------------------------------------------------------------------------------------------------------------------------
def test_physics_of_the_float64_form(rh):
    """O2W = s Q (a similarity), W2O its inverse, a unit delta: q_L = conj(q_Q) delta q_Q up to sign, L orthonormal, and the rotated coefficients
    shaded along L d equal the originals shaded along d -- 1e-9 relative: float64 rounding over <= 50 terms.  The distance of the float32 twin from the
    float64 form is recorded next to the same distance for BakeSplatTransform; by check 2 they are the same number."""
    rng = np.random.default_rng(417)
    worst_q = worst_sh = worst_q_bake = worst_sh_bake = 0.0
    for k in range(40):
        qQ, d = unit(rng.standard_normal(4)), unit(rng.standard_normal(4))
        s = float(rng.uniform(0.25, 4.0))
        Q = camera.quat_to_mat3(qQ)
        o2w, w2o = np.eye(4), np.eye(4)
        o2w[:3, :3], w2o[:3, :3] = s * Q, Q.T / s
        G = RM.rigid_rotate_of(o2w, w2o, d, f64)
        assert G.L.dtype == f64 and G.q.dtype == f64
        conj = qQ * [-1.0, -1.0, -1.0, 1.0]
        want = camera.quat_mul(camera.quat_mul(conj, d), qQ)
        assert min(np.abs(G.q - want).max(), np.abs(G.q + want).max()) <= 1e-9, (k, G.q, want)
        assert np.abs(G.L @ G.L.T - np.eye(3)).max() <= 1e-9 and abs(np.linalg.det(G.L) - 1.0) <= 1e-9
        sh = rng.standard_normal((32, 15, 3))
        out = XM.rotate_sh(sh, G.bands, f64)
        dirs = rng.standard_normal((32, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        got = np.einsum("nkc,nk->nc", out, RM.shade_basis(dirs @ G.L.T))          # along L d
        ref = np.einsum("nkc,nk->nc", sh, RM.shade_basis(dirs))
        mag = np.abs(sh).sum(axis=1) * 0.75
        assert (np.abs(got - ref) <= 1e-9 * mag).all(), (k, float(np.abs(got - ref).max()))
        # the float32 twin and the shipped merge on the same (rounded) inputs, against the float64 form
        o32, w32, d32 = o2w.astype(f32), w2o.astype(f32), d.astype(f32)
        G32 = RM.rigid_rotate_of(o32, w32, d32)
        words, rec = random_splats(rng, 32)
        tw = RM.rotate_sh_records(rec, G32.bands)[:, :45]
        bq, _, bsh = harness_rotate(rh, "rh_bake", o32, w32, d32, words, rec)
        exact = XM.rotate_sh(rec[:, :45].astype(f64).reshape(-1, 15, 3), G.bands, f64).reshape(-1, 45)
        rot = TM.decode_rotation(words)
        exact_q = np.stack([camera.quat_mul(G.q, r) for r in rot.astype(f64)])
        worst_sh = max(worst_sh, float(np.abs(tw - exact).max()))
        worst_sh_bake = max(worst_sh_bake, float(np.abs(bsh - exact).max()))
        worst_q = max(worst_q, float(np.abs(TM.quat_mul(G32.q, rot) - exact_q).max()))
        worst_q_bake = max(worst_q_bake, float(np.abs(bq - exact_q).max()))
    print(f"float32 against float64, 40 similarities x 32 splats: quaternion {worst_q:.3e} (merge {worst_q_bake:.3e}), sh {worst_sh:.3e} (merge {worst_sh_bake:.3e})")
    assert worst_q == worst_q_bake and worst_sh == worst_sh_bake


# ---- 4. end to end on the oracle --------------------------------------------------------------------------------------------------------------------
def oracle_frame(asset, cam, tr):
    orc = O.Oracle(asset)
    orc.sort(camera.sort_matrix(cam, tr.localToWorldMatrix))
    P = camera.frame_params(cam, tr)
    orc.calc_view(P)
    return orc.draw(P, 0)


def bounds_centre(asset):
    pos = TM.TransformModel(asset).pos_rows().astype(f64)
    return ((pos.min(axis=0) + pos.max(axis=0)) * 0.5).astype(f32)


def edited(asset, rigid, op):
    m = RM.RigidModel(asset, rigid)
    m.select_all()
    m.store_pos(); m.store_other(); m.store_sh()
    assert op(m)
    return m


@pytest.mark.parametrize("seed", [5, 9])
def test_a_rotated_object_looks_like_the_object_rotated(rh, seed):
    """Select all, rotate by a quarter turn about an oblique axis through the centre of the bounds (O2W = I), then draw the rewritten blobs under the
    object transform that undoes the rotation, T(c) R^-1 T(-c): a rigid rotation gives the original frame back, the reference's kernel (positions
    only, orientation multiplied on the wrong side, SH left alone) does not.  The assertion is the comparison of the two deviations."""
    a = small_asset(300, seed, "VeryHigh")
    cam = default_camera()
    before = oracle_frame(a, cam, camera.Transform())
    c = bounds_centre(a)
    d = axis_angle((1.0, 2.0, -0.5), np.pi / 2.0)
    R = camera.quat_to_mat3(d)
    undo = camera.Transform(position=tuple(c.astype(f64) - R.T @ c.astype(f64)), rotation=tuple(d * [-1.0, -1.0, -1.0, 1.0]))
    e = {}
    for rigid in (True, False):
        m = edited(a, rigid, lambda m: m.rotate(c, EYE, EYE, d.astype(f32)))
        if rigid:                                                  # the blobs that are drawn are the shipped lines' (the host build), not only the twin's
            m0 = RM.RigidModel(a)
            gw, gsh = harness_rotate(rh, "rh_rotate", EYE, EYE, d.astype(f32), m0.rot_words(), m0.sh_rows())
            assert np.array_equal(gw, m.rot_words()) and same_floats(gsh, m.sh_rows())
        e[rigid] = rt_err(oracle_frame(m.current_asset(), cam, undo), before)
    print(f"seed {seed}: rotated object against the original frame: rigid {e[True]:.5f}, reference mode {e[False]:.5f}")
    assert e[True] < e[False]


@pytest.mark.parametrize("seed", [5, 9])
def test_a_scaled_object_looks_like_the_object_from_twice_as_far(rh, seed):
    """Select all, scale uniformly by 2 about the centre of the bounds, and look at it from twice the distance (camera and target scaled about the same
    centre): a perspective image does not change under a similarity about a point when the eye follows it"""
    a = small_asset(300, seed, "VeryHigh")
    cam = default_camera()
    before = oracle_frame(a, cam, camera.Transform())
    c = bounds_centre(a)
    far = default_camera()
    far.position = tuple(c.astype(f64) + 2.0 * (np.asarray(cam.position, f64) - c))
    far.target = tuple(c.astype(f64) + 2.0 * (np.asarray(cam.target, f64) - c))
    e = {}
    for rigid in (True, False):
        m = edited(a, rigid, lambda m: m.scale(c, EYE, EYE, (2.0, 2.0, 2.0)))
        if rigid:                                                  # ... here too
            s0 = np.ascontiguousarray(RM.RigidModel(a).scale_rows(), f32)
            out = np.zeros_like(s0)
            assert rh.rh_scale(_p(np.full(3, 2.0, f32)), _p(s0), C.c_uint32(len(s0)), _p(out)) == 1 and same_floats(out, m.scale_rows())
        e[rigid] = rt_err(oracle_frame(m.current_asset(), far, camera.Transform()), before)
    print(f"seed {seed}: scaled object from twice as far against the original frame: rigid {e[True]:.5f}, reference mode {e[False]:.5f}")
    assert e[True] < e[False]


# ---- 5. the interface ---------------------------------------------------------------------------------------------------------------------------------
def test_setting_off_is_the_transform_model():
    a = small_asset(300, 5, "VeryHigh")
    tr = camera.Transform(position=(0.1, -0.2, 0.3), rotation=tuple(unit((0.2, -0.4, 0.1, 0.9))), scale=(1.5, 0.75, 2.0))
    q = np.asarray(unit((0.18, 0.36, 0.54, 0.73)), f32)
    m, t = RM.RigidModel(a), TM.TransformModel(a)
    for x in (m, t):
        x.upload_selected(EM.pack_bits(np.random.default_rng(3).random(300) < 0.5, x.nw))
        x.store_pos(); x.store_other()
    m.store_sh()
    for x in (m, t):
        assert x.rotate((0.3, -0.2, 0.1), tr.localToWorldMatrix, tr.worldToLocalMatrix, q)
    assert np.array_equal(m.pos_blob, t.pos_blob) and np.array_equal(m.other_blob, t.other_blob) and np.array_equal(m.sh_blob, np.asarray(a.shData, np.uint8))
    for x in (m, t):
        assert x.scale((0.3, -0.2, 0.1), tr.localToWorldMatrix, tr.worldToLocalMatrix, (2.0, 2.0, 2.0))
    assert np.array_equal(m.pos_blob, t.pos_blob) and np.array_equal(m.other_blob, t.other_blob)
    # ... and with it on, the positions are still the reference's; the rotation words, the SH and (uniform scale) the sizes are not
    r = RM.RigidModel(a, True)
    r.upload_selected(m.bits()[0]); r.store_pos(); r.store_other(); r.store_sh()
    assert r.rotate((0.3, -0.2, 0.1), tr.localToWorldMatrix, tr.worldToLocalMatrix, q)
    t2 = TM.TransformModel(a); t2.upload_selected(m.bits()[0]); t2.store_pos(); t2.store_other()
    t2.rotate((0.3, -0.2, 0.1), tr.localToWorldMatrix, tr.worldToLocalMatrix, q)
    sel = r.selected()
    assert np.array_equal(r.pos_blob, t2.pos_blob)
    assert (r.rot_words()[sel] != t2.rot_words()[sel]).any() and np.array_equal(r.rot_words()[~sel], t2.rot_words()[~sel])
    sh0 = np.asarray(a.shData, np.uint8)[:300 * 192].view(f32).reshape(300, 48)
    assert np.array_equal(bits(r.sh_rows()[~sel]), bits(sh0[~sel])) and np.array_equal(bits(r.sh_rows()[:, 45:]), bits(sh0[:, 45:]))
    assert (bits(r.sh_rows()[sel, :45]) != bits(sh0[sel, :45])).any()
    before = r.scale_rows().copy()
    assert r.scale((0.3, -0.2, 0.1), tr.localToWorldMatrix, tr.worldToLocalMatrix, (-2.0, -2.0, -2.0))
    assert np.array_equal(bits(r.scale_rows()[sel]), bits(before[sel] * f32(2.0))) and np.array_equal(bits(r.scale_rows()[~sel]), bits(before[~sel]))
    assert r.scale((0.3, -0.2, 0.1), tr.localToWorldMatrix, tr.worldToLocalMatrix, (3.0, 3.0, 2.0))       # not uniform: the sizes stay
    assert np.array_equal(bits(r.scale_rows()), bits(before * np.where(sel, f32(2.0), f32(1.0))[:, None]))


def test_error_paths_of_the_model():
    a = small_asset(300, 5, "VeryHigh")
    q = (0.0, 0.0, 0.0, 1.0)
    m = RM.RigidModel(a, True)
    m.select_all()
    m.store_pos(); m.store_other()
    assert not m.rotate((0, 0, 0), EYE, EYE, q)                                # all three copies
    m.store_sh()
    assert m.rotate((0, 0, 0), EYE, EYE, q)
    assert not m.rotate((0, 0, 0), EYE, EYE, (0, 0, 0, 0)) and not m.rotate((0, 0, 0), EYE, EYE, (np.nan, 0, 0, 1))
    bad = EYE.copy(); bad[1, :3] = 0.0
    assert not m.rotate((0, 0, 0), bad, EYE, q)
    m.set_rigid(False)
    assert m.rotate((0, 0, 0), bad, EYE, (0, 0, 0, 0))                         # errors of the rigid mode only
    m.set_rigid(True)
    m.release()
    m.select_all(); m.store_pos()
    assert not m.scale((0, 0, 0), EYE, EYE, (2.0, 2.0, 2.0))                   # the uniform handle needs the other copy
    assert m.scale((0, 0, 0), EYE, EYE, (2.0, 2.0, 1.0))                       # ... a non-uniform scale is the reference's and does not
    med = RM.RigidModel(small_asset(300, 5, "Medium"), True)                   # no gate passes: the copies are not made, the calls change nothing
    med.select_all(); med.store_pos(); med.store_other(); med.store_sh()
    assert med.sh_md is None and med.rotate((0, 0, 0), EYE, EYE, q) and med.scale((0, 0, 0), EYE, EYE, (2.0, 2.0, 2.0))
    assert np.array_equal(med.sh_blob, np.asarray(med.asset.shData, np.uint8)) and not med.sh_private


def test_the_entry_points_exist_everywhere():
    lib = _lib.lib()
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    assert lib.gs_abi_version() == 9
    assert lib.gs_renderer_edit_set_rigid_transforms(None, 1) == bad and lib.gs_renderer_edit_store_sh_mouse_down(None) == bad
    hdr = open(os.path.join(ROOT, "include", "gsplat_c.h")).read()
    cs = open(os.path.join(ROOT, "unitygaussiansplatting_amd", "dotnet", "GaussianSplatNative.cs")).read()
    for name in ("gs_renderer_edit_set_rigid_transforms", "gs_renderer_edit_store_sh_mouse_down"):
        assert re.search(r"int32_t\s+" + name + r"\s*\(", hdr) and name in _lib.SIGNATURES and re.search(r"extern\s+int\s+" + name + r"\s*\(", cs), name
    assert "unless" in re.search(r"SHs are not rotated and splat scales not scaled[^.]*\.", hdr).group(0)
    for name in ("EditSetRigidTransforms", "EditStoreSHMouseDown"):
        assert callable(getattr(GaussianSplatRenderer, name)), name
