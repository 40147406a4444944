"""Moving, rotating and scaling the selection on the CPU box: the C-ABI surface of the six new gs_renderer_edit_* calls, known answers of the numpy
model the GPU tests are held to (tests/transform_model.py), its rotation codec against the reference's own compiled text (oracle/_ref), the clamp, and
the host build of the kernels' per-splat arithmetic (csrc/gs_device_math.h through tests/transform_host_harness.cpp) against the model, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import edit_model as EM
import ref_lib
import transform_model as TM
from builders import pos_only_asset
from common import _p
from harness import build_harness
from unitygaussiansplatting_amd import _abi, _lib, camera
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

f32 = np.float32
EYE = np.eye(4, dtype=f32)
IDENT_Q = (0.0, 0.0, 0.0, 1.0)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_floats(a, b) -> bool:
    """bit for bit, a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_transform_entry_points_validate_a_null_renderer():
    lib = _lib.lib()
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    v3, v4, m = (C.c_float * 3)(0, 0, 0), (C.c_float * 4)(0, 0, 0, 1), (C.c_float * 16)(*EYE.reshape(-1))
    buf = (C.c_uint8 * 16)()
    assert lib.gs_renderer_edit_store_pos_mouse_down(None) == bad
    assert lib.gs_renderer_edit_store_other_mouse_down(None) == bad
    assert lib.gs_renderer_edit_translate_selection(None, v3) == bad
    assert lib.gs_renderer_edit_rotate_selection(None, v3, m, m, v4) == bad
    assert lib.gs_renderer_edit_scale_selection(None, v3, m, m, v3) == bad
    assert lib.gs_renderer_edit_download_pos_other(None, buf, 16, buf, 16) == bad
    assert lib.gs_last_error_string() not in (None, b"")
    assert lib.gs_abi_version() == 9                             # additions to ABI 9


def test_renderer_mirrors_the_transform_methods():
    for name in ("EditStorePosMouseDown", "EditStoreOtherMouseDown", "EditTranslateSelection", "EditRotateSelection", "EditScaleSelection", "DownloadPosOther"):
        assert callable(getattr(GaussianSplatRenderer, name)), name


# ---- 2. known answers of the model ------------------------------------------------------------------------------------------------------
def grid_asset(n, seed=11):
    """point_asset with positions on the grid of multiples of 2^-8 in [-2, 2): differences and sums of such numbers (and of a centre on the same grid) are
    exact in float32, so subtracting and adding the centre gives the position back"""
    import crafted
    rng = np.random.default_rng(seed)
    pos = (rng.integers(-512, 512, (n, 3)).astype(f32) / f32(256.0)).astype(f32)
    q = rng.standard_normal((n, 4))
    return crafted.asset(pos, np.full((n, 3), 0.02, f32), rot=q)


def half_selected(m, seed=4):
    flags = np.random.default_rng(seed).random(m.n) < 0.5
    assert 0 < flags.sum() < m.n
    m.upload_selected(EM.pack_bits(flags, m.nw))
    return flags


def test_translate_moves_exactly_the_selected_rows():
    m = TM.TransformModel(EM.point_asset(300))
    before, other_before = m.pos_rows().copy(), m.other_blob.copy()
    flags = half_selected(m)
    d = np.array([0.25, -1.5, 3.0e-3], f32)
    assert m.translate(d)
    after = m.pos_rows()
    assert np.array_equal(bits(after[~flags]), bits(before[~flags]))
    assert np.array_equal(bits(after[flags]), bits(before[flags] + d[None, :]))
    assert (after[flags] != before[flags]).all()
    assert np.array_equal(m.other_blob, other_before)
    assert np.array_equal(m.pos, after) and np.array_equal(m.lo, EM.splat_bounds(after)[0])      # the edit model's bounds follow the move
    info = m.info()
    assert info[0] == flags.sum() and info[3:6].view(f32).tolist() == after[flags].min(axis=0).tolist()


def test_tail_bits_select_nothing():
    m = TM.TransformModel(EM.point_asset(33))
    m.select_all()
    assert m.bits()[0].tolist() == [0xFFFFFFFF, 0xFFFFFFFF] and m.selected().sum() == 33
    n_bytes = len(m.pos_blob)
    assert m.translate((1.0, 1.0, 1.0)) and len(m.pos_blob) == n_bytes == 33 * 12


@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), (0.75, -1.25, 0.5), (-1.99609375, 1.5, 0.00390625)])
def test_identity_rotation_and_unit_scale_give_the_mouse_down_state_back(centre):
    """Identity transform, identity quaternion / scale (1, 1, 1).  mul(I, p) and QuatRotateVector(p, identity) are exact; (p - c) + c is exact when p and c
    lie on a common binary grid (grid_asset) or c = 0 -- for an ARBITRARY centre it is not a float32 identity (asserted at the end)."""
    m = TM.TransformModel(grid_asset(400))
    flags = half_selected(m)
    m.store_pos(); m.store_other()
    pos0, words0 = m.pos_rows().copy(), m.rot_words().copy()
    quat0 = TM.decode_rotation(words0)
    assert m.translate((0.5, 0.25, -0.125))                       # the current blob moves away from the mouse-down copy ...
    assert (m.pos_rows()[flags] != pos0[flags]).any()
    assert m.rotate(centre, EYE, EYE, IDENT_Q)                    # ... and rotate goes back to it
    assert np.array_equal(bits(m.pos_rows()), bits(pos0))
    # the re-encoded words decode to the quaternion they decoded to before (QuatMul(q, identity) = q exactly); almost all are the same word
    assert np.array_equal(bits(TM.decode_rotation(m.rot_words())), bits(quat0))
    assert np.array_equal(m.rot_words()[~flags], words0[~flags])
    assert m.translate((0.5, 0.25, -0.125))
    assert m.scale(centre, EYE, EYE, (1.0, 1.0, 1.0))
    assert np.array_equal(bits(m.pos_rows()), bits(pos0))
    # the premise of the grid: with a centre off it, some last bits change
    off = TM.rotate_pos(pos0, (0.123456789, -1.987654321, 0.3333333), EYE, EYE, IDENT_Q)
    assert not np.array_equal(bits(off), bits(pos0)) and np.abs(off - pos0).max() <= 2.0 ** -22


def test_turns_about_z():
    """A half turn about z, q = (0, 0, 1, 0), maps (1, 0, 0) to (-1, 0, 0) exactly.  A quarter turn, q = (0, 0, s, s) with s = float32(sqrt(1/2)), maps it to
    (1 - 2 s s, 2 s s, 0) in the reference's operation order: s s rounds to 0.5 - 2^-25, so the result is (2^-24, 1 - 2^-24, 0) -- (0, 1, 0) to within one
    rounding of a number near 1, which is all a float32 unit quaternion can give (no float32 s has 2 s s = 1)."""
    p = np.array([[1.0, 0.0, 0.0]], f32)
    half = TM.rotate_pos(p, (0.0, 0.0, 0.0), EYE, EYE, (0.0, 0.0, 1.0, 0.0))
    assert half.tolist() == [[-1.0, 0.0, 0.0]]
    s = np.sqrt(f32(0.5))
    assert type(s) is f32
    quarter = TM.rotate_pos(p, (0.0, 0.0, 0.0), EYE, EYE, (0.0, 0.0, s, s))
    assert quarter.tolist() == [[2.0 ** -24, 1.0 - 2.0 ** -24, 0.0]]
    assert np.abs(quarter - np.array([[0.0, 1.0, 0.0]], f32)).max() <= 2.0 ** -24
    # about a centre, through a transform that moves and mirrors: back in place after the inverse
    tr = camera.Transform(position=(0.5, -1.0, 2.0), scale=(1.0, 1.0, -1.0))
    q = TM.rotate_pos(p, (1.0, 0.0, 0.0), tr.localToWorldMatrix, tr.worldToLocalMatrix, (0.0, 0.0, 1.0, 0.0))
    # p - c = 0 goes to the world point (0.5, -1, 2); the half turn about the world's z axis takes it to (-0.5, 1, 2); back in object space, plus c: (0, 2, 0)
    assert np.abs(q - np.array([[0.0, 2.0, 0.0]], f32)).max() <= 1e-6


def test_rotate_and_scale_need_their_mouse_down_copies():
    m = TM.TransformModel(EM.point_asset(65))
    m.select_all()
    before = m.pos_blob.copy()
    assert not m.rotate((0, 0, 0), EYE, EYE, (0.0, 0.0, 1.0, 0.0)) and not m.scale((0, 0, 0), EYE, EYE, (2.0, 2.0, 2.0))
    m.store_pos()
    assert not m.rotate((0, 0, 0), EYE, EYE, (0.0, 0.0, 1.0, 0.0))      # both copies
    assert np.array_equal(m.pos_blob, before)
    assert m.scale((0, 0, 0), EYE, EYE, (2.0, 2.0, 2.0))
    assert np.array_equal(bits(m.pos_rows()), bits(before[:65 * 12].view(f32).reshape(65, 3) * f32(2.0)))
    m.store_other()
    assert m.rotate((0, 0, 0), EYE, EYE, (0.0, 0.0, 1.0, 0.0))
    m.release()
    assert not m.scale((0, 0, 0), EYE, EYE, (2.0, 2.0, 2.0))      # the copies went with the release; the moved splats stay
    assert not np.array_equal(m.pos_blob, before)


def test_the_format_gates():
    from common import small_asset
    chunked = TM.TransformModel(small_asset(257, 5, "Medium"))
    assert not chunked.pos_gate and not chunked.rot_gate
    chunked.select_all(); chunked.store_pos(); chunked.store_other()
    p0, o0 = chunked.pos_blob.copy(), chunked.other_blob.copy()
    assert chunked.translate((1, 2, 3)) and chunked.rotate((0, 0, 0), EYE, EYE, (0.0, 0.0, 1.0, 0.0)) and chunked.scale((0, 0, 0), EYE, EYE, (2, 2, 2))
    assert np.array_equal(chunked.pos_blob, p0) and np.array_equal(chunked.other_blob, o0) and chunked.pos_md is None and chunked.other_md is None
    half = TM.TransformModel(pos_only_asset(257))
    assert half.pos_gate and not half.rot_gate
    half.select_all(); half.store_pos(); half.store_other()
    p0, o0 = half.pos_blob.copy(), half.other_blob.copy()
    assert half.rotate((0, 0, 0), EYE, EYE, (0.0, 0.0, 1.0, 0.0))
    assert np.array_equal(half.other_blob, o0) and not np.array_equal(half.pos_blob, p0)


# ---- 3. the codec against the reference's compiled text -------------------------------------------------------------------------------------
def codec_quaternions():
    rng = np.random.default_rng(31)
    q = rng.standard_normal((4000, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    h, r = f32(0.5), np.sqrt(f32(0.5))
    ties = []
    for sx in (1, -1):
        for sw in (1, -1):
            ties += [(sx * h, h, h, sw * h), (sx * h, -h, h, sw * h)]                    # four equal magnitudes: index 0 wins
    for i in range(4):
        for j in range(i + 1, 4):
            for sgn in (1, -1):
                t = np.zeros(4, f32); t[i] = r; t[j] = sgn * r; ties.append(tuple(t))   # two equal magnitudes: the first wins
    for w in (0.0, -0.0):                                                               # w = +-0: q.w >= 0 holds for both
        ties += [(1.0, 0.0, 0.0, w), (0.0, -1.0, 0.0, w), (r, r, 0.0, w), (0.6, 0.0, 0.8, w)]
    return np.concatenate([q, np.array(ties, f32)])


@pytest.mark.parametrize("which", ["strict", "fused"])
def test_pack_and_encode_equal_the_reference_text(which):
    L = ref_lib.lib(which)
    q = codec_quaternions()
    packed = TM.pack_smallest3(q)
    enc = TM.encode_quat_norm10(packed, clamp=False)
    assert np.array_equal(enc, TM.encode_quat_norm10(packed, clamp=True))              # in range: the clamp changes nothing
    out = np.zeros(4, f32)
    for i in range(len(q)):
        L.gsr_cs_pack_smallest3(q[i].ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(bits(out), bits(packed[i])), (i, q[i], out, packed[i])
        assert int(L.gsr_cs_encode_quat_norm10(out.ctypes.data_as(C.c_void_p))) == int(enc[i]), (i, q[i])
    assert set((enc >> np.uint32(30)).tolist()) == {0, 1, 2, 3}
    n_ties = len(q) - 4000
    assert (enc[4000:4008] >> np.uint32(30)).tolist() == [0] * 8 and n_ties == 8 + 12 + 8


def test_decode_equals_the_reference_text():
    """The product's DecodeRotation is the fused member (mad chains); bit-equal to the `fused` build under the compiler that build is pinned to.  The strict build
    rounds every operation on its own: within 4 float32 ulps of a number below 1 per component of x y z, and w = sqrt(1 - d) within what d's error allows."""
    words = np.concatenate([TM.encode_quat_norm10(TM.pack_smallest3(codec_quaternions())), np.array([0, 0xFFFFFFFF, 0x3FFFFFFF, 0xC0000000, 1023 << 10], np.uint32)])
    got = TM.decode_rotation(words)
    out = np.zeros(4, f32)
    for which in ("fused", "strict"):
        L = ref_lib.lib(which)
        ref = np.zeros_like(got)
        for i, w in enumerate(words):
            L.gsr_cs_decode_rotation(C.c_uint32(int(w)), out.ctypes.data_as(C.c_void_p))
            ref[i] = out
        if which == "fused" and ref_lib.fused_is_pinned():
            assert np.array_equal(bits(ref), bits(got))
        else:
            idx = (words >> np.uint32(30)).astype(int)
            wcol = np.where(idx == 3, 3, idx)
            xyz = np.ones_like(got, bool); xyz[np.arange(len(words)), wcol] = False
            assert np.abs(ref - got)[xyz].max() <= 4 * 2.0 ** -24
            d = np.abs(ref.astype(np.float64) ** 2 - got.astype(np.float64) ** 2)[~xyz]      # w^2 = 1 - d: compare d, not its square root near 0
            assert d.max() <= 16 * 2.0 ** -24


# ---- 4. the clamp -----------------------------------------------------------------------------------------------------------------------
def test_a_delta_quaternion_of_length_two_stays_inside_the_fields():
    q = codec_quaternions()[:4000]
    words = TM.encode_quat_norm10(TM.pack_smallest3(q))
    delta = np.array([0.6, 0.0, 0.8, 0.0], f32) * f32(2.0)
    prod = TM.quat_mul(TM.decode_rotation(words), delta)
    packed = TM.pack_smallest3(prod)
    assert ((packed[:, :3] > 1.0) | (packed[:, :3] < 0.0)).any(axis=1).mean() > 0.5           # the premise: out of range without the clamp
    out = TM.rotate_words(words, delta)
    fields = np.stack([(out >> np.uint32(s)) & np.uint32(1023) for s in (0, 10, 20)], axis=1)
    with np.errstate(all="ignore"):
        want = np.clip(np.trunc((packed[:, :3] * f32(1023.5)).astype(f32)), 0, 1023).astype(np.uint32)
    assert np.array_equal(fields, want)                                                       # every field is its own value, clamped: nothing spills
    assert np.array_equal(out >> np.uint32(30), np.rint(packed[:, 3] * 3).astype(np.uint32))
    # a NaN and infinities
    weird = np.array([[np.nan, 0.2, 0.3, 0.0], [np.inf, -np.inf, 0.5, 1.0], [2.0, -1.0, 0.5, 5.0]], f32)
    assert TM.encode_quat_norm10(weird).tolist() == [0 | (204 << 10) | (307 << 20), 1023 | (0 << 10) | (511 << 20) | (3 << 30), 1023 | (0 << 10) | (511 << 20) | (3 << 30)]


# ---- 5. the host build of the kernels' arithmetic against the model ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def th(tmp_path_factory):
    return C.CDLL(build_harness(tmp_path_factory.mktemp("th"), "transform_host_harness.cpp"))


def test_host_build_of_the_codec_equals_the_model(th):
    q = codec_quaternions()
    q = np.concatenate([q, q[:500] * f32(2.0), np.array([[np.nan, 0.1, 0.2, 0.3], [0.0, 0.0, 0.0, 0.0], [np.inf, 1.0, -np.inf, 0.0]], f32)])
    n = len(q)
    packed, enc, dec = np.zeros((n, 4), f32), np.zeros(n, np.uint32), np.zeros((n, 4), f32)
    th.th_codec(_p(q), C.c_uint32(n), _p(packed), _p(enc), _p(dec))
    want_packed = TM.pack_smallest3(q)
    assert same_floats(packed, want_packed)
    assert np.array_equal(enc, TM.encode_quat_norm10(want_packed))
    assert same_floats(dec, TM.decode_rotation(enc))


def test_host_build_of_the_transform_arithmetic_equals_the_model(th):
    rng = np.random.default_rng(77)
    n = 3000
    transforms = [camera.Transform(), camera.Transform(position=(0.1, -0.2, 0.3), rotation=(0.1, 0.2, 0.05, 0.9695), scale=(1.5, 0.5, 2.0)),
                  camera.Transform(position=(-0.3, 0.1, 0.0), scale=(1.0, 1.0, -1.0)),
                  camera.Transform(position=(3.0, 1.0, -2.0), rotation=(0.5, -0.5, 0.5, 0.5), scale=(-0.75, 1.25, 3.0))]
    for case in range(40):
        pos = (rng.standard_normal((n, 3)) * rng.choice([0.1, 2.0, 50.0])).astype(f32)
        pos[0] = (np.nan, 1.0, -1.0); pos[1] = (np.inf, 0.0, 0.0); pos[2] = (0.0, -0.0, 1e-40)
        words = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        centre = (rng.standard_normal(3) * 2.0).astype(f32)
        tr = transforms[case % 4]
        l2w, w2l = np.ascontiguousarray(tr.localToWorldMatrix, f32), np.ascontiguousarray(tr.worldToLocalMatrix, f32)
        rot = rng.standard_normal(4)
        rot = (rot / np.linalg.norm(rot) * (1.0 if case % 5 else 2.0)).astype(f32)           # every fifth: not of unit length
        delta = (rng.standard_normal(3) * 1.5).astype(f32)
        if case % 7 == 0:
            delta[case % 3] = 0.0 if case % 2 else -delta[case % 3]
        outT, outR, outS, outW = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, np.uint32)
        th.th_eval(_p(pos), _p(words), C.c_uint32(n), _p(centre), _p(l2w), _p(w2l), _p(delta), _p(rot), _p(outT), _p(outR), _p(outS), _p(outW))
        with np.errstate(all="ignore"):
            assert same_floats(outT, TM.translate_pos(pos, delta)), case
            assert same_floats(outR, TM.rotate_pos(pos, centre, l2w, w2l, rot)), case
            assert same_floats(outS, TM.scale_pos(pos, centre, l2w, w2l, delta)), case
            assert np.array_equal(outW, TM.rotate_words(words, rot)), case
