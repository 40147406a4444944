"""The merge on the CPU box: the C-ABI surface of gs_renderer_edit_set_splat_count / _copy_splats_into / _download_splat_data / gs_renderer_splat_count,
the host build of gsm::CopySplat (tests/copy_host_harness.cpp) against the numpy model of CSCopySplats (tests/copy_model.py) bit for bit -- a NaN
equal to any NaN -- over every source preset, the identity's known answers, the literal idx / srcIdx split, and the resize bookkeeping."""
import ctypes as C
import os

import numpy as np
import pytest

import copy_model as CM
import edit_model as EM
import transform_model as TM
from builders import DST_TR, SRC_TR, params_of
from common import PRESETS, _p, small_asset
from harness import FP, build_harness, run_under_sanitizers
from unitygaussiansplatting_amd import _abi, _lib, asset as A, camera, creator, renderer
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32


@pytest.fixture(scope="module")
def ch(tmp_path_factory):
    L = C.CDLL(build_harness(tmp_path_factory.mktemp("ch"), "copy_host_harness.cpp"))
    L.ch_sizes.restype = C.c_uint32
    return L


def host_records(ch, asset, transform=None, first=0, n=None):
    keep = []
    desc = _abi.make_asset_desc(asset, keep)
    n = asset.splatCount - first if n is None else n
    pos, other, texel, sh = np.zeros((n, 3), f32), np.zeros((n, 4), np.uint32), np.zeros((n, 4), f32), np.zeros((n, 45), f32)
    p = None if transform is None else C.byref(params_of(transform))
    ch.ch_copy(C.byref(desc), p, C.c_uint32(first), C.c_uint32(n), _p(pos), _p(other), _p(texel), _p(sh))
    return pos, other, texel, sh


def same_bits_nan(got, want) -> bool:
    """bit for bit, a NaN equal to any NaN"""
    g, w = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    return g.shape == w.shape and bool(((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())


def assert_records_equal(got, want, what):
    for name, g, w in zip(("pos", "other", "texel", "sh"), got, want):
        if name == "other":                                        # the rotation word exactly; the scales as floats
            assert np.array_equal(g[:, 0], w[:, 0]), (what, "rotation word", np.flatnonzero(g[:, 0] != w[:, 0])[:6])
            g, w = g[:, 1:].copy().view(f32), w[:, 1:].copy().view(f32)
        assert same_bits_nan(g, w), (what, name, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:6])


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_merge_entry_points_validate_their_arguments(ch):
    lib = _lib.lib()
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    assert C.sizeof(_abi.gs_copy_params) == (16 + 4 + 3) * 4 == ch.ch_sizes(0)
    assert ch.ch_sizes(1) == (12 + 4 + 3 + 83) * 4               # matrix rows 0..2, rotation, scale, the band matrices: a kernel argument
    n = C.c_uint32(7)
    p = _abi.gs_copy_params()
    some = C.create_string_buffer(64)
    assert lib.gs_renderer_splat_count(None, C.byref(n)) == bad and n.value == 7
    assert lib.gs_renderer_edit_set_splat_count(None, 10, None) == bad
    assert lib.gs_renderer_edit_set_splat_count(None, 10, C.byref(p)) == bad
    assert lib.gs_renderer_edit_copy_splats_into(None, None, C.byref(p), 0, 0, 1) == bad
    assert lib.gs_renderer_edit_copy_splats_into(None, some, None, 0, 0, 1) == bad       # (`some` is never dereferenced)
    assert lib.gs_renderer_edit_copy_splats_into(some, None, None, 0, 0, 1) == bad
    assert lib.gs_renderer_edit_copy_splats_into(some, some, None, 0, 0, 1) == bad       # src == dst is refused before either is looked at
    assert lib.gs_renderer_edit_download_splat_data(None, some, 1, None, 0, None, 0, None, 0) == bad
    assert lib.gs_abi_version() == 9                             # additions to ABI 9


def test_renderer_mirrors_the_merge_methods():
    for name in ("EditSetSplatCount", "EditCopySplatsInto", "DownloadSplatData", "CopyParams"):
        assert callable(getattr(GaussianSplatRenderer, name)), name
    assert callable(renderer.MergeSplatObjects)
    src, dst = GaussianSplatRenderer.__new__(GaussianSplatRenderer), GaussianSplatRenderer.__new__(GaussianSplatRenderer)      # no context: CopyParams reads the transforms only
    src.transform, dst.transform = SRC_TR, DST_TR
    p = src.CopyParams(dst)
    m, q, s = CM.copy_transform(SRC_TR, DST_TR)
    assert np.array_equal(np.array(p.matrix[:], f32).reshape(4, 4), m) and list(p.rotation) == [float(v) for v in q] and list(p.scale) == [float(v) for v in s]
    assert np.array_equal(m, camera.mat_mul(DST_TR.worldToLocalMatrix, SRC_TR.localToWorldMatrix)) and m.dtype == f32


def test_matrix_decomposition():
    """camera.matrix_rotation_scale: column lengths, x negated under a negative determinant; the quaternion of the normalised columns"""
    rng = np.random.default_rng(3)
    for k in range(40):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        s = rng.uniform(0.3, 3.0, 3) * (rng.choice([-1.0, 1.0], 3) if k % 2 else 1.0)
        tr = camera.Transform(position=tuple(rng.standard_normal(3)), rotation=tuple(q), scale=tuple(s))
        M = np.asarray(tr.localToWorldMatrix, np.float64)
        gq, gs = camera.matrix_rotation_scale(M)
        assert gq.dtype == f32 and gs.dtype == f32
        assert np.allclose(np.abs(gs), np.abs(s), rtol=1e-5) and (gs[1:] > 0).all() and (gs[0] < 0) == (np.prod(s) < 0)
        back = camera.quat_to_mat3(gq) @ np.diag(gs.astype(np.float64))
        assert np.allclose(back, M[:3, :3], atol=2e-5), k        # rotation x scale reproduces the matrix (what the kernel's flips assume of a mirror in x)
        assert abs(float(np.linalg.norm(gq.astype(np.float64))) - 1.0) < 1e-6
    gq, gs = camera.matrix_rotation_scale(np.eye(4, dtype=f32))
    assert gq.tolist() == [0.0, 0.0, 0.0, 1.0] and gs.tolist() == [1.0, 1.0, 1.0]


# ---- 2. the host build against the model, every source preset -----------------------------------------------------------------------------
@pytest.mark.parametrize("quality", PRESETS)
def test_host_build_of_copy_splat_equals_the_model(ch, quality):
    asset = small_asset(20000, 5, quality)                        # (Cluster16k needs more than 16,384 splats; 78 chunks + 32 splats)
    dec = CM.decode(asset)
    for what, tr in (("identity", None), ("mirrored", CM.copy_transform(SRC_TR, DST_TR))):
        want = CM.copy_records(dec, tr)
        got = host_records(ch, asset, tr)
        assert_records_equal(got, want, (quality, what))
    ident = CM.copy_records(dec, None)
    assert not same_bits_nan(ident[3], want[3]) and not same_bits_nan(ident[0], want[0]) and (ident[1][:, 0] != want[1][:, 0]).any()      # the transform did something


# ---- 3. known answers ---------------------------------------------------------------------------------------------------------------------
def test_identity_copies_a_very_high_source_byte_for_byte(ch):
    """With the exact identity, pos, scale, colour, opacity and SH bytes are the source's and the rotation word is the model's re-encoding of the
    decoded word.  x * 1 + 0 turns -0 into +0 and a NaN's payload is not defined, so the case asserts that the source holds neither."""
    asset = small_asset(5003, 5, "VeryHigh")
    src = CM.blobs_of(asset)
    floats = np.concatenate([src.pos.view(f32), src.other.view(f32).reshape(-1, 4)[:, 1:].reshape(-1), src.sh.view(f32).reshape(-1, 48)[:, :45].reshape(-1)])
    assert not np.isnan(floats).any() and not ((floats == 0) & np.signbit(floats)).any() and np.isfinite(floats).all()
    n = asset.splatCount
    pos, other, texel, sh = host_records(ch, asset, None)
    assert np.array_equal(pos.view(np.uint32), src.pos.view(np.uint32).reshape(n, 3))
    assert np.array_equal(other[:, 1:], src.other.view(np.uint32).reshape(n, 4)[:, 1:])
    assert np.array_equal(sh.view(np.uint32), src.sh.view(np.uint32).reshape(n, 48)[:, :45])
    tex = src.color.view(np.uint32).reshape(-1, 4)[creator.SplatIndexToTextureIndex(np.arange(n, dtype=np.uint32))]
    assert np.array_equal(texel.view(np.uint32), tex)
    words = src.other.view(np.uint32).reshape(n, 4)[:, 0]
    assert np.array_equal(other[:, 0], TM.encode_quat_norm10(TM.pack_smallest3(TM.decode_rotation(words))))
    # ... and the model of a whole resize to the same layout reproduces the source's blobs but for the rotation words
    out = CM.set_splat_count(CM.decode(asset), None, n)
    assert np.array_equal(out.pos, src.pos) and np.array_equal(out.sh.view(np.uint32).reshape(n, 48)[:, :45], src.sh.view(np.uint32).reshape(n, 48)[:, :45])
    assert np.array_equal(out.color.view(np.uint32).reshape(-1, 4)[creator.SplatIndexToTextureIndex(np.arange(n, dtype=np.uint32))], tex)
    assert not out.deleted.any() and len(out.deleted) == (n + 31) // 32


def test_src_start_copies_the_data_of_idx_with_the_deleted_bits_of_src_idx(ch):
    """SplatUtilities.compute:697: LoadSplatData(idx), while the bounds check and the deleted bit use srcIdx = srcStart + idx"""
    asset = small_asset(300, 5, "VeryHigh")
    dec = CM.decode(asset)
    flags = np.zeros(300, bool)
    flags[[5, 6, 36, 37, 299]] = True                              # srcIdx 5, 6 -> dst bits 0, 1; 36, 37 -> 31, 32 (both sides of a word boundary)
    words = EM.pack_bits(flags, 10)
    dst = CM.zero_blobs(64)
    dst.deleted = None
    CM.copy_splats(dec, words, dst, None, 5, 0, 300)               # count runs past both ends: 64 records (dst), and srcIdx < 300
    want = CM.copy_records(dec[:64], None)                         # the records of idx 0 .. 63, not 5 .. 68
    assert np.array_equal(dst.pos.view(f32).reshape(64, 3).view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(dst.other.view(np.uint32).reshape(64, 4), want[1])
    got = host_records(ch, asset, None, 0, 64)
    assert_records_equal(got, want, "src_start 5")
    assert EM.unpack_bits(dst.deleted, 64).nonzero()[0].tolist() == [0, 1, 31, 32] and len(dst.deleted) == 2
    # src_start + count past the source's end clamps: srcIdx 296 .. 299 only
    dst2 = CM.zero_blobs(64)
    CM.copy_splats(dec, words, dst2, None, 296, 10, 40)
    assert np.array_equal(dst2.pos.view(f32).reshape(64, 3)[10:14].view(np.uint32), want[0][0:4].view(np.uint32))
    assert not dst2.pos.view(f32).reshape(64, 3)[14:].any() and not dst2.pos.view(f32).reshape(64, 3)[:10].any()
    assert EM.unpack_bits(dst2.deleted, 64).nonzero()[0].tolist() == [13]      # srcIdx 299 -> dstIdx 13


# ---- 4. the resize bookkeeping ------------------------------------------------------------------------------------------------------------
def test_resize_model_shrinks_grows_and_never_writes_beyond_n():
    asset = small_asset(300, 5, "VeryHigh")
    dec = CM.decode(asset)
    words = EM.pack_bits(np.random.default_rng(9).random(300) < 0.5, 10)
    small = CM.set_splat_count(dec, words, 130)
    assert small.n == 130 and len(small.pos) == 130 * 12 and len(small.sh) == 130 * 192 and len(small.deleted) == 5
    assert np.array_equal(EM.unpack_bits(small.deleted, 160)[:130], EM.unpack_bits(words, 300)[:130]) and not EM.unpack_bits(small.deleted, 160)[130:].any()
    assert not small.sh.view(np.uint32).reshape(130, 48)[:, 45:].any()      # the pad of a zero-filled buffer stays zero
    texels = small.color.view(np.uint32).reshape(-1, 4)
    used = np.zeros(len(texels), bool)
    used[creator.SplatIndexToTextureIndex(np.arange(130, dtype=np.uint32))] = True
    assert not texels[~used].any() and texels[used].any(axis=1).all()
    big = CM.set_splat_count(dec, words, 1000)
    assert np.array_equal(big.pos[:300 * 12], CM.set_splat_count(dec, words, 300).pos) and not big.pos[300 * 12:].any()
    assert A.CalcTextureSize(32700) == (2048, 16) and A.CalcTextureSize(32800) == (2048, 32)      # the second Morton band starts at 32,768
    assert len(CM.zero_blobs(32800).color) == 2048 * 32 * 16


def test_merge_model_counts():
    target, a, b = small_asset(300, 5, "VeryHigh"), small_asset(257, 6, "Medium"), small_asset(65, 7, "VeryHigh")
    out = CM.merge(CM.blobs_of(target), DST_TR, [(CM.decode(a), None, camera.Transform()), (CM.decode(b), None, SRC_TR)])
    assert out.n == 622 and not out.deleted.any()
    ident = CM.copy_records(CM.decode(target), None)
    assert np.array_equal(out.pos.view(np.uint32).reshape(622, 3)[:300], ident[0].view(np.uint32))
    assert out.pos.view(f32).reshape(622, 3)[300:].any(axis=1).all()
    # premise of the GPU test of the edit tools: a rectangle through the first test camera selects splats of the target and of the merged ones
    from common import default_camera
    m = EM.EditModel(out.asset())
    m.select_all()
    assert m.info()[0] == 640                                      # the tail bits of the last word count
    m.deselect_all(); m.store_selection()
    probe = GaussianSplatRenderer.__new__(GaussianSplatRenderer)
    probe.transform, probe.m_SplatScale, probe.m_OpacityScale, probe.m_SHOrder, probe.m_SHOnly = DST_TR, 1.0, 1.0, 3, False
    m.update_selection(probe.FrameParams(default_camera(az=25.0)), EM.PREMISE_RECT, False)
    flags = EM.unpack_bits(m.bits()[0], 622)
    assert int(flags.sum()) == 134 and int(flags[300:].sum()) == 84


# ---- 5. the kernel's own text, thread for thread on the host ------------------------------------------------------------------------------
def kernel_text() -> str:
    """copy_splats_kernel and what it needs, cut out of csrc/gs_copy.hip: from its first constant to the line before the host part"""
    src = open(os.path.join(HERE, "..", "unitygaussiansplatting_amd", "csrc", "gs_copy.hip")).read()
    a, b = src.index("constexpr uint32_t kCopySHFloats"), src.index("// ---- host ---")
    text = src[a:b]
    assert "copy_splats_kernel" in text and "hipLaunchKernelGGL" not in text
    return text


def test_kernel_text_run_thread_for_thread_equals_the_model(tmp_path):
    """tests/copy_kernel_host_emulation.cpp: every offset case of the GPU test, the destinations' shared deleted words, the literal src_start, both
    clamps, count = 0, the SH pad and the texels nobody writes -- all four blobs and the deleted words byte for byte after every call"""
    inc = tmp_path / "kernel_text.inc"
    inc.write_text(kernel_text())
    L = C.CDLL(build_harness(tmp_path, "copy_kernel_host_emulation.cpp", ["-O1", "-std=c++20", "-pthread"] + FP, [f'COPY_KERNEL_TEXT="{inc}"']))

    def bits(n):
        flags = np.zeros(n, bool)
        flags[[k for k in (0, 31, 32, 63, 64, 255, 256, n - 1) if k < n]] = True
        return EM.pack_bits(flags, (n + 31) // 32)

    for dst_n in (33, 257, 300, 1000):
        want = CM.zero_blobs(1000) if dst_n == 1000 else CM.blobs_of(small_asset(dst_n, 5, "VeryHigh"))
        want.deleted = np.zeros(want.words, np.uint32)
        got = want.copy()
        for n, quality in ((1, "VeryHigh"), (63, "VeryHigh"), (65, "VeryHigh"), (257, "Medium"), (513, "High")):
            asset = small_asset(n, 5, quality)
            dec, words = CM.decode(asset), (bits(n) if n >= 65 else None)
            xf = CM.copy_transform(SRC_TR if n in (65, 513) else camera.Transform(), DST_TR)
            keep = []
            desc, p = _abi.make_asset_desc(asset, keep), params_of(xf)
            for src_start, dst_start, count in ((0, 0, n), (0, 33, n), (0, 95, n + 100), (5, 33, 600), (0, 0, 0)):
                CM.copy_splats(dec, words, want, xf, src_start, dst_start, count)
                L.emu_copy(C.byref(desc), None if words is None else _p(words), C.byref(p), _p(got.pos), _p(got.other), _p(got.color), _p(got.sh), _p(got.deleted),
                           C.c_uint32(dst_n), C.c_uint32(src_start), C.c_uint32(dst_start), C.c_uint32(count))
                for f in ("pos", "other", "color", "sh", "deleted"):
                    assert np.array_equal(getattr(got, f), getattr(want, f)), (dst_n, n, quality, src_start, dst_start, count, f)
        assert want.deleted.any() and want.pos.any()


# ---- 6. the harness as a stand-alone program under the host sanitizers --------------------------------------------------------------------
def test_stand_alone_harness_runs_clean_under_the_host_sanitizers(tmp_path):
    out = run_under_sanitizers(tmp_path, "copy_host_harness.cpp", "COPY_HARNESS_MAIN")
    assert out.returncode == 0 and "copy harness ok" in out.stdout, (out.stdout, out.stderr[-2000:])
