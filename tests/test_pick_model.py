"""-m "not gpu": the premises of the pick output's parity tests, from the CPU oracle alone (tests/pick_model.py), and the surface the feature adds to the
host layers.  The GPU tests (tests/test_gpu_pick.py) hold the records to this model; here the model is held to what it claims: the fixed scenes stay inside
the ambiguity cap and are not vacuous, the last prefix is the whole frame, and the numpy twin of select_surface does what the header says."""
import os
import re

import numpy as np
import pytest

import pick_model as PM
from unitygaussiansplatting_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("scene", [s.name for s in PM.SCENES])
def test_fixed_scenes_are_inside_the_cap_and_not_vacuous(scene, mode):
    orc, P, exp = PM.scene_expected(scene, mode)
    w = orc.view["pos"][:, 3]
    for tau, e in exp.items():
        crossed, amb = e.shares()
        print(scene, "mode", mode, "tau", tau, f"crossed {crossed:.3f} ambiguous {amb:.4f} covered {int(e.covered.sum())}")
        assert amb <= PM.AMBIGUOUS_CAP, (scene, mode, tau, amb)
        assert e.covered.sum() > 0.5 * e.covered.size
        if tau == 0.5:
            assert e.crossed.sum() >= 0.5 * e.crossed.size, (scene, mode, float(e.crossed.mean()))      # at least half the pixels are crossed
        assert PM.consistent(e.records, w, orc.n).all()
        assert (e.records["splat"][e.crossed] < orc.n).all() and (e.records["splat"][~e.crossed] == _abi.GS_PICK_NO_SPLAT).all()
        assert np.isinf(e.records["depth"][~e.crossed]).all() and (e.records["depth"][e.crossed] > 0).all()
    # a higher threshold is crossed later or never: depth order along the draw order is the sort's, so only "never" is checked
    assert not (exp[0.95].crossed & ~exp[0.5].crossed).any()


def test_a_draw_without_a_clear_keeps_the_records_of_crossed_pixels():
    """two halves of one draw order, the second onto the first's target: the records are those of the whole draw"""
    import ctypes as C
    import oracle_lib as O
    from common import _p
    orc, P, exp = PM.scene_expected(PM.SCENES[0].name, 0)
    whole = exp[0.5]
    order = PM.draw_order(orc, P)
    half = len(order) // 3
    keep = orc.order
    try:
        orc.order = order[:half]
        first = PM.expected(orc, P, 0, (0.5,), tag=1)[0.5]
        rt = np.zeros((int(P.screen_h), int(P.screen_w), 4), np.uint16)
        O.lib().gso_draw_ex(_p(orc.view), _p(orc.order), C.c_uint32(half), C.byref(P), C.c_int32(0), _p(rt), None, None, None, None)
        orc.order = order[half:]
        second = PM.expected(orc, P, 0, (0.5,), tag=2, start=rt, start_records=first.records)[0.5]
    finally:
        orc.order = keep
    assert np.array_equal(second.crossed, whole.crossed)
    assert np.array_equal(second.records["splat"], whole.records["splat"]) and np.array_equal(second.records["depth"].view(np.uint32), whole.records["depth"].view(np.uint32))
    assert set(np.unique(second.records["tag"][second.crossed]).tolist()) == {1, 2} and (second.records["tag"][first.crossed] == 1).all()


def test_select_surface_twin():
    rec = PM.none_records(4, 6)
    def put(x, y, splat, tag):
        rec[y, x] = (1.0, splat, tag, 0)
    put(0, 0, 3, 7); put(1, 0, 40, 7); put(2, 1, 40, 7); put(5, 3, 65, 7); put(3, 2, 9, 8); put(4, 2, 70, 7)      # 70 >= n
    n, words = 66, 3
    zero = np.zeros(words, np.uint32)
    got = PM.select_surface(rec, zero, (0, 0, 5, 3), 7, n)
    assert got.tolist() == [1 << 3, 1 << 8, 1 << 1]
    assert PM.select_surface(rec, zero, (-5, -5, 0, 0), 7, n).tolist() == [1 << 3, 0, 0]                            # clipped; a click on pixel (0, 0)
    assert PM.select_surface(rec, zero, (6, 0, 9, 3), 7, n).tolist() == [0, 0, 0]                                   # wholly outside
    assert PM.select_surface(rec, zero, (0, 0, 5, 3), 9, n).tolist() == [0, 0, 0]                                   # a tag nobody drew with
    assert PM.select_surface(rec, got, (1, 0, 2, 1), 7, n, subtract=True).tolist() == [1 << 3, 0, 1 << 1]
    deleted = np.array([0, 1 << 8, 0], np.uint32)
    assert PM.select_surface(rec, zero, (0, 0, 5, 3), 7, n, deleted=deleted).tolist() == [1 << 3, 0, 1 << 1]
    cut = np.zeros(n, bool); cut[65] = True
    assert PM.select_surface(rec, zero, (0, 0, 5, 3), 7, n, cut=cut).tolist() == [1 << 3, 1 << 8, 0]


def test_consistent_rejects_a_wrong_depth_and_a_stray_tag():
    w = np.array([1.5, 2.5, 3.5], np.float32)
    rec = PM.none_records(1, 3)
    rec[0, 1] = (2.5, 1, 0, 0)
    assert PM.consistent(rec, w, 3).all()
    rec[0, 2] = (2.5, 2, 0, 0)
    assert PM.consistent(rec, w, 3).tolist() == [[True, True, False]]
    rec[0, 2] = (3.5, 2, 4, 0)
    assert PM.consistent(rec, w, 3).tolist() == [[True, True, False]] and PM.consistent(rec, w, 3, tags=(0, 4)).all()
    rec[0, 0] = (np.inf, 5, 0, 0)
    assert not PM.consistent(rec, w, 3)[0, 0]


NEW_CALLS = ("gs_target_set_pick_output", "gs_target_download_pick", "gs_target_pick_at", "gs_target_pick_device_ptr", "gs_renderer_set_pick_tag",
             "gs_renderer_edit_select_surface")


def test_the_new_calls_are_declared_in_every_layer():
    hdr = open(os.path.join(ROOT, "include", "gsplat_c.h")).read()
    cs = open(os.path.join(ROOT, "unitygaussiansplatting_amd", "dotnet", "GaussianSplatNative.cs")).read()
    lib = _lib.lib()
    for name in NEW_CALLS:
        assert re.search(r"int32_t\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"extern\s+int\s+" + name + r"\s*\(", cs), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define\s+GS_ABI_VERSION\s+9\b", hdr) and C_sizeof_pick() == 16 and PM.PICK.itemsize == 16
    for rel in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "gs_target_set_pick_output" in open(os.path.join(ROOT, rel)).read(), rel


def C_sizeof_pick() -> int:
    import ctypes as C
    return C.sizeof(_abi.gs_pick_record)


def test_null_handles_and_bad_thresholds_are_refused_without_a_device():
    import ctypes as C
    lib = _lib.lib()
    BAD = _abi.GS_ERR_INVALID_ARGUMENT
    assert lib.gs_target_set_pick_output(None, 1, 0.5) == BAD
    assert lib.gs_target_download_pick(None, None, 0) == BAD
    assert lib.gs_target_pick_at(None, 0, 0, C.byref(_abi.gs_pick_record())) == BAD
    assert lib.gs_target_pick_device_ptr(None, None) == BAD
    assert lib.gs_renderer_set_pick_tag(None, 1) == BAD
    assert lib.gs_renderer_edit_select_surface(None, None, 0, 0, 0, 0, 0) == BAD


def test_the_rectangle_marshalling_clips_like_the_twin(tmp_path):
    """gs_params.h pick_select_of, built for the host: the clipped rectangle is the twin's for every corner around the target's edges and at the ends of int32"""
    import ctypes as C
    import itertools
    from harness import build_harness, run_under_sanitizers
    lib = C.CDLL(build_harness(tmp_path, "pick_host_harness.cpp"))
    W, H = 6, 4
    vals = (-2 ** 31, -1, 0, 1, W - 1, W, H - 1, H, 2 ** 31 - 1)
    out = (C.c_uint32 * 7)()
    for x0, y0, x1, y1 in itertools.product(vals, repeat=4):
        if x0 > x1 or y0 > y1:
            continue
        lib.ph_select_of(C.c_int32(x0), C.c_int32(y0), C.c_int32(x1), C.c_int32(y1), C.c_uint32(W), C.c_uint32(H), C.c_uint32(9), C.c_int32(3), out)
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
        want = [0, 0, 0, 0] if cx0 > cx1 or cy0 > cy1 else [cx0, cy0, cx1 - cx0 + 1, cy1 - cy0 + 1]
        assert list(out) == want + [W, 9, 1], (x0, y0, x1, y1, list(out))
    p = run_under_sanitizers(tmp_path, "pick_host_harness.cpp", "PICK_HARNESS_MAIN")
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout, p.stderr)
