"""The selection highlight (RenderGaussianSplats.shader:63-73,87-101) on the CPU: the host build of the kernels' selected fragment against the reference's
own frag(), the model of a highlighted frame (tests/highlight_model.py) against the reference's own vert + frag, the host build of calc_view's records
against the oracle's opacity-1 records, and the public surface.  The GPU is held to the model in tests/test_gpu_highlight.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import highlight_model as HM
import oracle_lib as O
import ref_lib as R
from common import RT_TOL, default_camera, rt_diff, small_asset
from unitygaussiansplatting_amd import _abi, _lib, camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = {1: 1.0 / 255.0, 7: 7.0 / 255.0, 10: 10.0 / 255.0}
TBITS = {1: 0x3B808081, 7: 0x3CE0E0E1, 10: 0x3D20A0A1}       # the fp32 quotients 1.0f / 255.0f ... as the shader's literals fold


@pytest.fixture(scope="module")
def hl(tmp_path_factory):
    return HM.build(tmp_path_factory.mktemp("hl"))


def ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _native_e_bits(q):
    """bits of e = exp2(fl(power log2 e)) for an array of fp32 q (numpy twin of hl_native_e: only used to PICK fragments)"""
    q = q.astype(np.float32)
    power = -(q[:, 1].astype(np.float64) * q[:, 1].astype(np.float64) + (q[:, 0] * q[:, 0]).astype(np.float64)).astype(np.float32)
    y = power * np.float32(1.44269504088896340736)
    return np.exp2(y.astype(np.float64)).astype(np.float32).view(np.uint32)


def fragments():
    """>= 20,000 fragments: a third spread over the quad, the rest with e within +-3e-7 (relative) of 1/255, 7/255 and 10/255 -- and, found by search, fragments
    whose native e is the fp32 value 7/255 or 10/255 itself or one of its closest reachable neighbours on either side"""
    rng = np.random.default_rng(21)
    n = 21000
    q = rng.uniform(-2.2, 2.2, (n, 2))
    k = n // 9
    for j, t in enumerate((1, 7, 10)):
        for half in range(2):                                    # two ninths per threshold
            sl = slice(n // 3 + (2 * j + half) * k, n // 3 + (2 * j + half + 1) * k)
            r = np.sqrt(-np.log(T[t] * (1.0 + rng.uniform(-3e-7, 3e-7, k))))
            th = rng.uniform(0, 2 * np.pi, k)
            q[sl] = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    q = q.astype(np.float32)
    extra = []
    for t in (7, 10):
        r0 = np.sqrt(-np.log(T[t]))
        th = rng.uniform(0, 2 * np.pi, 400000)
        rr = r0 * (1.0 + rng.uniform(-2e-7, 2e-7, 400000))
        c = np.stack([rr * np.cos(th), rr * np.sin(th)], axis=1).astype(np.float32)
        d = _native_e_bits(c).astype(np.int64) - TBITS[t]
        for want in sorted(set(d[np.abs(d) <= 4])):
            extra.append(c[np.flatnonzero(d == want)[:3]])
    q = np.concatenate([q] + extra)
    col = rng.uniform(0, 1.5, (len(q), 3)).astype(np.float32)
    return q, col


def test_fragment_picks_reach_the_thresholds(hl):
    """the premise of the fragment tests: the set holds fragments whose native e is AT the fp32 thresholds 7/255 and 10/255 or their closest reachable
    neighbours on both sides (y = fl(power log2 e) moves e in steps of 3-4 ulps, so not every float is an e), and thousands within 3e-7 of each threshold"""
    q, _ = fragments()
    y = C.c_float()
    e = np.array([hl.hl_native_e(q[i].ctypes.data_as(C.c_void_p), C.byref(y)) for i in range(len(q))], np.float32)
    bits = e.view(np.uint32).astype(np.int64)
    for t in (7, 10):
        d = bits - TBITS[t]
        assert ((d >= -4) & (d < 0)).any() and ((d >= 0) & (d <= 4)).any(), (t, sorted(set(d[np.abs(d) <= 4])))
        print(f"native e - fl({t}/255) in ulps, reached: {sorted(set(d[np.abs(d) <= 4]))}")
    for t in (1, 7, 10):
        assert (np.abs(e.astype(np.float64) / T[t] - 1.0) <= 1e-6).sum() >= 2000


@pytest.mark.parametrize("which", ["strict", "fused"])
def test_selected_fragment_is_the_references(hl, which):
    """frag() with col.a = -1 (what vert() hands it for a selected splat) vs the host build of gsm::SelectedFragment.  fused: the same discard and bit-equal
    rgba un-windowed -- which pins the literal folding and lerp as the shader text evaluates them; windowed (as the kernel and the model evaluate it) it may
    differ only where e is within 1.5e-6 of one of the three thresholds (8 ulps <= 2^-20 relative, plus Exp2Det's < 1 ulp).  strict (correctly rounded e^x):
    within 16 ulps, decisions differing only within 2e-6 of a threshold.

    What the windows are for is then shown with the native e moved by one ulp either way, which is what a GPU's exp2 unit may return: windowed, all three
    natives give the same decisions everywhere and the same bits inside a window; un-windowed, some fragment jumps across the ring (moved > 0).
    With the canon's own correctly rounded exp2 nothing moves: the three windows hold 15 values of y = fl(power log2 e) in all (y steps e by 3-4 ulps), and
    Exp2Det returns the correctly rounded result at every one of them (measured by enumeration), so on the host windowed == un-windowed for every fragment
    there is -- moved counts the one-ulp natives instead, which is the case the window exists for."""
    q, col = fragments()
    n = len(q)
    assert n >= 20000
    e64 = np.exp(-(q.astype(np.float64) ** 2).sum(axis=1))
    near = lambda i, tol: min(abs(e64[i] / T[t] - 1.0) for t in T) <= tol
    band = lambda d, o: -1 if d else (2 if o[3] == 1.0 and o[0] == 1.0 and o[1] == 0.0 else (1 if o[3] < 0.3 else 3))      # discarded / low / ring / above
    moved = flips = worst = inside = 0
    for i in range(n):
        dr, out_r = R.fragment(which, q[i], np.append(col[i], np.float32(-1.0)))
        dh, out_h = HM.fragment(hl, q[i], col[i], False)
        if which == "fused":
            assert dh == dr and np.array_equal(out_h.view(np.uint32), out_r.view(np.uint32)), (i, q[i], col[i], out_h, out_r)
            dw, out_w = HM.fragment(hl, q[i], col[i], True)
            if dw != dh or not np.array_equal(out_w.view(np.uint32), out_h.view(np.uint32)):
                assert near(i, 1.5e-6), (i, e64[i])
            if not near(i, 3e-6):
                continue
            e, y = HM.native_e(hl, q[i])
            for step in (-1, 1):
                e1 = (e.view(np.uint32) + np.uint32(step)).view(np.float32) if step > 0 else (e.view(np.uint32) - np.uint32(1)).view(np.float32)
                d1, o1 = HM.fragment_from(hl, e1, y, col[i], True)
                assert band(d1, o1) == band(dw, out_w), (i, e, e1, o1, out_w)                    # windowed: one ulp of the native changes no decision
                in_win = min(abs(int(e.view(np.uint32)) - TBITS[t]) for t in TBITS) <= 6        # both natives inside a window: the same bits
                if in_win:
                    inside += 1
                    assert d1 == dw and np.array_equal(o1.view(np.uint32), out_w.view(np.uint32)), (i, e, e1, o1, out_w)
                else:
                    assert d1 or ulps(o1[3:], out_w[3:]).max() <= 1
                d0, o0 = HM.fragment_from(hl, e1, y, col[i], False)
                if band(d0, o0) != band(dh, out_h):
                    moved += 1
                    assert near(i, 1.5e-6), (i, e64[i])
        else:
            jump = dh != dr or (not dh and ulps(out_h, out_r).max() > 16)
            if jump:
                flips += 1
                assert near(i, 2e-6), (i, e64[i], out_h, out_r)
            elif not dh:
                worst = max(worst, int(ulps(out_h, out_r).max()))
    if which == "fused":
        print(f"fused: {inside} one-ulp natives inside a window, {moved} of them change a decision un-windowed, none windowed")
        assert moved > 0 and inside > 1000
    else:
        print(f"strict: worst {worst} ulps, {flips} decisions differ, each within 2e-6 of a threshold")
        assert worst <= 16


def test_known_fragments(hl):
    """the issue's example and the three bands: q = (1.8, 0) lies on the ring and returns (1, 0, 1, 1)"""
    for which in ("fused", "strict"):
        d, out = R.fragment(which, [1.8, 0.0], [0.2, 0.5, 0.7, -1.0])
        assert d == 0 and list(out) == [1.0, 0.0, 1.0, 1.0]
    d, out = HM.fragment(hl, [1.8, 0.0], [0.2, 0.5, 0.7], True)
    assert d == 0 and list(out) == [1.0, 0.0, 1.0, 1.0]
    d, out = HM.fragment(hl, [0.0, 0.0], [0.2, 0.5, 0.7], True)                # centre: alpha = saturate(1 + 0.3) = 1, the tint
    assert d == 0 and np.allclose(out, [0.6, 0.25, 0.85, 1.0], atol=1e-7)
    d, out = HM.fragment(hl, [2.0, 1.0], [0.2, 0.5, 0.7], True)                # e = exp(-5) = 1.7/255: the low band, alpha = e
    assert d == 0 and abs(out[3] - np.exp(-5.0)) < 1e-8 and abs(out[0] - 0.6 * np.exp(-5.0)) < 1e-8
    d, out = HM.fragment(hl, [2.0, 1.3], [0.2, 0.5, 0.7], True)                # e = exp(-5.69) < 1/255: discarded
    assert d == 1


def _scene():
    a = small_asset(3000, 5, "Medium")
    cam = default_camera(W=160, H=100, az=25.0)
    tr = camera.Transform()
    sel = np.zeros(a.splatCount, bool)
    sel[::3] = True
    return a, cam, tr, sel


@pytest.fixture(scope="module")
def ref_frames():
    """the reference's own frames of the scene, computed once: unselected, and with every third splat selected (vert() handing frag() col.a = -1)"""
    a, cam, tr, sel = _scene()
    P = camera.frame_params(cam, tr)
    ref = R.Ref(a, "fused")
    ref.set_indices()
    keys = ref.calc_distances(camera.sort_matrix(cam, tr.localToWorldMatrix))
    _, ref.order = O.sort_pairs(keys, ref.order)
    ref.calc_view(R.flipped(P))
    W, H = cam.pixelWidth, cam.pixelHeight
    plain = ref.draw(W, H, P.near_clip, P.far_clip)[::-1].copy()
    front = sel & (ref.view["pos"][:, 3] > 0)
    ref.view["color"][front, 1] = (ref.view["color"][front, 1] & np.uint32(0xFFFF0000)) | np.uint32(0xBC00)
    marked = ref.draw(W, H, P.near_clip, P.far_clip)[::-1].copy()
    return plain, marked


@pytest.mark.parametrize("mode", [0, 1])
def test_model_frame_is_the_references_frame(hl, ref_frames, mode):
    """small_asset(3000, 5, Medium) at 160x100, every third splat selected: the model's frame vs the frame of the reference's own vert + frag under D3D raster
    rules.  RT_TOL on every pixel that has no fragment within 1e-5 (relative, float64) of a decision -- e against the three thresholds, alpha against 1/255 for
    unselected splats, |q_k| against 2 -- and at most 0.1 % of the pixels may be excused so (measured: none)."""
    a, cam, tr, sel = _scene()
    plain, marked = ref_frames
    P = camera.frame_params(cam, tr)
    orc = O.Oracle(a)
    orc.sort(camera.sort_matrix(cam, tr.localToWorldMatrix))
    view = orc.calc_view(P).copy()
    f = HM.Frame(hl, view, P, HM.bits_of(sel), orc.order)
    rt = f.draw(mode, classify=True)
    W, H = cam.pixelWidth, cam.pixelHeight
    c = f.counts
    touched = np.zeros((H, W), bool)
    for s in np.flatnonzero(f.selected & f.visible):
        x0, y0, x1, y1 = f.rects[s, 0] & 0xFFFF, f.rects[s, 0] >> 16, f.rects[s, 1] & 0xFFFF, f.rects[s, 1] >> 16
        touched[y0:y1, x0:x1] = True
    faint = int((f.selected & f.visible & (view["color"][:, 1].astype(np.uint32) & 0xFFFF < 0x1C04)).sum())      # opacity half below 1/255
    print(f"mode {mode}: selected in front {int(f.selected.sum())}, drawn {int((f.selected & f.visible).sum())}, of opacity < 1/255: {faint}; fragments {c}; "
          f"pixels inside a selected splat's rectangle {touched.mean():.3f}")
    # premises
    assert f.selected.sum() == 1000 and c["ring"] >= 1000 and c["low"] >= 1000 and faint >= 1
    excused = f.excused.astype(bool)
    assert excused.sum() <= 0.001 * W * H
    e = rt_diff(rt, marked).max(axis=-1)
    print(f"mode {mode}: max error vs the reference's frame {e[~excused].max() / RT_TOL:.3f} x RT_TOL, excused pixels {int(excused.sum())}, band flips {c['band_flips']}")
    assert e[~excused].max() <= RT_TOL, (e.max() / RT_TOL, np.argwhere(e > RT_TOL)[:5])
    # the highlight is not a detail: the frame differs from the unselected one on a third of the pixels at least
    changed = (rt_diff(marked, plain).max(axis=-1) > RT_TOL).mean()
    assert changed > 0.30 and (rt_diff(rt, plain).max(axis=-1) > RT_TOL).mean() > 0.30, changed
    # ... and without a selection the model is the oracle's draw, bit for bit
    f0 = HM.Frame(hl, view, P, None, orc.order)
    assert np.array_equal(f0.draw(mode), orc.draw(P, mode))


def test_host_records_of_selected_splats_are_the_oracles_opacity_one_records(hl):
    """gsm::PrepareSplatHighlight / RecordColor1 compiled for the host: visibility, pixel rectangle and record of a selected splat equal the oracle's for the
    same splat at opacity 1 bit for bit (with the alpha half -1); those of an unselected splat equal today's."""
    a, cam, tr, sel = _scene()
    for az, W, H in ((25.0, 160, 100), (140.0, 333, 77)):
        cam = default_camera(W=W, H=H, az=az)
        P = camera.frame_params(cam, tr)
        orc = O.Oracle(a)
        view = orc.calc_view(P).copy()
        bits = HM.bits_of(sel)
        f = HM.Frame(hl, view, P, bits, orc.order)
        recs, rects, vis = HM.host_records(hl, view, P, bits)
        assert np.array_equal(vis, f.vis) and np.array_equal(rects, f.rects) and np.array_equal(recs, f.want_recs)
        m = f.selected & f.visible
        assert m.sum() > 300 and ((recs[m, 7] & 0xFFFF) == 0xBC00).all() and ((recs[~m, 7] & 0xFFFF) != 0xBC00).all()
        o_recs, o_rects, o_vis = orc.raster_records(P)                 # today's records
        u = ~f.selected
        assert np.array_equal(rects[u], o_rects[u]) and np.array_equal(recs[u], o_recs[u])
        ovis = np.unpackbits(o_vis.view(np.uint8), bitorder="little")[:orc.n].astype(bool)
        assert np.array_equal(f.visible[u], ovis[u])
        assert (f.visible[f.selected] >= ovis[f.selected]).all() and (f.visible & ~ovis).sum() >= 1      # a splat the opacity cull drops is drawn when selected
        grown = (rects[m] != o_rects[m]).any(axis=1).sum()
        assert grown > 100                                             # the opacity-1 footprint is larger than the splat's own
        r0, rects0, vis0 = HM.host_records(hl, view, P, None)          # no selected bits: exactly today's
        assert np.array_equal(r0, o_recs) and np.array_equal(rects0, o_rects) and np.array_equal(vis0, o_vis)


def test_half_rounding_of_the_model_is_the_oracles(hl):
    rng = np.random.default_rng(3)
    vals = np.concatenate([rng.uniform(-70000, 70000, 2000), rng.uniform(-1, 1, 4000), rng.uniform(-1e-4, 1e-4, 2000), 2.0 ** rng.uniform(-26, 17, 2000),
                           [0.0, 65504.0, 65519.99, 65520.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -14, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]])
    for v in vals:
        assert hl.hl_half_of(float(v)) == O.lib().gso_f64tof16(float(v)), v


# ---- the public surface (these fail on a library without the feature) ------------------------------------------------------------------
def test_surface_symbol_default_and_bindings():
    lib = _lib.lib()
    assert hasattr(lib, "gs_renderer_set_selection_highlight") and "gs_renderer_set_selection_highlight" in _lib.SIGNATURES
    assert lib.gs_renderer_set_selection_highlight(None, 1) == _abi.GS_ERR_INVALID_ARGUMENT
    assert lib.gs_abi_version() == 9                                   # an addition to ABI 9
    hdr = open(os.path.join(ROOT, "include", "gsplat_c.h")).read()
    assert re.search(r"int32_t\s+gs_renderer_set_selection_highlight\s*\(\s*gs_renderer\s*\*\s*r\s*,\s*int32_t\s+enabled\s*\)\s*;", hdr)
    cs = open(os.path.join(ROOT, "unitygaussiansplatting_amd", "dotnet", "GaussianSplatNative.cs")).read()
    assert re.search(r"extern\s+int\s+gs_renderer_set_selection_highlight\s*\(\s*IntPtr\s+\w+\s*,\s*int\s+\w+\s*\)", cs)


def test_python_wrapper_round_trips_and_defaults_to_off():
    from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer

    class NoContext:
        def _adopt(self, r):
            pass

    r = GaussianSplatRenderer(NoContext())
    assert r.selectionHighlight is False
    r.SetSelectionHighlight(True)                                     # no native renderer yet: kept, and applied when the resources are created
    assert r.selectionHighlight is True
    r.SetSelectionHighlight(0)
    assert r.selectionHighlight is False


def test_documents_no_longer_say_that_selection_cannot_be_seen():
    for rel in ("include/gsplat_c.h", "DESIGN.md", "INTEGRATION.md", "README.md", "unitygaussiansplatting_amd/csrc/gs_edit.hip", "unitygaussiansplatting_amd/renderer.py"):
        txt = open(os.path.join(ROOT, rel)).read()
        assert "NO VISUAL EFFECT" not in txt and "not highlighted" not in txt, rel
        assert "gs_renderer_set_selection_highlight" in txt or "SetSelectionHighlight" in txt, rel
