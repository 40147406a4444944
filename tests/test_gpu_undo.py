"""Undo and redo of the edit state on the GPU (csrc/gs_edit.hip: hist_count / hist_gather / hist_swap through gs_renderer_edit_history_enable,
_checkpoint, _undo, _redo) in lock step with the numpy model of the history (tests/undo_model.py) composed over the edit, transform and rigid models.
Nothing here is arithmetic: every comparison is bit for bit."""
import numpy as np
import pytest

import edit_model as EM
import undo_model as UM
from common import RT_TOL, default_camera, rt_err, small_asset
from gpu_rig import BAD, draw_frame
from undo_rig import FULL, OPS, URig, selections
from unitygaussiansplatting_amd import _abi, _lib
from unitygaussiansplatting_amd.renderer import EditHistoryFlags, GaussianSplatRenderer, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
BIG = 262989                                                       # 1,028 blocks: the scan's loop runs twice, and the last block holds 77 splats


def entry_bound(n, k):
    return 8 * ((n + 31) // 32) + 224 * k + 4096                   # the issue's condition on an entry's size


def gesture(rig, name, words, k, op):
    """select, checkpoint, operation (against the model), undo (the state before), redo (the state after)"""
    what = f"{name} / {op}"
    rig.upload_selected(words)
    rig.set_rigid(op.startswith("rigid"))                          # the setting is the gesture's before its checkpoint: GS_HIST_TRANSFORM reads it
    rig.checkpoint(FULL)
    before = rig.model_state()
    info = rig.info()
    assert info["top_splats"] == k and info["top_bytes"] <= entry_bound(rig.m.n, k), (what, info)
    assert info["top_what"] == UM.SELECTION | UM.DELETED | UM.POS | UM.OTHER | (UM.SH if rig.m.rigid else 0)
    rig.operation(op)
    rig.check(what + ": the operation")
    after = rig.model_state()
    if k:
        assert not all(np.array_equal(a, b) for a, b in zip(before, after)), what
    rig.undo()
    rig.same(rig.state(), before, what + ": undo")
    rig.check(what + ": undo against the model")
    rig.redo()
    rig.same(rig.state(), after, what + ": redo")
    rig.check(what + ": redo against the model")


# ---- 1. every operation, at the seams of the kernels' shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 257, 1000])
def test_every_operation_is_undone_and_redone(gpu_ctx, n):
    rig = URig(gpu_ctx, small_asset(n, 5, "VeryHigh"), rigid=True)
    for name, words, k in selections(n):
        for op in OPS:
            gesture(rig, name, words, k, op)
            if name == "all, tail bits set":
                assert rig.info()["top_splats"] == n and EM.popcount(words) == 32 * rig.m.nw      # not 64 at N = 33
        rig.r.EditHistoryClear(); rig.h.clear()
        rig.asset_untouched(gpu_ctx)
    rig.close()


@pytest.mark.parametrize("op", OPS)
def test_a_large_asset(gpu_ctx, op):
    """more than 1,024 blocks and a partial last one; the 1 % entry is far below the three blobs it replaces"""
    rig = URig(gpu_ctx, small_asset(BIG, 5, "VeryHigh"), rigid=True)
    for name, words, k in selections(BIG):
        gesture(rig, name, words, k, op)
        if name == "a seeded 1 %":
            assert rig.info()["top_bytes"] <= entry_bound(BIG, k) < (12 + 16 + 192) * BIG // 20
        rig.r.EditHistoryClear(); rig.h.clear()
    rig.asset_untouched(gpu_ctx)
    rig.close()


# ---- 2. gates ---------------------------------------------------------------------------------------------------------------------------------
def test_a_medium_asset_journals_bits_only(gpu_ctx):
    rig = URig(gpu_ctx, small_asset(300, 5, "Medium"), rigid=True)
    assert not rig.m.pos_gate and not rig.m.rot_gate
    rig.select_all()
    rig.checkpoint(UM.TRANSFORM)
    rig.checkpoint(UM.POS | UM.OTHER | UM.SH)
    assert rig.info()["undo_depth"] == 0                           # nothing is left of the flags: nothing is pushed
    rig.checkpoint(FULL)
    assert rig.info()["top_what"] == UM.SELECTION | UM.DELETED and rig.info()["top_splats"] == 0
    before = rig.model_state()
    rig.delete()
    rig.check("delete")
    rig.undo()
    rig.same(rig.state(), before, "undo of a delete on a Medium asset")
    rig.redo()
    rig.check("redo")
    rig.close()


def test_a_blob_without_a_private_copy_is_skipped(gpu_ctx):
    a = small_asset(300, 5, "VeryHigh")
    rig = URig(gpu_ctx, a, rigid=True)
    rig.upload_selected(selections(300)[4][1])
    rig.checkpoint(UM.TRANSFORM)
    held = rig.info()["bytes"]
    rig.undo()                                                     # nothing was written since: no blob is private, nothing is swapped, nothing is allocated
    pos, other = rig.r.DownloadPosOther()
    assert np.array_equal(pos, np.asarray(a.posData, np.uint8)) and np.array_equal(other, np.asarray(a.otherData, np.uint8))
    assert rig.info()["bytes"] == held and rig.info()["redo_depth"] == 1
    rig.redo()
    rig.check("undo and redo of an untouched checkpoint")
    rig.store3(); rig.translate()                                  # now pos is private; other and sh are still the asset's
    rig.check("translate")
    rig.undo()
    rig.check("undo with only the position blob private")
    pos, other = rig.r.DownloadPosOther()
    assert np.array_equal(pos, np.asarray(a.posData, np.uint8)) and np.array_equal(other, np.asarray(a.otherData, np.uint8))
    rig.asset_untouched(gpu_ctx)
    rig.close()


# ---- 3. the budget ------------------------------------------------------------------------------------------------------------------------------
def test_budget_eviction_and_an_entry_over_the_budget(gpu_ctx):
    n = 1000
    flags = np.zeros(n, bool)
    flags[::3] = True
    words, k = EM.pack_bits(flags, (n + 31) // 32), int(flags.sum())
    one = UM.entry_bytes(UM.SELECTION | UM.DELETED | UM.RECORDS, (n + 31) // 32, k)
    assert 2 * one + one // 2 < UM.entry_bytes(UM.SELECTION | UM.DELETED | UM.RECORDS, (n + 31) // 32, n)
    rig = URig(gpu_ctx, small_asset(n, 5, "VeryHigh"), max_bytes=2 * one + one // 2, rigid=True)
    rig.upload_selected(words)
    rig.store3()
    states = []
    for step in range(3):
        rig.checkpoint(FULL)
        states.append(rig.model_state())
        rig.translate((0.125 * (step + 1), 0.0, -0.25))
    info = rig.info()
    assert (info["undo_depth"], info["evicted"]) == (2, 1) and info["bytes"] == 2 * one <= info["max_bytes"]
    rig.check("three checkpoints in a budget of two")
    rig.undo(); rig.undo(); rig.undo()                             # the third does nothing: the oldest entry is gone
    rig.same(rig.state(), states[1], "the oldest surviving checkpoint")
    rig.check("the whole stack undone")
    rig.redo(); rig.redo()
    # an entry that alone exceeds the budget: refused, state and stack unchanged
    rig.select_all()
    before, info = rig.state(), rig.info()
    rig.checkpoint(FULL, want=UM.OOM)
    assert rig.lib.gs_renderer_edit_checkpoint(rig.r._r_h, FULL) == _abi.GS_ERR_OUT_OF_MEMORY
    rig.same(rig.state(), before, "a refused checkpoint")
    assert rig.info() == info
    rig.check("after the refusal")
    rig.close()


# ---- 4. invalidation and refusals -------------------------------------------------------------------------------------------------------------------
def test_every_mutating_call_drops_redo(gpu_ctx):
    rig = URig(gpu_ctx, small_asset(300, 5, "VeryHigh"), rigid=True)
    words = selections(300)[4][1]
    cam = default_camera()
    calls = {"select all": rig.select_all, "deselect all": rig.deselect_all, "invert": rig.invert, "delete": rig.delete, "translate": rig.translate,
             "rotate": rig.rotate, "scale": rig.scale, "upload selected": lambda: rig.upload_selected(words),
             "set deleted bits": lambda: rig.set_deleted_bits(words), "no deleted bits": lambda: rig.set_deleted_bits(None)}

    def update():
        rig.r.EditUpdateSelection((80.25, 150.0), (200.75, 50.5), cam, False)
        rig.h.mutated(True); rig.m.update_selection(rig.r.FrameParams(cam), EM.PREMISE_RECT, False)
    calls["update selection"] = update
    for name, fn in calls.items():
        rig.upload_selected(words)
        rig.store3()
        rig.checkpoint(FULL)
        rig.translate()
        rig.undo()
        assert rig.info()["redo_depth"] == 1, name
        fn()
        assert rig.info()["redo_depth"] == 0, name
        rig.check(name)
        rig.redo()                                                 # nothing to redo: nothing happens
        rig.check(name + ", redo of nothing")
    rig.close()


def test_a_resize_and_a_copy_clear_the_history(gpu_ctx):
    a = small_asset(300, 5, "VeryHigh")
    rig = URig(gpu_ctx, a, rigid=True)
    src = URig(gpu_ctx, small_asset(257, 6, "VeryHigh"), max_bytes=0)
    rig.select_all(); rig.store3()
    rig.checkpoint(FULL); rig.translate(); rig.checkpoint(FULL); rig.undo()
    assert (rig.info()["undo_depth"], rig.info()["redo_depth"]) == (1, 1)
    src.r.EditCopySplatsInto(rig.r, 0, 10, 50)
    info = rig.info()
    assert (info["enabled"], info["undo_depth"], info["redo_depth"], info["bytes"]) == (1, 0, 0, 0)
    rig.r.EditCheckpoint(FULL)
    assert rig.info()["undo_depth"] == 1
    rig.r.EditSetSplatCount(310)
    info = rig.info()
    assert (info["enabled"], info["undo_depth"], info["redo_depth"], info["bytes"], info["max_bytes"]) == (1, 0, 0, 0, 1 << 30)
    rig.r.EditSelectAll()
    with rig.r.EditGesture(EditHistoryFlags.Selection | EditHistoryFlags.Transform) as r:     # the history works at the new count
        before = r.DownloadSplatData()
        r.EditTranslateSelection((0.5, 0.0, 0.0))
    assert rig.info()["top_splats"] == 310 and not np.array_equal(rig.r.DownloadSplatData()[0], before[0])
    rig.r.EditUndo()
    assert all(np.array_equal(g, w) for g, w in zip(rig.r.DownloadSplatData(), before))
    src.close(); rig.close()


def test_release_keeps_the_history_and_undo_makes_the_buffers_again(gpu_ctx):
    rig = URig(gpu_ctx, small_asset(257, 5, "VeryHigh"), rigid=True)
    name, words, k = selections(257)[4]
    rig.upload_selected(words)
    rig.store3()
    rig.checkpoint(FULL)
    before = rig.model_state()
    rig.rotate()
    rig.delete()
    rig.set_deleted_bits(None)                                     # the deleted buffer goes too
    rig.release()
    assert rig.info()["undo_depth"] == 1
    rig.check("released")
    rig.undo()
    got = rig.state()
    for j in (0, 1, 2, 3, 4, 6):                                   # everything but the mouse-down selection, which the history leaves alone
        assert np.array_equal(got[j], before[j]), j
    rig.check("undo after a release")
    assert rig.r.EditHistoryInfo().redo_depth == 1
    rig.close()


def test_refusals(gpu_ctx):
    rig = URig(gpu_ctx, small_asset(33, 5, "VeryHigh"), max_bytes=0)
    h, lib = rig.r._r_h, rig.lib
    assert rig.info()["enabled"] == 0
    for fn in (lib.gs_renderer_edit_undo, lib.gs_renderer_edit_redo):
        assert fn(h) == BAD
    assert lib.gs_renderer_edit_checkpoint(h, FULL) == BAD and b"off" in lib.gs_last_error_string()
    assert lib.gs_renderer_edit_history_clear(h) == 0 and lib.gs_renderer_edit_history_info(h, None) == BAD
    rig.select_all(); rig.translate()                              # the hooks do nothing while the history is off
    assert rig.info() == UM.History(rig.m).info()
    rig.r.EditHistoryEnable(1 << 20); rig.h.enable(1 << 20)
    for what in (0, 32, 64, FULL | 0x100, 0x40000000):
        assert lib.gs_renderer_edit_checkpoint(h, what) == BAD
    rig.check("refused checkpoints change nothing")
    rig.checkpoint(FULL)
    rig.r.EditHistoryEnable(0); rig.h.enable(0)
    assert rig.info() == rig.h.info() and rig.info()["bytes"] == 0
    rig.close()


# ---- 5. frames --------------------------------------------------------------------------------------------------------------------------------------
def _frame(r, cam, rt):
    r.ResetOrder()                                                 # the order's tie-breaking depends on the sort history
    draw_frame(r, cam, rt)
    return r.DownloadOrder(), r.DownloadView(), rt.Download()


@pytest.mark.parametrize("op", ["translate", "rigid rotate", "delete"])
def test_frames_after_an_undo_are_those_of_a_fresh_renderer(gpu_ctx, op):
    a = small_asset(1000, 5, "VeryHigh")
    cam = default_camera()
    rt = RenderTarget(gpu_ctx, 320, 200)
    highlight = op == "delete"

    def fresh():
        r = GaussianSplatRenderer(gpu_ctx, a)
        r.CreateResourcesForAsset()
        if highlight:
            r.SetSelectionHighlight(True)
            r.UploadSelectedBits(words)
        out = _frame(r, cam, rt)
        r.DisposeResourcesForAsset()
        return out

    rig = URig(gpu_ctx, a, rigid=True)
    words = selections(1000)[4][1]
    if highlight:
        rig.r.SetSelectionHighlight(True)
    rig.upload_selected(words)
    first = _frame(rig.r, cam, rt)
    rig.checkpoint(FULL)
    rig.operation(op)
    moved = _frame(rig.r, cam, rt)
    assert not np.array_equal(moved[2], first[2])
    rig.undo()
    again = _frame(rig.r, cam, rt)
    want = fresh()
    for g, w, f in zip(again, want, first):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)) and np.array_equal(g.view(np.uint8), f.view(np.uint8))
    rig.redo()
    redone = _frame(rig.r, cam, rt)
    assert all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(redone, moved))
    rt.Dispose(); rig.close()


@pytest.mark.parametrize("op", ["translate", "delete"])
def test_undo_between_frames_in_flight(gpu_ctx, op):
    """GS_SORT_VISIBLE, two frames in flight, frames dealt alternately, the raw asynchronous calls between them: every frame equals the
    one-at-a-time renderer's, a frame dealt before the undo keeps the state of its time"""
    a = small_asset(1000, 5, "VeryHigh")
    words = selections(1000)[4][1]
    cams = [default_camera(az=10.0), default_camera(az=20.0), default_camera(az=20.0), default_camera(az=20.0), default_camera(az=35.0), default_camera(az=50.0)]

    def run(frames):
        rig = URig(gpu_ctx, a, rigid=True, sort_mode=SortMode.Visible, frames=frames)
        r = rig.r
        if frames > 1:
            assert r.FramesInFlight() == (frames, True)
        rig.upload_selected(words)
        rig.store3()
        rts = [RenderTarget(gpu_ctx, 320, 200) for _ in cams]
        for k, cam in enumerate(cams):
            r.SortPoints(cam); r.CalcViewData(cam); rts[k].Clear(); r.Draw(cam, rts[k])
            if k == 1:
                rig.checkpoint(FULL)
                rig.operation(op)
            if k == 2:
                rig.undo()
                if op == "translate" and frames == 1:
                    with pytest.raises(_lib.GsError) as err:       # as after a transform: the view buffer is that of the old positions
                        r.DownloadView()
                    assert err.value.code == BAD and "calc_view has not run since the splats were moved" in str(err.value)
            if k == 4:
                rig.redo()
        out = [t.Download() for t in rts]
        rig.check("at the end")
        for t in rts:
            t.Dispose()
        rig.close()
        return out

    want = run(1)
    got = run(2)
    for k in range(len(cams)):
        assert np.array_equal(got[k], want[k]), f"frame {k}"
    assert not np.array_equal(want[2], want[1])                    # frame 1 shows the state before the edit, frame 2 (the same camera) the edited one
    # ... and frame 3, dealt after the undo, the state before it again (a delete moves nothing: the same bits; a move and its undo leave the order's
    # ties to a different sort history, so that frame is held to the parity bar instead)
    assert not np.array_equal(want[3], want[2])
    if op == "delete":
        assert np.array_equal(want[3], want[1])
    else:
        assert rt_err(want[3], want[1]) <= RT_TOL
