"""The lock-step rig of the edit-history suites (helper, not a test): one renderer with its history on, the rigid model of its edit state
(tests/rigid_model.py) and the model of the history over it (tests/undo_model.py), moved together.  Every call goes to both sides with the hook
the library's call has; check() compares everything a host can read -- the four blobs, the three bit buffers, the history's info -- bit for bit.
Imports without a GPU; nothing here makes a context."""
import numpy as np

import edit_model as EM
import rigid_model as RM
import transform_model as TM
import undo_model as UM
from builders import TOOL
from gpu_rig import fptr
from unitygaussiansplatting_amd import _lib
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, SortMode

CENTRE = (0.3, -0.2, 0.1)
Q1 = (0.18257419, 0.36514837, 0.54772256, 0.73029674)
FULL = UM.SELECTION | UM.DELETED | UM.TRANSFORM
OPS = ("delete", "translate", "rotate", "scale", "rigid rotate", "rigid scale")


def selections(n: int):
    """the selections at the seams of the kernels' shape: (name, words, splats journalled)"""
    nw = (n + 31) // 32
    tail = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF) if n % 32 else np.uint32(0)

    def of(idx):
        flags = np.zeros(n, bool)
        flags[np.asarray(idx, np.int64)] = True
        return EM.pack_bits(flags, nw)
    every = ~np.zeros(nw, np.uint32)                               # what select-all leaves without cutouts: the tail bits set
    wave = np.arange(64 * ((n // 64) // 2), min(n, 64 * ((n // 64) // 2) + 64))         # exactly one wave's two words (all of a 33-splat asset's)
    out = [("empty", np.zeros(nw, np.uint32), 0), ("splat 0", of([0]), 1), ("the last splat", of([n - 1]), 1), ("all, tail bits set", every, n),
           ("every other splat", of(np.arange(0, n, 2)), (n + 1) // 2), ("one wave's two words", of(wave), len(wave))]
    one = np.flatnonzero(np.random.default_rng(n).random(n) < 0.01)
    words = of(one)
    words[-1] |= tail                                              # ... and a seeded 1 % with the tail bits set as well
    out.append(("a seeded 1 %", words, len(one)))
    return out


class URig:
    def __init__(self, ctx, asset, max_bytes=1 << 30, rigid=False, sort_mode=SortMode.Full, frames=1, transform=None):
        """ctx None: the models alone (a dry run of a session's plan on a box without a GPU)"""
        self.r = r = GaussianSplatRenderer(ctx, asset, transform) if ctx is not None else None
        if r is not None:
            r.sortMode, r.framesInFlight, r.rigidTransforms = sort_mode, frames, rigid
            r.CreateResourcesForAsset()
        self.lib = _lib.lib()
        self.m = RM.RigidModel(asset, rigid)
        self.h = UM.History(self.m)
        self.color0 = np.ascontiguousarray(asset.colorData, np.uint8).copy()
        self.asset_blobs = [np.ascontiguousarray(b, np.uint8).copy() for b in (asset.posData, asset.otherData, asset.colorData, asset.shData)]
        if max_bytes:
            if r is not None:
                r.EditHistoryEnable(max_bytes)
            self.h.enable(max_bytes)

    def close(self):
        if self.r is not None:
            self.r.DisposeResourcesForAsset()

    # -- what can be read back ------------------------------------------------------------------------------------------------------------------
    def info(self) -> dict:
        return UM.info_dict(self.r.EditHistoryInfo()) if self.r is not None else self.h.info()

    def state(self):
        """(pos, other, color, sh, selected, mouse-down, deleted) of the renderer"""
        return tuple(self.r.DownloadSplatData()) + tuple(self.r.DownloadEditBits())

    def model_state(self):
        return (self.m.pos_blob.copy(), self.m.other_blob.copy(), self.color0, self.m.sh_blob.copy()) + tuple(b.copy() for b in self.m.bits())

    @staticmethod
    def same(got, want, what):
        for name, g, w, floats in zip(("pos", "other", "color", "sh", "selected", "mouse-down", "deleted"), got, want, (True, False, False, True, False, False, False)):
            assert TM.blobs_equal(g.view(np.uint8), w.view(np.uint8), floats=floats), f"{what}: {name} differs at {np.flatnonzero(g.view(np.uint8) != w.view(np.uint8))[:8]}"

    def check(self, what, blobs=True):
        if self.r is None:
            return
        if blobs:
            self.same(self.state(), self.model_state(), what)
        else:
            self.same((self.color0,) * 4 + tuple(self.r.DownloadEditBits()), (self.color0,) * 4 + self.m.bits(), what)
        assert self.info() == self.h.info(), (what, self.info(), self.h.info())

    # -- the calls, on both sides: raw C calls, so that nothing waits between them ----------------------------------------------------------------
    def call(self, name, *args):
        if self.r is None:
            return
        _lib.check(getattr(self.lib, name)(self.r._r_h, *args), name)
        self.r.m_GpuEditSelected = True                            # (what DisposeResourcesForAsset goes by)

    def upload_selected(self, words):
        w = np.ascontiguousarray(words, np.uint32)
        self.call("gs_renderer_edit_upload_selected_bits", w.ctypes.data, len(w))
        self.h.mutated(True); self.m.upload_selected(w)

    def select_all(self):
        self.call("gs_renderer_edit_select_all"); self.h.mutated(True); self.m.select_all()

    def deselect_all(self):
        self.call("gs_renderer_edit_deselect_all"); self.h.mutated(True); self.m.deselect_all()

    def invert(self):
        self.call("gs_renderer_edit_invert_selection"); self.h.mutated(True); self.m.invert_selection()

    def delete(self):
        self.call("gs_renderer_edit_delete_selected"); self.h.mutated(True); self.m.delete_selected()

    def set_deleted_bits(self, words):
        if self.r is not None:
            self.r.SetDeletedBits(words)
        self.h.mutated(False); self.m.set_deleted_bits(words)

    def store3(self):
        for name in ("pos", "other", "sh"):
            self.call(f"gs_renderer_edit_store_{name}_mouse_down")
        if self.r is not None:
            self.r.m_GpuEditPosMouseDown = self.r.m_GpuEditOtherMouseDown = self.r.m_GpuEditSHMouseDown = True
        self.m.store_pos(); self.m.store_other(); self.m.store_sh()

    def set_rigid(self, on):
        if self.r is not None:
            self.r.EditSetRigidTransforms(on)
        self.m.set_rigid(on)

    def translate(self, delta=(0.25, -0.5, 0.125)):
        self.call("gs_renderer_edit_translate_selection", fptr(delta)[1])
        self.h.transform(); assert self.m.translate(delta)

    def rotate(self, q=Q1, tr=TOOL, centre=CENTRE):
        (_, c), (_, a), (_, b), (_, v) = fptr(centre), fptr(tr.localToWorldMatrix), fptr(tr.worldToLocalMatrix), fptr(q)
        self.call("gs_renderer_edit_rotate_selection", c, a, b, v)
        self.h.transform(); assert self.m.rotate(centre, tr.localToWorldMatrix, tr.worldToLocalMatrix, q)

    def scale(self, s=(1.5, -0.5, 0.25), tr=TOOL, centre=CENTRE):
        (_, c), (_, a), (_, b), (_, v) = fptr(centre), fptr(tr.localToWorldMatrix), fptr(tr.worldToLocalMatrix), fptr(s)
        self.call("gs_renderer_edit_scale_selection", c, a, b, v)
        self.h.transform(); assert self.m.scale(centre, tr.localToWorldMatrix, tr.worldToLocalMatrix, s)

    def operation(self, op):
        """one of OPS, with the mouse-down copies it reads stored first (the model's transforms are the reference's or the rigid ones by the setting)"""
        if op == "delete":
            return self.delete()
        self.set_rigid(op.startswith("rigid"))
        self.store3()
        {"translate": self.translate, "rotate": self.rotate, "scale": self.scale, "rigid rotate": self.rotate,
         "rigid scale": lambda: self.scale((1.25, 1.25, 1.25))}[op]()

    def checkpoint(self, what=FULL, want=UM.OK):
        """want None: whatever the model says (GS_OK, or GS_ERR_OUT_OF_MEMORY for an entry over the budget)"""
        code = self.h.checkpoint(what)
        assert want is None or code == want, (code, want)
        if self.r is not None:
            rc = self.lib.gs_renderer_edit_checkpoint(self.r._r_h, what)
            assert rc == code, (rc, code, self.lib.gs_last_error_string())
            self.r.m_GpuEditSelected = True
        return code

    def undo(self):
        self.call("gs_renderer_edit_undo"); assert self.h.undo() == UM.OK

    def redo(self):
        self.call("gs_renderer_edit_redo"); assert self.h.redo() == UM.OK

    def release(self):
        _lib.check(self.lib.gs_renderer_edit_release(self.r._r_h), "gs_renderer_edit_release")
        self.r.m_GpuEditSelected = self.r.m_GpuEditPosMouseDown = self.r.m_GpuEditOtherMouseDown = self.r.m_GpuEditSHMouseDown = False
        self.m.release()

    def asset_untouched(self, ctx):
        """another renderer over the same device asset still reads the asset's own bytes"""
        other = GaussianSplatRenderer(ctx, self.r.m_Asset)
        other.ShareResourcesOf(self.r)
        try:
            for g, w in zip(other.DownloadSplatData(), self.asset_blobs):
                assert np.array_equal(g, w), "the asset's own blobs were written"
        finally:
            other.DisposeResourcesForAsset()
