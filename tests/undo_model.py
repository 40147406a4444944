"""The yardstick of the edit history (helper, not a test): a numpy restatement of gs_renderer_edit_checkpoint / _undo / _redo and of the bookkeeping
around them (include/gsplat_c.h), written from the contract, over any model of the edit state that has the fields of
tests/rigid_model.RigidModel: sel / deleted (uint32 words, or None while the buffer does not exist), n, nw, pos_blob / other_blob / sh_blob (uint8,
whole records first), pos_gate / rot_gate, rigid, _ensure() and -- optionally -- _moved().  `State` below is the smallest such model.

An entry holds the two bit buffers whole and the records of the splats selected at its checkpoint (index < N, index order) with their index list; undo and
redo SWAP an entry with the current state.  What the library keeps to itself (which blobs are private, when dropped entries are released) has no effect on
anything a host can read, and is not modelled."""
from __future__ import annotations

import dataclasses

import numpy as np

SELECTION, DELETED, POS, OTHER, SH, TRANSFORM = 1, 2, 4, 8, 16, 0x80000000
RECORDS = POS | OTHER | SH
KNOWN = SELECTION | DELETED | RECORDS | TRANSFORM
STRIDE = {POS: 12, OTHER: 16, SH: 192}
BLOB = {POS: "pos_blob", OTHER: "other_blob", SH: "sh_blob"}
OK, BAD, OOM = 0, -1, -4


def selected_indices(words, n: int) -> np.ndarray:
    """the splats a checkpoint journals: the set bits at indices < n, ascending (the tail bits of the last word name no splat)"""
    if words is None:
        return np.zeros(0, np.uint32)
    bits = np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little")[:n]
    return np.flatnonzero(bits).astype(np.uint32)


def block_counts(words, n: int) -> np.ndarray:
    """selected splats with index < n per 256-splat block: what hist_count leaves for the scan"""
    idx = selected_indices(words, n)
    return np.bincount(idx >> 8, minlength=(n + 255) // 256).astype(np.uint32)


def gather(blob, idx, stride: int) -> np.ndarray:
    """the journal array of one kind: the records of idx, contiguous, as bytes"""
    rows = np.ascontiguousarray(blob, np.uint8)[:(int(idx.max()) + 1 if len(idx) else 0) * stride].reshape(-1, stride)
    return rows[idx].reshape(-1).copy()


def swap_records(blob, journal, idx, stride: int) -> None:
    """hist_swap: blob record idx[i] <-> journal record i, in place on both"""
    if len(idx) == 0:
        return
    top = (int(idx.max()) + 1) * stride
    rows, j = blob[:top].reshape(-1, stride), journal.reshape(-1, stride)
    tmp = rows[idx].copy()
    rows[idx] = j
    j[:] = tmp


def entry_bytes(what: int, words: int, k: int) -> int:
    """4 ceil(N/32) per bit buffer + k x (4 + 12 + 16 + 192) (less without a kind)"""
    per = 4 + sum(s for f, s in STRIDE.items() if what & f)
    return (4 * words if what & SELECTION else 0) + (4 * words if what & DELETED else 0) + (per * k if what & RECORDS else 0)


@dataclasses.dataclass
class Entry:
    what: int
    idx: np.ndarray
    sel_gen: int
    bytes: int
    sel: np.ndarray | None = None
    deleted: np.ndarray | None = None
    rec: dict = dataclasses.field(default_factory=dict)           # POS / OTHER / SH -> journal bytes


class State:
    """a VeryHigh renderer's journalable state and nothing else (tests/test_undo_model.py)"""

    def __init__(self, n: int, rng, pos_gate=True, rot_gate=True, rigid=True):
        self.n, self.nw = n, (n + 31) // 32
        self.pos_gate, self.rot_gate, self.rigid = pos_gate, rot_gate, rigid
        self.sel = self.md = self.deleted = None
        self.pos_blob = rng.integers(0, 256, 12 * n + 4, dtype=np.uint8)      # (the importer pads its blobs: more than whole records)
        self.other_blob = rng.integers(0, 256, 16 * n + 4, dtype=np.uint8)
        self.sh_blob = rng.integers(0, 256, 192 * n + 4, dtype=np.uint8)

    def _ensure(self) -> None:
        if self.sel is None:
            self.sel, self.md = np.zeros(self.nw, np.uint32), np.zeros(self.nw, np.uint32)

    def snapshot(self):
        z = np.zeros(self.nw, np.uint32)
        return tuple(a.copy() for a in (z if self.sel is None else self.sel, z if self.deleted is None else self.deleted, self.pos_blob, self.other_blob, self.sh_blob))


class History:
    def __init__(self, target):
        self.t = target
        self.enabled = False
        self.max_bytes = self.bytes = 0
        self.undo_stack: list[Entry] = []
        self.redo_stack: list[Entry] = []
        self.evicted = self.uncovered = 0
        self.sel_gen = 0

    # -- the switch -------------------------------------------------------------------------------------------------------------------------
    def enable(self, max_bytes: int) -> int:
        if max_bytes == 0:
            self.__init__(self.t)
            return OK
        if not self.enabled:
            self.enabled, self.evicted, self.uncovered, self.sel_gen, self.bytes = True, 0, 0, 0, 0
        self.max_bytes = max_bytes
        self._evict_for(0)
        while self.redo_stack and self.bytes > self.max_bytes:    # then the farthest redo entries
            self.bytes -= self.redo_stack.pop(0).bytes
            self.evicted += 1
        return OK

    def clear(self) -> int:
        self.undo_stack, self.redo_stack, self.bytes = [], [], 0
        return OK

    # -- the hooks of the calls that change journalable state ---------------------------------------------------------------------------------
    def _drop_redo(self) -> None:
        self.bytes -= sum(e.bytes for e in self.redo_stack)
        self.redo_stack = []

    def mutated(self, selection: bool) -> None:
        """every selection call, delete (selection = True) and the bit uploads (the deleted bits': selection = False)"""
        if not self.enabled:
            return
        self._drop_redo()
        if selection:
            self.sel_gen += 1

    def transform(self) -> None:
        """a translate / rotate / scale that passed its argument checks"""
        if not self.enabled:
            return
        self._drop_redo()
        top = self.undo_stack[-1] if self.undo_stack else None
        if top is None or not (top.what & RECORDS) or top.sel_gen != self.sel_gen:
            self.uncovered += 1

    def forget(self) -> None:
        """gs_renderer_edit_copy_splats_into on its destination: every entry goes"""
        if not self.enabled:
            return
        self.clear()
        self.sel_gen += 1

    def resized(self, target) -> None:
        """gs_renderer_edit_set_splat_count: the entries go with the old state; the switch, the budget and the counters stay"""
        self.t = target
        if self.enabled:
            self.clear()
            self.sel_gen += 1

    # -- checkpoint, undo, redo ------------------------------------------------------------------------------------------------------------------
    def resolve(self, what: int) -> int:
        t = self.t
        if what & TRANSFORM:
            what = (what & ~TRANSFORM) | POS | OTHER | (SH if t.rigid else 0)
        if not t.pos_gate:
            what &= ~POS
        if not t.rot_gate:
            what &= ~(OTHER | SH)
        return what

    def _evict_for(self, extra: int) -> None:
        while self.undo_stack and self.bytes + extra > self.max_bytes:
            self.bytes -= self.undo_stack.pop(0).bytes
            self.evicted += 1

    def checkpoint(self, what: int) -> int:
        t = self.t
        if not self.enabled or what == 0 or what & ~KNOWN:
            return BAD
        what = self.resolve(what)
        if not what:
            return OK
        if what & (SELECTION | RECORDS):
            t._ensure()
        idx = selected_indices(t.sel, t.n) if what & RECORDS else np.zeros(0, np.uint32)
        size = entry_bytes(what, t.nw, len(idx))
        if size > self.max_bytes:
            return OOM
        e = Entry(what, idx, self.sel_gen, size)
        if what & SELECTION:
            e.sel = t.sel.copy()
        if what & DELETED:
            e.deleted = np.zeros(t.nw, np.uint32) if t.deleted is None else t.deleted.copy()
        for flag, stride in STRIDE.items():
            if what & flag:
                e.rec[flag] = gather(getattr(t, BLOB[flag]), idx, stride)
        self._drop_redo()
        self._evict_for(size)
        self.bytes += size
        self.undo_stack.append(e)
        return OK

    def _apply(self, src: list, dst: list) -> int:
        if not self.enabled:
            return BAD
        if not src:
            return OK
        t, e = self.t, src.pop()
        moved = False
        for flag, stride in STRIDE.items():
            if e.what & flag and len(e.idx):
                swap_records(getattr(t, BLOB[flag]), e.rec[flag], e.idx, stride)
                moved = True
        if moved and hasattr(t, "_moved"):
            t._moved()
        if e.what & DELETED:
            cur = np.zeros(t.nw, np.uint32) if t.deleted is None else t.deleted
            t.deleted, e.deleted = e.deleted, cur.copy()
        if e.what & SELECTION:
            t._ensure()
            t.sel, e.sel = e.sel, t.sel.copy()
            self.sel_gen += 1
        dst.append(e)
        return OK

    def undo(self) -> int:
        return self._apply(self.undo_stack, self.redo_stack)

    def redo(self) -> int:
        return self._apply(self.redo_stack, self.undo_stack)

    def info(self) -> dict:
        top = self.undo_stack[-1] if self.undo_stack else None
        return dict(enabled=int(self.enabled), undo_depth=len(self.undo_stack), redo_depth=len(self.redo_stack), top_what=top.what if top else 0,
                    bytes=self.bytes, max_bytes=self.max_bytes, top_bytes=top.bytes if top else 0, top_splats=len(top.idx) if top else 0,
                    evicted=self.evicted, uncovered_transforms=self.uncovered)


def info_dict(native) -> dict:
    """a gs_edit_history_info as the dictionary History.info() returns"""
    return {name: int(getattr(native, name)) for name, _ in native._fields_}
