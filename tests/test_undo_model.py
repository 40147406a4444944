"""The edit history without a GPU: the numpy model of the stack (tests/undo_model.py) held to the properties an undo must have on seeded random
sequences, the shipped count / rank arithmetic (csrc/gs_device_math.h, run by tests/undo_host_harness.cpp the way the kernels run it) held to the model
byte for byte, the bindings' layout, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import undo_model as UM
from harness import build_harness, run_under_sanitizers
from unitygaussiansplatting_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = UM.SELECTION | UM.DELETED | UM.TRANSFORM
SIZES = [1, 31, 32, 33, 70, 255, 256, 257, 300]
SEEDS = 240


def random_words(rng, n, nw, density):
    w = np.zeros(nw, np.uint32)
    idx = np.flatnonzero(rng.random(n) < density)
    np.bitwise_or.at(w, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    if n % 32 and rng.random() < 0.5:
        w[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # the bits beyond N that select-all and invert set
    return w


def same(a, b) -> bool:
    return all(np.array_equal(x, y) for x, y in zip(a, b))


class Session:
    """one seeded sequence of {mutate, checkpoint, undo, redo} over a State and its History, asserting as it goes"""

    def __init__(self, seed):
        self.rng = rng = np.random.default_rng(seed)
        n = SIZES[seed % len(SIZES)]
        self.full_only = seed % 2 == 0                             # every checkpoint captures everything: the LIFO property applies
        self.careful = seed % 4 == 0                               # ... and every transform follows a checkpoint of its own
        self.t = UM.State(n, rng, pos_gate=seed % 7 != 3, rot_gate=seed % 11 != 5, rigid=seed % 3 != 1)
        self.h = UM.History(self.t)
        one = UM.entry_bytes(self.h.resolve(FULL), self.t.nw, n)
        self.h.enable(max(1, int(one * [0.5, 1.2, 2.5, 100.0][(seed // 2) % 4])))
        self.snap = {}                                             # id(entry) -> the state at its checkpoint
        self.owner = None                                          # the entry whose gesture is in progress: pushed last, no undo / redo since
        self.owner_exact = False                                   # ... and everything changed since was captured by it
        self.last_op = None
        self.streak = []                                           # the undo / redo calls since the last other call that did something
        self.kinds = set()

    # -- the mutations, each with the hook the library's call has ------------------------------------------------------------------------------
    def select(self):
        t = self.t
        self.h.mutated(True)
        t._ensure()
        t.sel = random_words(self.rng, t.n, t.nw, self.rng.choice([0.0, 0.05, 0.5, 1.0]))
        self._changed(UM.SELECTION)

    def delete(self):
        t = self.t
        self.h.mutated(True)
        t._ensure()
        t.deleted = (np.zeros(t.nw, np.uint32) if t.deleted is None else t.deleted) | t.sel
        t.sel = np.zeros(t.nw, np.uint32)
        self._changed(UM.SELECTION | UM.DELETED)

    def set_deleted(self):
        t = self.t
        self.h.mutated(False)
        t.deleted = None if self.rng.random() < 0.2 else random_words(self.rng, t.n, t.nw, 0.3)
        self._changed(UM.DELETED)

    def transform(self):
        """what a transform may write: the selected splats' records, of the kinds whose gate passes (SH only in rigid mode)"""
        t = self.t
        before = self.h.uncovered
        self.h.transform()
        t._ensure()
        idx = UM.selected_indices(t.sel, t.n)
        wrote = 0
        for flag, on in ((UM.POS, t.pos_gate), (UM.OTHER, t.rot_gate), (UM.SH, t.rot_gate and t.rigid)):
            if on:
                rows = getattr(t, UM.BLOB[flag])[:t.n * UM.STRIDE[flag]].reshape(t.n, UM.STRIDE[flag])
                rows[idx] = self.rng.integers(0, 256, (len(idx), UM.STRIDE[flag]), dtype=np.uint8)
                wrote |= flag
        if self.h.uncovered != before:
            self.kinds.add("uncovered transform")
            self.owner_exact = False
        else:
            self._changed(wrote)
        self.last_op = "transform"

    def gesture(self):
        """what an editor does: the checkpoint where the tool stores its mouse-down copies, then the transform"""
        self.checkpoint()
        self.transform()

    def _changed(self, flags):
        if self.owner is not None and flags & ~self.owner.what:
            self.owner_exact = False
        self.streak = []
        self.last_op = "mutate"

    # -- the history's calls ---------------------------------------------------------------------------------------------------------------------
    def checkpoint(self):
        h = self.h
        what = FULL if self.full_only else int(self.rng.choice([FULL, UM.SELECTION, UM.DELETED, UM.TRANSFORM, UM.POS | UM.SELECTION, UM.SELECTION | UM.DELETED]))
        state, depth, redo, evicted = self.t.snapshot(), len(h.undo_stack), len(h.redo_stack), h.evicted
        rc = h.checkpoint(what)
        if rc == UM.OOM:
            self.kinds.add("entry over the budget")
            assert same(self.t.snapshot(), state) and (len(h.undo_stack), len(h.redo_stack), h.evicted) == (depth, redo, evicted)
            return
        assert rc == UM.OK
        if h.resolve(what) == 0:
            self.kinds.add("nothing captured")
            assert len(h.undo_stack) == depth
            return
        assert same(self.t.snapshot(), state), "a checkpoint changes nothing"
        assert not h.redo_stack
        if redo:
            self.kinds.add("checkpoint drops redo")
        if h.evicted != evicted:
            self.kinds.add("eviction")
        e = h.undo_stack[-1]
        assert e.bytes == UM.entry_bytes(e.what, self.t.nw, len(e.idx)) <= 8 * self.t.nw + 224 * len(e.idx) + 4096
        self.snap[id(e)] = state
        self.owner, self.owner_exact = e, True
        self.streak = []
        self.last_op = "checkpoint"

    def undo(self):
        h = self.h
        if not h.undo_stack:
            self.kinds.add("undo of an empty stack")
            state = self.t.snapshot()
            assert h.undo() == UM.OK and same(self.t.snapshot(), state)
            return
        e = h.undo_stack[-1]
        before = self.t.snapshot()
        if self.last_op == "transform":
            self.kinds.add("undo directly after a transform")
        assert h.undo() == UM.OK and h.redo_stack[-1] is e
        mid = self.t.snapshot()
        if e is self.owner and self.owner_exact:                   # checkpoint, mutations of captured state, undo: the identity
            assert same(mid, self.snap[id(e)]), "undo did not restore the checkpoint's state"
            self.kinds.add("undo is the identity")
        assert h.redo() == UM.OK and same(self.t.snapshot(), before), "redo after undo is not the identity"
        assert h.undo() == UM.OK and same(self.t.snapshot(), mid)
        self.owner = None
        self.streak.append("undo")
        self.last_op = "undo"

    def redo(self):
        h = self.h
        if not h.redo_stack:
            state = self.t.snapshot()
            assert h.redo() == UM.OK and same(self.t.snapshot(), state)
            return
        assert h.redo() == UM.OK
        self.owner = None
        self.streak.append("redo")
        if self.streak[-2:] == ["undo", "redo"]:
            self.kinds.add("undo then redo")
        self.last_op = "redo"

    def run(self, steps=40):
        h = self.h
        move = self.gesture if self.careful else self.transform
        ops = [self.select, self.delete, self.set_deleted, move, move, self.checkpoint, self.checkpoint, self.undo, self.undo, self.redo]
        for _ in range(steps):
            redo = len(h.redo_stack)
            op = ops[int(self.rng.integers(len(ops)))]
            op()
            if op in (self.select, self.delete, self.set_deleted, self.transform, self.gesture):
                assert not h.redo_stack
                if redo:
                    self.kinds.add("a mutation drops redo")
            if self.streak[-3:] == ["undo", "redo", "undo"]:
                self.kinds.add("undo, redo, undo")
            assert h.bytes == sum(e.bytes for e in h.undo_stack + h.redo_stack) <= h.max_bytes, "the budget is exceeded"
            info = h.info()
            assert (info["undo_depth"], info["redo_depth"]) == (len(h.undo_stack), len(h.redo_stack))
        # LIFO undo of the whole stack
        if h.undo_stack:
            want = self.snap[id(h.undo_stack[0])]
            while h.undo_stack:
                assert h.undo() == UM.OK
            if self.full_only and h.uncovered == 0:
                assert same(self.t.snapshot(), want), "undoing the whole stack did not restore the oldest checkpoint's state"
                self.kinds.add("whole stack undone")
        return self.kinds


def test_properties_on_seeded_sequences():
    kinds = set()
    for seed in range(SEEDS):
        kinds |= Session(seed).run()
    want = {"uncovered transform", "entry over the budget", "nothing captured", "checkpoint drops redo", "eviction", "undo of an empty stack",
            "undo directly after a transform", "undo is the identity", "undo then redo", "undo, redo, undo", "a mutation drops redo", "whole stack undone"}
    assert kinds == want, (want - kinds, kinds - want)


def test_refusals_and_the_switch():
    t = UM.State(70, np.random.default_rng(1))
    h = UM.History(t)
    assert h.checkpoint(FULL) == UM.BAD and h.undo() == UM.BAD and h.redo() == UM.BAD      # off
    h.transform(); h.mutated(True)
    assert h.uncovered == 0 and h.sel_gen == 0                     # the hooks do nothing while it is off
    h.enable(1 << 20)
    assert h.checkpoint(0) == UM.BAD and h.checkpoint(32) == UM.BAD and h.checkpoint(FULL | 64) == UM.BAD
    t._ensure(); t.sel[0] = 0b1011
    assert h.checkpoint(FULL) == UM.OK and h.info()["top_splats"] == 3 and h.info()["top_what"] == UM.SELECTION | UM.DELETED | UM.RECORDS
    t.rigid = False
    assert h.checkpoint(UM.TRANSFORM) == UM.OK and h.info()["top_what"] == UM.POS | UM.OTHER
    h.enable(h.undo_stack[-1].bytes)                               # a smaller budget evicts the oldest
    assert h.info()["undo_depth"] == 1 and h.evicted == 1
    h.enable(0)
    assert not h.enabled and not h.undo_stack and h.evicted == 0


# ---- the shipped arithmetic, on the host ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def undo_harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("undo"), "undo_host_harness.cpp", exe=True)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 513])
def test_host_gather_and_swap_equal_the_model(undo_harness, tmp_path, n):
    rng = np.random.default_rng(n)
    nw = (n + 31) // 32
    tail = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF) if n % 32 else np.uint32(0)
    cases = {"all with the tail bits": ~np.zeros(nw, np.uint32), "none but the tail bits": np.zeros(nw, np.uint32), "half": random_words(rng, n, nw, 0.5),
             "few": random_words(rng, n, nw, 0.03)}
    cases["none but the tail bits"][-1] |= tail
    cases["half"][-1] |= tail
    for name, sel in cases.items():
        then = [rng.integers(0, 256, n * s, dtype=np.uint8) for s in (12, 16, 192)]
        now = [rng.integers(0, 256, n * s, dtype=np.uint8) for s in (12, 16, 192)]
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        with open(src, "wb") as f:
            f.write(np.array([n, nw], np.uint32).tobytes() + sel.tobytes() + b"".join(b.tobytes() for b in then + now))
        out = subprocess.run([undo_harness, str(src), str(dst)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (name, out.stderr)
        got = np.fromfile(dst, np.uint8)
        # the model: a checkpoint of the records in the first state, an undo in the second
        idx = UM.selected_indices(sel, n)
        if name == "all with the tail bits":
            assert len(idx) == n                                   # not 64 at N = 33
        journal = [UM.gather(b, idx, s) for b, s in zip(then, (12, 16, 192))]
        after = [b.copy() for b in now]
        for b, j, s in zip(after, journal, (12, 16, 192)):
            UM.swap_records(b, j, idx, s)
        assert all(np.array_equal(j, UM.gather(b, idx, s)) for j, b, s in zip(journal, now, (12, 16, 192)))       # the entry holds what it replaced
        want = np.concatenate([np.array([len(idx)], np.uint32).view(np.uint8), UM.block_counts(sel, n).view(np.uint8), idx.view(np.uint8)] + journal + after)
        assert np.array_equal(got, want), (name, n)


def test_host_harness_under_the_sanitizers(tmp_path):
    """the stand-alone program over its own input (513 splats, every third selected, the tail bits set), built with ASan and UBSan"""
    out = run_under_sanitizers(tmp_path, "undo_host_harness.cpp", "UNDO_HARNESS_SANITIZED")
    assert out.returncode == 0 and "undo_host_harness ok" in out.stdout, out.stderr[-2000:]


# ---- the bindings -----------------------------------------------------------------------------------------------------------------------------
def test_the_struct_and_the_flags_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "gsplat_c.h")).read()
    flags = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define GS_HIST_([A-Z]+)\s+(0x[0-9A-Fa-f]+u|\d+u)", hdr)}
    assert flags == {"SELECTION": UM.SELECTION, "DELETED": UM.DELETED, "POS": UM.POS, "OTHER": UM.OTHER, "SH": UM.SH, "TRANSFORM": UM.TRANSFORM}
    assert flags == {k: getattr(_abi, "GS_HIST_" + k) for k in flags}
    body = re.search(r"typedef struct gs_edit_history_info \{(.*?)\} gs_edit_history_info;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S).group(1)
    names = [n for decl in re.findall(r"uint(?:32|64)_t ([^;]+);", body) for n in re.split(r",\s*", decl.strip())]
    assert names == [n for n, _ in _abi.gs_edit_history_info._fields_]
    assert C.sizeof(_abi.gs_edit_history_info) == 56
    from unitygaussiansplatting_amd.renderer import EditHistoryFlags
    assert {f.name.upper(): int(f) for f in EditHistoryFlags} == flags


def test_argument_validation_without_a_device():
    lib = _lib.lib()
    bad = _abi.GS_ERR_INVALID_ARGUMENT
    info = _abi.gs_edit_history_info()
    assert lib.gs_renderer_edit_history_enable(None, 1 << 20) == bad and lib.gs_renderer_edit_history_enable(None, 0) == bad
    assert lib.gs_renderer_edit_checkpoint(None, _abi.GS_HIST_SELECTION) == bad and lib.gs_renderer_edit_checkpoint(None, 0) == bad
    assert lib.gs_renderer_edit_undo(None) == bad and lib.gs_renderer_edit_redo(None) == bad
    assert lib.gs_renderer_edit_history_clear(None) == bad
    assert lib.gs_renderer_edit_history_info(None, C.byref(info)) == bad and lib.gs_renderer_edit_history_info(None, None) == bad
    assert b"null" in lib.gs_last_error_string()
