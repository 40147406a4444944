"""Seeded edit sessions with undo and redo on the GPU: eight seeds of about forty calls on 1,000 splats -- selection calls, delete, the transforms with
their mouse-down stores, the rigid setting on and off, checkpoints, undo, redo -- enqueued back to back (the raw C calls; only a checkpoint waits, for
its 4-byte count) and run in lock step with tests/undo_model.py composed over the edit / transform / rigid models (tests/undo_rig.py).  The renderer's
whole state is compared at checkpoints only and at the end, so that an ordering edge missing between two calls shows.  The plan of a seed is made on the
host from the seed alone; the CPU test runs the same plans through the models and asserts what they cover."""
import numpy as np
import pytest

import edit_model as EM
import undo_model as UM
from common import small_asset
from undo_rig import FULL, Q1, URig

N, SEEDS, CALLS = 1000, 8, 40
Q2 = (-1.0, 1.0, 1.0, 1.0)
WHATS = (FULL, FULL, FULL, UM.SELECTION | UM.DELETED, UM.TRANSFORM, UM.SELECTION, UM.POS | UM.SELECTION)


def budget() -> int:
    """one entry of a 30 % selection with every kind: a 60 % selection alone does not fit, and a busy session evicts (its entries are mostly smaller)"""
    return UM.entry_bytes(UM.SELECTION | UM.DELETED | UM.RECORDS, (N + 31) // 32, (3 * N) // 10)


def run_session(seed: int, rig: URig) -> set:
    """the session of `seed` on rig (ctx None: the models alone); returns the kinds of situation it met"""
    rng = np.random.default_rng(1000 + seed)
    kinds, h = set(), rig.h
    last = []                                                      # the calls so far, by name
    rig.upload_selected(EM.pack_bits(rng.random(N) < 0.3, rig.m.nw))
    rig.store3()

    def upload():
        rig.upload_selected(EM.pack_bits(rng.random(N) < float(rng.choice([0.02, 0.3, 0.6])), rig.m.nw))

    def checkpoint(what=None):
        evicted = h.evicted
        code = rig.checkpoint(int(rng.choice(WHATS)) if what is None else what, want=None)
        if code == UM.OOM:
            kinds.add("entry over the budget")
        if h.evicted != evicted:
            kinds.add("eviction")
        rig.check(f"seed {seed}, call {len(last)}: checkpoint")     # the only comparisons before the end

    def transform(fn, *args):
        uncovered = h.uncovered
        fn(*args)
        if h.uncovered != uncovered:
            kinds.add("uncovered transform")

    def gesture(fn, *args):
        rig.store3()
        checkpoint(FULL)
        transform(fn, *args)

    def toggle_rigid():
        rig.set_rigid(not rig.m.rigid)

    def undo():
        if h.undo_stack and last and last[-1] in ("translate", "rotate", "scale", "bare translate"):
            kinds.add("undo directly after a transform")
        rig.undo()

    calls = [("upload", upload), ("select all", rig.select_all), ("deselect all", rig.deselect_all), ("invert", rig.invert), ("delete", rig.delete),
             ("translate", lambda: gesture(rig.translate, tuple(rng.uniform(-0.5, 0.5, 3)))),
             ("rotate", lambda: gesture(rig.rotate, Q1 if rng.random() < 0.5 else Q2)),
             ("scale", lambda: gesture(rig.scale, (1.25, 1.25, 1.25) if rng.random() < 0.5 else (1.5, -0.5, 0.25))),
             ("bare translate", lambda: transform(rig.translate, (0.125, 0.0, -0.25))), ("rigid", toggle_rigid), ("checkpoint", checkpoint),
             ("undo", undo), ("undo", undo), ("undo", undo), ("redo", rig.redo), ("redo", rig.redo)]
    for _ in range(CALLS):
        name, fn = calls[int(rng.integers(len(calls)))]
        depth = (len(h.undo_stack), len(h.redo_stack))
        fn()
        if name in ("undo", "redo") and depth == (len(h.undo_stack), len(h.redo_stack)):
            name += " of nothing"
        last.append(name)
        if [c for c in last if not c.endswith("of nothing")][-3:] == ["undo", "redo", "undo"] and last[-1] == "undo":
            kinds.add("undo, redo, undo")
    rig.check(f"seed {seed}: the end")
    while h.undo_stack:                                            # ... and the whole stack undone, back to back
        rig.undo()
    rig.check(f"seed {seed}: the whole stack undone")
    return kinds


def test_the_seeds_cover_what_they_are_for():
    a = small_asset(N, 5, "VeryHigh")
    kinds, uncovered = set(), 0
    for seed in range(SEEDS):
        rig = URig(None, a, max_bytes=budget(), rigid=seed % 2 == 1)
        kinds |= run_session(seed, rig)
        uncovered += rig.h.uncovered
    assert {"undo directly after a transform", "undo, redo, undo", "eviction", "uncovered transform"} <= kinds, kinds
    assert uncovered > 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(SEEDS))
def test_session(gpu_ctx, seed):
    rig = URig(gpu_ctx, small_asset(N, 5, "VeryHigh"), max_bytes=budget(), rigid=seed % 2 == 1)
    run_session(seed, rig)
    assert rig.info() == rig.h.info()                              # the counters, uncovered_transforms among them, and the partly restored state above
    rig.close()
