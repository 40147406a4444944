"""The session model on the CPU box (tests/session_model.py; the GPU side is tests/test_gpu_session_fuzz.py): the premises of the suite's eight programs --
every op kind and every listed transition occurs inside a burst --, the conditions that keep the checkpoints from being vacuous, the observability of
ten rules of DESIGN.md sections 4.7-4.10 (the model broken one rule at a time must be told from the true one by some checkpoint of some program), and
one program's transform, resize and copy steps replayed through the host builds of gs_device_math.h (tests/transform_host_harness.cpp,
tests/copy_host_harness.cpp), bit for bit.  No renderer is made: FrameParams comes from a context-free probe."""
import ctypes as C
import functools

import numpy as np
import pytest

import bake_model as BM
import copy_model as CM
import edit_model as EM
import session_model as SM
import transform_model as TM
from builders import params_of
from common import _p
from harness import build_harness
from unitygaussiansplatting_amd import _abi, creator

f32 = np.float32
TRANSFORMS = ("translate", "rotate", "scale")


@functools.lru_cache(maxsize=None)
def trace(seed: int):
    """the true model run over a program: [(op, result, burst number, context)] and the digests.  context: what a premise needs to know about the moment"""
    s = SM.Session(seed)
    rows, digests, burst = [], [], 0
    last_store = {"T": -1, "S": -1, "G": -1}
    for k, op in enumerate(SM.program(seed)):
        if op.name in SM.CHECKPOINTS:
            burst += 1
        if op.name in ("store_pos", "store_other"):
            last_store[op.who] = k
        res = s.apply(op)
        if op.name == "bake" and res.bake is not None and res.bake[0] is not None:
            BM.assert_no_negative_zero(BM.columns(res.bake[0]))    # the input of every bake checkpoint
        if op.name == "bake_cluster" and res.bake[0] is not None:
            BM.assert_no_negative_zero(BM.columns(res.bake[0]))
            assert np.isfinite(res.bake[0]).all()
        ctx = dict(step=k, lanes_t=s.r["T"].settings["lanes"], last_store=dict(last_store), n_t=s.r["T"].n,
                   alive={w: (int(s.r[w].alive().sum()), s.r[w].n) for w in s.live()} if op.name in ("export", "export_all", "bake", "bake_cluster") else None)
        rows.append((op, res, burst, ctx))
        digests.append(s.observe(op, res))
    return rows, digests


def in_burst(rows, preds, adjacent=True):
    """some burst holds calls matching preds in this order (adjacent: with no other call between them); never a checkpoint between them"""
    bursts = {}
    for row in rows:
        if row[0].name not in SM.CHECKPOINTS:
            bursts.setdefault(row[2], []).append(row)
    for calls in bursts.values():
        for start in range(len(calls)):
            k, matched = start, 0
            for p in preds:
                while not adjacent and matched and k < len(calls) and not p(*calls[k]):
                    k += 1
                if k >= len(calls) or not p(*calls[k]):
                    break
                k, matched = k + 1, matched + 1
            if matched == len(preds):
                return True
    return False


def is_op(name, who=None, moved=False, rc=None, arg0=None):
    def p(op, res, burst, ctx):
        return ((op.name == name if isinstance(name, str) else op.name in name) and (who is None or op.who == who) and (not moved or res.moved > 0)
                and (rc is None or res.rc == rc) and (arg0 is None or op.args[0] == arg0))
    return p


# ---- 1. premises ---------------------------------------------------------------------------------------------------------------------------------
def test_the_program_is_a_pure_function_of_the_seed():
    a = SM._Gen(3).run()
    assert tuple(a) == SM.program(3) and tuple(SM._Gen(4).run()) != tuple(a)
    for seed in SM.SUITE_SEEDS:
        ops = SM.program(seed)
        calls = [op for op in ops if op.name not in SM.CHECKPOINTS]
        bursts = SM.bursts_of(ops)
        print(seed, "calls", len(calls), "bursts", len(bursts), "checkpoints", len(ops) - len(calls))
        assert 35 <= len(calls) <= 65 and all(len(b) >= 1 for b in bursts)      # at most 5 mutating calls in a burst, and the blocking calls that came with them
        assert all(sum(op.name in SM.MUTATING for op in b) <= 5 for b in bursts)
        assert ops[-1].name == "state"
        for op in ops:
            assert all(isinstance(v, (int, float, str, type(None))) for v in op.args)
            assert all(float(f32(v)) == v for v in op.args if isinstance(v, float))   # arguments are float32 values


def test_the_suite_covers_the_configurations():
    cfg = [SM.config(s) for s in SM.SUITE_SEEDS]
    assert {c.preset for c in cfg} == {"VeryLow", "Low", "Medium", "High", "VeryHigh"}
    assert {int(c.mode) for c in cfg} == {int(SM.SortMode.Full), int(SM.SortMode.Visible)}
    assert sum(c.lanes == 2 for c in cfg) == 2 and sum(c.ctx2 for c in cfg) == 2 and sum(c.cluster for c in cfg) == 2
    assert SM.SRC_TR.scale[0] < 0 and len(set(np.abs(SM.SRC_TR.scale))) == 3       # mirrored, non-uniformly scaled
    # the signal_to pair of a cross-context copy inside a burst, with a source that really moves before and after the copy
    cross = [s for s in SM.SUITE_SEEDS if SM.config(s).ctx2]
    for name in ("transform of S -> copy S->T", "copy S->T -> transform of S"):
        assert any(in_burst(trace(s)[0], TRANSITIONS[name]) for s in cross), name


def test_every_op_kind_occurs():
    seen = {op.name for s in SM.SUITE_SEEDS for op in SM.program(s)}
    assert seen == SM.MUTATING | SM.BLOCKING | SM.CHECKPOINTS, (SM.MUTATING | SM.BLOCKING | SM.CHECKPOINTS) ^ seen
    rows = [r for s in SM.SUITE_SEEDS for r in trace(s)[0]]
    refused = lambda name, who: any(op.name == name and op.who in who and res.rc == SM.BAD for op, res, _, _ in rows)
    assert refused("rotate", "T") and refused("scale", "T")         # without the stores
    assert refused("resize", "SG")                                 # a chunked renderer
    assert any(op.name == "resize" and res.rc == SM.OK and op.args[0] == ctx["n_t"] for op, res, _, ctx in rows)
    assert {op.args[0] for op, _, _, _ in rows if op.name == "bake_refused"} == {"bc7", "cluster"}
    assert any(op.name == "copy" and op.who == "G" and res.moved for op, res, _, _ in rows) and any(op.name == "bake" and op.who == "G" and res.rc == SM.OK for op, res, _, _ in rows)
    assert any(op.name == "copy" and op.args[1] % 32 and op.args[0] for op, _, _, _ in rows)      # srcStart != 0, dstStart off the word grid
    assert any(op.name == "set_deleted" and op.args[0] is None for op, _, _, _ in rows)
    assert any(op.name == "update" and op.args[0] == 1 for op, _, _, _ in rows) and any(op.name == "update" and op.args[5] == 1 for op, _, _, _ in rows)
    assert sum(op.name == "bake_cluster" and res.rc == SM.OK and res.alive[0] > 4096 for op, res, _, _ in rows) == 2


TRANSITIONS = {
    "translate -> copy-into": [is_op("translate", "T", moved=True), is_op("copy", moved=True)],
    "copy-into -> rotate from an older mouse-down copy": [is_op("copy", moved=True), lambda op, res, b, ctx: is_op("rotate", "T", moved=True, rc=SM.OK)(op, res, b, ctx) and 0 <= ctx["last_store"]["T"] < ctx["step"] - 1],
    "resize -> store -> rotate": [is_op("resize", "T", rc=SM.OK), is_op("store_pos", "T"), is_op("store_other", "T"), is_op("rotate", "T", moved=True, rc=SM.OK)],
    "delete -> translate with two lanes": [is_op("delete", "T"), lambda op, res, b, ctx: is_op("translate", "T")(op, res, b, ctx) and ctx["lanes_t"] == 2],
    "transform of S -> copy S->T": [is_op(TRANSFORMS, "S", moved=True), is_op("copy", "S", moved=True)],
    "copy S->T -> transform of S": [is_op("copy", "S", moved=True), is_op(TRANSFORMS, "S", moved=True)],
    "set cutouts -> resize -> export": [is_op("set_cutouts", "T"), is_op("resize", "T", rc=SM.OK), is_op("export", "T")],
    "bake -> make G -> delete on G -> bake G": [is_op("bake", "T", rc=SM.OK), is_op("make_g"), is_op("delete", "G"), is_op("bake", "G", rc=SM.OK)],
    "release -> translate": [is_op("release", "T"), is_op("translate", "T")],
    "highlight on -> delete -> frame": [is_op("highlight", "T", arg0=1), is_op("delete", "T"), is_op("frame", "T")],
}
# a selection is uploaded between two of the calls, or (cutouts) the raw bake stands between the resize and the export, which on the GPU sends the cutouts again; still no checkpoint
LOOSE = {"resize -> store -> rotate", "bake -> make G -> delete on G -> bake G", "set cutouts -> resize -> export"}


@pytest.mark.parametrize("name", list(TRANSITIONS))
def test_transition_occurs_inside_a_burst(name):
    where = [s for s in SM.SUITE_SEEDS if in_burst(trace(s)[0], TRANSITIONS[name], adjacent=name not in LOOSE)]
    print(name, "in seeds", where)
    assert where


def test_a_raw_reader_of_the_cutouts_follows_a_resize():
    """"Cutouts are re-applied by resize_build" shows on the GPU only to a call that reads the library's cutouts as the resize left them: an export, a frame
    and a twin send the renderer's m_Cutouts again first (SM.REUPLOADS) and so repair whatever the resize did.  So: after a resize of T under cutouts
    that cut an alive splat, a compared raw reader of T (SM.RAW_CUT_READERS) comes before any call of T that sends them again"""
    seen = []
    for seed in SM.SUITE_SEEDS:
        s, pending = SM.Session(seed), None
        for k, op in enumerate(SM.program(seed)):
            n_before = s.r["T"].n
            res = s.apply(op)
            t = s.r["T"]
            if op.name in ("resize", "merge") and (op.who == "T" or op.name == "merge") and res.rc == SM.OK and t.n != n_before:
                pending = k if t.cut_name != "none" and (t.tm.cut & ~t.deleted_flags()).any() else None
            elif pending is not None and (op.who == "T" or op.name == "state"):
                if op.name in SM.RAW_CUT_READERS and op.name in SM.COMPARED and res.rc == SM.OK:
                    seen.append((seed, pending, k, op.name))
                    pending = None
                elif op.name in SM.REUPLOADS:
                    pending = None
    print("resize under cutouts -> raw reader:", seen)
    assert len({seed for seed, _, _, _ in seen}) >= 2, seen


# ---- 2. the checkpoints are not vacuous ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SM.SUITE_SEEDS)
def test_non_vacuity(seed):
    rows, _ = trace(seed)                                          # (BM.assert_no_negative_zero ran on the input of every bake)
    moves = [res.moved > 0 for op, res, _, _ in rows if op.name in TRANSFORMS]
    print(seed, "transforms", len(moves), "that move", sum(moves))
    assert 2 * sum(moves) >= len(moves) > 0
    partial = []
    for op, res, _, ctx in rows:
        if op.name in ("export", "export_all", "bake", "bake_cluster"):
            alive, n = res.alive
            assert res.rc == SM.OK and 1 <= alive, (str(op), alive, n)      # nothing of the suite exports or bakes nothing: the refusals are bake_refused
            assert any(1 <= a <= m - 1 for a, m in ctx["alive"].values()), (str(op), ctx["alive"])
            partial.append(1 <= alive <= n - 1)
    print(seed, "exports and bakes", len(partial), "of a renderer with some but not all alive", sum(partial))
    assert sum(partial) >= 1


def test_copies_copy():
    copies = [res.moved > 0 for s in SM.SUITE_SEEDS for op, res, _, _ in trace(s)[0] if op.name == "copy"]
    print("copies", len(copies), "of at least one splat", sum(copies))
    assert 4 * sum(copies) >= 3 * len(copies) and len(copies) >= 16


# ---- 3. observability ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("broken", SM.BROKEN)
def test_a_broken_rule_is_observed(broken):
    seen = []
    for seed in SM.SUITE_SEEDS:
        truth = trace(seed)[1]
        got = SM.run_model(seed, broken, stop_at=truth)
        k = len(got) - 1
        op = SM.program(seed)[k]
        if got[k] != truth[k] and op.name in SM.COMPARED:          # (a return code alone is not a checkpoint)
            seen.append((seed, k, op.name))
    print(broken, "->", seen)
    assert seen, f"no program of the suite can tell a model in which '{broken}' from the true one"


# ---- 4. the composed model against the host build of gs_device_math.h -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    d = tmp_path_factory.mktemp("session")
    return C.CDLL(build_harness(d, "transform_host_harness.cpp")), C.CDLL(build_harness(d, "copy_host_harness.cpp"))


def host_transform(th, name, st, args):
    """the pos / other blobs the host build leaves after one transform of the state `st` (read before the model applies the op)"""
    tm = st.tm
    pos, other = tm.pos_blob.copy(), tm.other_blob.copy()
    stored = tm.pos_stored and (tm.other_stored or name == "scale")
    if not (tm.pos_gate and tm.rot_gate) or (name != "translate" and not stored) or tm.sel is None:
        return pos, other
    m = tm.selected()
    n = int(m.sum())
    src = tm.pos_rows(pos if name == "translate" else tm.pos_md)[m].copy()
    words = tm.rot_words(other if name != "rotate" else tm.other_md)[m].copy()
    v = np.array(args, f32)
    centre = np.zeros(3, f32) if name == "translate" else v[-3:].copy()
    delta = v[:3].copy() if name != "rotate" else np.ones(3, f32)
    rot = v[:4].copy() if name == "rotate" else np.array([0, 0, 0, 1], f32)
    l2w, w2l = np.ascontiguousarray(SM.TOOL.localToWorldMatrix, f32), np.ascontiguousarray(SM.TOOL.worldToLocalMatrix, f32)
    outT, outR, outS, outW = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, np.uint32)
    th.th_eval(_p(src), _p(words), C.c_uint32(n), _p(centre), _p(l2w), _p(w2l), _p(delta), _p(rot), _p(outT), _p(outR), _p(outS), _p(outW))
    pos[:12 * tm.n].view(f32).reshape(-1, 3)[m] = {"translate": outT, "rotate": outR, "scale": outS}[name]
    if name == "rotate":
        other[:16 * tm.n].view(np.uint32).reshape(-1, 4)[m, 0] = outW
    return pos, other


def host_copy(ch, src, dst: CM.Blobs, transform, src_start, dst_start, count):
    """CSCopySplats' indexing around the host build of gsm::CopySplat, into dst in place"""
    idx = np.arange(count, dtype=np.int64)
    idx = idx[(src_start + idx < src.n) & (dst_start + idx < dst.n)]
    if len(idx) == 0:
        return
    keep = []
    desc = _abi.make_asset_desc(src.asset(), keep)
    n = int(idx[-1]) + 1
    pos, other, texel, sh = np.zeros((n, 3), f32), np.zeros((n, 4), np.uint32), np.zeros((n, 4), f32), np.zeros((n, 45), f32)
    ch.ch_copy(C.byref(desc), None if transform is None else C.byref(params_of(transform)), C.c_uint32(0), C.c_uint32(n), _p(pos), _p(other), _p(texel), _p(sh))
    d = dst_start + idx
    dst.pos.view(f32).reshape(dst.n, 3)[d] = pos[idx]
    dst.other.view(np.uint32).reshape(dst.n, 4)[d] = other[idx]
    dst.color.view(f32).reshape(-1, 4)[creator.SplatIndexToTextureIndex(d.astype(np.uint32))] = texel[idx]
    dst.sh.view(f32).reshape(dst.n, 48)[d, :45] = sh[idx]


def test_one_program_replayed_through_the_host_harnesses(harnesses):
    """seed 7: a VeryHigh source that is itself transformed.  Before every transform, resize and copy step the host build computes, from the model's
    state, what the step must leave; after it the model's blobs must be those, bit for bit"""
    th, ch = harnesses
    seed = 7
    s = SM.Session(seed)
    checked = {"translate": 0, "rotate": 0, "scale": 0, "copy": 0, "resize": 0}
    for k, op in enumerate(SM.program(seed)):
        want = None
        if op.name in TRANSFORMS and s.r[op.who].very_high:
            want = host_transform(th, op.name, s.r[op.who], op.args)
        elif op.name == "copy":
            src, dst = s.r[op.who], s.r["T"]
            want = dst.blobs()
            host_copy(ch, src, want, CM.copy_transform(src.tr, dst.tr), *op.args)
        elif op.name == "resize" and op.who == "T" and op.args[0] != s.r["T"].n:
            want = CM.zero_blobs(op.args[0])
            host_copy(ch, s.r["T"], want, None, 0, 0, s.r["T"].n)
        res = s.apply(op)
        if want is None:
            continue
        st = s.r[op.who] if op.name in TRANSFORMS else s.r["T"]
        if op.name in TRANSFORMS:
            assert TM.blobs_equal(st.tm.pos_blob, want[0], floats=True) and TM.blobs_equal(st.tm.other_blob, want[1], floats=False), (k, str(op))
            checked[op.name] += int(res.moved > 0)
        else:
            got = st.blobs()
            for f in ("pos", "other", "color", "sh"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (k, str(op), f, np.flatnonzero(getattr(got, f) != getattr(want, f))[:8])
            checked[op.name] += int(res.moved > 0 or op.name == "resize")
    print(checked)
    assert all(v > 0 for v in checked.values()), checked
