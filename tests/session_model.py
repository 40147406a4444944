"""One model of an edit session (helper, not a test): the models of the edit features composed -- edit_model / transform_model (selection, deletion,
the three transforms), copy_model (resize and copy-into), export_model (the export records) and bake_model / the Cluster yardstick of
tests/gpu_rig.py (the bake) -- under the rules DESIGN.md sections 4.7-4.10 state about what one feature leaves for another.  No arithmetic of its
own: every number comes out of one of those models.

A session holds up to three renderers' worth of state: T, the target (VeryHigh, 300 splats, under DST_TR); S, a source (one preset per seed, under
SRC_TR: rotated, non-uniformly scaled, mirrored); G, "generation two", a renderer over the asset a bake of T produced.  `program(seed)` is a pure
function of the seed: a list of Ops in bursts of mutating calls with checkpoints between them.  tests/test_session_model.py asserts its premises on the
CPU, tests/test_gpu_session_fuzz.py runs it on the renderers and on this model in lock step.

`Session(seed, broken=...)` breaks exactly one rule (BROKEN): what the CPU test uses to show that the suite's programs can observe each rule.  The
breakage is the library's as the GPU test would meet it (cutouts a resize dropped come back with the next call of REUPLOADS), and `observe` digests
only what the GPU checkpoint of that kind compares."""
from __future__ import annotations

import dataclasses
import functools
import hashlib

import numpy as np

import bake_model as BM
import copy_model as CM
import edit_model as EM
import export_model as XM
import oracle_lib as O
import transform_model as TM
from builders import CAMS, CLUSTER4K, DST_TR, SRC_TR, TOOL
from common import default_camera, small_asset
from unitygaussiansplatting_amd import _abi, asset as A, camera
from unitygaussiansplatting_amd.cutout import shader_data_array
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, SortMode

f32 = np.float32
OK, BAD = 0, _abi.GS_ERR_INVALID_ARGUMENT
RECT_CAMS = [default_camera(), EM.inside_camera()]                 # rectangle selection: an orbit camera and one inside the cloud
CUTOUT_NAMES = list(EM.cutout_lists())
RESIZE_COUNTS = (33, 130, 255, 256, 257, 300, 513, 1000)           # the word and chunk seams, and 300 = N at the start: a no-op
TILES = ((0, 0), (16, 16), (32, 16), (32, 32))
SCALES = (0.5, 0.75, 1.25, 1.5, 2.0, -0.5, -1.25)                  # never 0
VF, CF, SF = A.VectorFormat, A.ColorFormat, A.SHFormat
BC7_TARGET = (VF.Norm11, VF.Norm11, CF.BC7, SF.Norm6)
SUITE_SEEDS = tuple(range(8))
#          S preset    S splats  of which copied  T sort mode       lanes  S on a second context  Cluster4k seed
CONFIGS = [("VeryLow", 20000, 513, SortMode.Full, 1, False, False),
           ("Low", 20000, 513, SortMode.Visible, 1, False, False),
           ("Medium", 257, 257, SortMode.Full, 2, False, False),
           ("High", 513, 513, SortMode.Visible, 2, True, False),
           ("VeryHigh", 513, 513, SortMode.Full, 1, False, False),
           ("VeryHigh", 4500, 4500, SortMode.Visible, 1, False, True),
           ("VeryHigh", 4500, 4500, SortMode.Full, 1, False, True),
           ("VeryHigh", 257, 257, SortMode.Visible, 1, True, False)]     # (a source that is itself moved, on the second context: the phrases with an odd index)
MUTATING = frozenset("""select_all deselect_all invert store_sel update delete set_deleted upload_sel set_cutouts release store_pos store_other translate rotate scale
                        resize copy merge sort_mode lanes limit highlight tile frame""".split())
BLOCKING = frozenset("info export export_all bake bake_cluster bake_refused make_g".split())      # block by themselves: part of a burst as they come
CHECKPOINTS = frozenset("state twin".split())
COMPARED = CHECKPOINTS | frozenset("info export export_all bake bake_cluster".split())      # where the GPU test compares data, not only a return code
# The GPU test makes every call of a burst through the raw entry point, which reads the cutouts the library holds.  These are the exceptions: calls it can
# only make through a method of GaussianSplatRenderer that begins with UpdateCutoutsBuffer() (ExportAlive, ExportPlyFile, EditExportData, CalcViewData), so
# the renderer's m_Cutouts reach the library again before anything reads them; and set_cutouts, which is that upload.  A twin checkpoint draws frames.
REUPLOADS = frozenset("set_cutouts export export_all frame twin".split())
RAW_CUT_READERS = frozenset("info bake bake_cluster state".split())      # compared on the GPU, and read the library's cutouts as a resize left them
BROKEN = ("mouse-down copies survive a resize", "selection survives a resize", "cutouts dropped by a resize", "copy clears deleted bits", "copy skips cut splats",
          "copy loads srcStart + idx", "copy reads the source asset", "release drops the private blobs", "rotate reads the current pos", "export and bake ignore cutouts")


@dataclasses.dataclass(frozen=True)
class Config:
    preset: str
    s_n: int
    s_use: int
    mode: SortMode
    lanes: int
    ctx2: bool
    cluster: bool


def config(seed: int) -> Config:
    return Config(*CONFIGS[seed % len(CONFIGS)])


@dataclasses.dataclass(frozen=True)
class Op:
    name: str
    who: str = "T"                                                 # T, S or G
    args: tuple = ()

    def __str__(self):
        a = ",".join(f"{v:.4g}" if isinstance(v, float) else str(v) for v in self.args)
        return f"{self.name}[{self.who}]({a})" if a else f"{self.name}[{self.who}]"


def words_of(subseed: int, n: int, k: int) -> np.ndarray:
    """ceil(n / 32) random words, the AND of k draws (density 2^-k): a function of the sub-seed and of the N the renderer has when the op runs"""
    rng = np.random.default_rng(90000 + subseed)
    nw = (n + 31) // 32
    w = np.full(nw, 0xFFFFFFFF, np.uint32)
    for _ in range(k):
        w &= rng.integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32)
    return w


def frame_params(tr, cam):
    probe = GaussianSplatRenderer.__new__(GaussianSplatRenderer)   # no context: FrameParams reads the transform and the serialized fields only
    probe.transform, probe.m_SplatScale, probe.m_OpacityScale, probe.m_SHOrder, probe.m_SHOnly = tr, 1.0, 1.0, 3, False
    return probe.FrameParams(cam)


@functools.lru_cache(maxsize=None)
def source_asset(n: int, quality: str, seed: int = 5):
    return small_asset(n, seed, quality)


# ---- the program -------------------------------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, seed: int):
        self.seed, self.cfg = seed, config(seed)
        self.rng = np.random.default_rng(7000 + seed)
        self.ops: list[Op] = []
        self.n_t = 300                                             # T's count: every resize of T succeeds, so the generator knows it
        self.has_g = False
        self.sub = 0

    # -- argument draws: everything a float32 value, so both sides of the lock step read the same bits
    def f(self, lo, hi, k=1):
        v = [float(f32(self.rng.uniform(lo, hi))) for _ in range(k)]
        return v[0] if k == 1 else tuple(v)

    def subseed(self) -> int:
        self.sub += 1
        return self.seed * 1000 + self.sub

    def pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def quat(self):
        q = self.rng.standard_normal(4)
        return tuple(float(v) for v in (q / np.linalg.norm(q)).astype(f32))

    def who(self, allow_s=True):
        r = self.rng.random()
        if self.has_g and r < 0.15:
            return "G"
        return "S" if allow_s and r < 0.4 else "T"

    # -- single ops
    def sel(self, who):
        return Op("upload_sel", who, (self.subseed(), 1))

    def translate(self, who):
        return Op("translate", who, self.f(-0.6, 0.6, 3))

    def rotate(self, who):
        return Op("rotate", who, self.quat() + self.f(-0.5, 0.5, 3))

    def scale(self, who):
        return Op("scale", who, tuple(float(self.pick(SCALES)) for _ in range(3)) + self.f(-0.5, 0.5, 3))

    def copy(self, src):
        use = self.cfg.s_use if src == "S" else 300
        src_start = 0 if self.rng.random() < 0.55 else int(self.rng.integers(1, 41))
        dst_start = int(self.rng.integers(0, max(1, self.n_t - 8))) if self.rng.random() < 0.9 else self.n_t + 5      # (rarely past the end: nothing is copied)
        count = int(self.rng.integers(1, use + 1)) + (100 if self.rng.random() < 0.3 else 0)                          # (+100: past the source's end)
        return Op("copy", src, (src_start, dst_start, min(count, 700)))

    def resize(self, who="T", avoid=None):
        n = int(self.pick([c for c in RESIZE_COUNTS if c != avoid]))
        if who == "T":
            self.n_t = n
        return Op("resize", who, (n,))

    def update(self, who):
        x, y = np.sort(self.rng.uniform(-32.0, 352.0, 2)), np.sort(self.rng.uniform(-20.0, 220.0, 2))
        return Op("update", who, (int(self.rng.integers(2)), float(f32(x[0])), float(f32(y[0])), float(f32(x[1])), float(f32(y[1])), int(self.rng.integers(2))))

    def bake(self, who, chunked=False):
        k = int(self.rng.integers(4 if chunked else len(BM.FORMAT_TARGETS)))
        return Op("bake", who, (k, int(self.rng.integers(2))))

    def export(self, who):
        return Op("export", who, (int(self.rng.integers(2)),))

    def random_op(self) -> Op:
        g = self.rng.random()
        if g < 0.40:                                               # selection and deletion
            who = self.who()
            name = self.pick(["select_all", "deselect_all", "invert", "store_sel", "update", "update", "delete", "set_deleted", "set_deleted_none", "upload_sel",
                              "set_cutouts", "release", "info"])
            if name == "update":
                return self.update(who)
            if name == "set_deleted":
                return Op("set_deleted", who, (self.subseed(), 2))
            if name == "set_deleted_none":                        # (S keeps its bits: every export and bake has a renderer with some but not all splats alive)
                return Op("set_deleted", "T" if who == "S" else who, (None, 0))
            if name == "upload_sel":
                return self.sel(who)
            if name == "set_cutouts":
                return Op("set_cutouts", who, (self.pick(CUTOUT_NAMES),))
            return Op(name, who)
        if g < 0.65:                                               # transforms (rotate / scale also where the stores were not made: the refusal)
            who = self.who(allow_s=self.cfg.preset == "VeryHigh")     # (mostly where the format gates pass: a chunked renderer is left alone)
            name = self.pick(["store_pos", "store_other", "translate", "translate", "translate", "translate", "rotate", "scale"])
            return getattr(self, name)(who) if name in ("translate", "rotate", "scale") else Op(name, who)
        if g < 0.80:                                               # merge
            r = self.rng.random()
            if r < 0.35:
                return self.resize("T")
            if r < 0.45 and (self.cfg.preset != "VeryHigh" or self.has_g):      # refused: a chunked renderer
                return self.resize("G" if self.has_g and (self.cfg.preset == "VeryHigh" or self.rng.random() < 0.5) else "S")
            return self.copy("G" if self.has_g and self.rng.random() < 0.4 else "S")
        who = self.who(allow_s=False) if self.rng.random() < 0.8 else "S"      # settings and frames
        name = self.pick(["sort_mode", "lanes", "limit", "highlight", "tile", "frame", "frame", "frame"])
        if name == "sort_mode":
            return Op(name, who, (int(self.pick([SortMode.Full, SortMode.Visible])),))
        if name == "lanes":
            return Op(name, who, (int(self.pick([1, 2])),))
        if name == "limit":
            return Op(name, who, (int(self.rng.integers(2, 6)),))
        if name == "highlight":
            return Op(name, who, (int(self.rng.integers(2)),))
        if name == "tile":
            return Op(name, who, self.pick(TILES))
        return Op("frame", who, (int(self.rng.integers(len(CAMS))),))

    # -- phrases: the transitions the issue lists, each inside one burst
    def phrases(self):
        c = self.cfg
        yield "move, copy", lambda: [self.sel("T"), self.translate("T"), self.copy("S")]
        yield "copy, rotate from an older mouse-down copy", lambda: [self.sel("T"), Op("store_pos"), Op("store_other"), self.copy("S"), self.rotate("T")]
        yield "resize, store, rotate", lambda: [self.resize("T", avoid=self.n_t), self.sel("T"), Op("store_pos"), Op("store_other"), self.rotate("T")]
        yield "delete, translate", lambda: [self.sel("T"), Op("delete"), self.translate("T"), self.sel("T"), self.translate("T")]
        yield "bits between two moves", lambda: [self.sel("T"), self.translate("T"), Op("set_deleted", "T", (self.subseed(), 2)), self.translate("T"), Op("frame", "T", (1,))]
        if c.preset == "VeryHigh":
            yield "move S, copy, move S", lambda: [self.sel("S"), self.translate("S"), self.copy("S"), self.translate("S")]
        else:                                                      # (a chunked source is left alone by the move)
            yield "move S, copy, move T", lambda: [self.sel("S"), self.translate("S"), self.copy("S"), self.sel("T"), self.translate("T")]
        yield "lanes come and go", lambda: [Op("lanes", "T", (3 - c.lanes,)), self.sel("T"), self.translate("T"), Op("frame", "T", (2,)), Op("lanes", "T", (c.lanes,))]
        # (the raw bake BEFORE the export: on the GPU the export sends the renderer's cutouts again (REUPLOADS), so only a raw reader directly behind the
        #  resize sees what resize_build made of them)
        yield "cutouts, resize, export", lambda: [Op("set_cutouts", "T", (self.pick(CUTOUT_NAMES[1:]),)), self.resize("T", avoid=self.n_t), self.bake("T"), self.export("T"), Op("set_cutouts", "T", ("none",))]
        yield "release, translate", lambda: [self.sel("T"), self.translate("T"), Op("release"), self.translate("T"), self.scale("T")]      # (the scale: refused)
        yield "highlight, delete, frame", lambda: [self.sel("T"), Op("highlight", "T", (1,)), Op("delete"), Op("frame", "T", (0,)), Op("highlight", "T", (0,))]
        yield "select, resize, raw rotate", lambda: [Op("store_pos"), Op("store_other"), self.resize("T", avoid=self.n_t), self.sel("T"), self.rotate("T")]      # (refused)
        yield "cut source, copy", lambda: [Op("set_cutouts", "S", (self.pick(CUTOUT_NAMES[1:]),)), self.copy("S"), Op("set_cutouts", "S", ("none",))]
        yield "deleted under a copy", lambda: [Op("set_deleted", "T", (self.subseed(), 1)), Op("set_deleted", "S", (self.subseed(), 2)), Op("copy", "S", (3, 16, 200))]
        yield "scale from the mouse-down copy", lambda: [self.sel("T"), Op("store_pos"), self.translate("T"), self.scale("T")]
        yield "settings", lambda: [Op("limit", "T", (int(self.rng.integers(2, 6)),)), Op("tile", "T", self.pick(TILES[1:])), Op("sort_mode", "T", (1 - int(c.mode),)), Op("frame", "T", (1,)), Op("info", "T")]
        yield "rectangles", lambda: [Op("select_all"), self.update("T"), Op("invert"), Op("store_sel"), self.update("T")]
        yield "refusals", lambda: [Op("bake_refused", "T", ("bc7",)), Op("bake_refused", "T", ("cluster",))] if not c.cluster else [Op("bake_refused", "T", ("bc7",))]

    def generation_two(self):
        ops = [Op("set_cutouts", "T", ("none",)), Op("set_deleted", "T", (self.subseed(), 2)), self.bake("T", chunked=True), Op("make_g", "T"),
               self.sel("G"), Op("delete", "G"), Op("resize", "G", (513,)), self.bake("G")]      # (three quarters of T alive when it is baked; the resize of G: refused)
        self.has_g = True
        return ops

    def cluster(self):
        """grow T past 4,096 alive by MergeSplatObjects' two calls from the 4,500-splat source, then bake to Cluster4k"""
        ops = [Op("set_deleted", "S", (None, 0)), Op("set_deleted", "T", (self.subseed(), 3)), Op("set_cutouts", "T", ("none",)), Op("merge", "S"), Op("bake_cluster", "T", (int(self.rng.integers(2)),))]
        self.n_t += self.cfg.s_n
        return ops

    def burst(self, ops, twin=None):
        self.ops += ops
        self.ops.append(Op("state"))
        if twin:
            self.ops.append(Op("twin", twin))

    def run(self) -> list[Op]:
        rng, c = self.rng, self.cfg
        self.burst([Op("set_deleted", "S", (self.subseed(), 3))])
        named = list(self.phrases())
        keep = [k for k in range(len(named)) if (k + self.seed) % 2 == 0]      # every other phrase: each phrase in four of the suite's eight seeds
        picked = [named[int(k)] for k in rng.permutation(keep)]
        # first, while T still holds the asset's 300 splats: the release (later a resize leaves nothing behind the private blobs) and the export under cutouts
        picked.sort(key=lambda p: p[0] not in ("release, translate", "cutouts, resize, export"))
        slots = [p[1] for p in picked]
        slots.insert(int(rng.integers(2, 5)), self.generation_two)
        if c.cluster:
            slots.insert(int(rng.integers(4, 7)), self.cluster)
        twins = 0
        for k, make in enumerate(slots):
            ops = make()
            who = "G" if (self.has_g and twins % 3 == 1) else ("S" if twins % 3 == 2 else "T")      # the twins go round: T, G, S
            want_twin = k % 3 == 1
            self.burst(ops, who if want_twin else None)
            twins += int(want_twin)
            if k % 4 == 1:                                         # a random burst of 1 to 5 calls
                extra = []
                for _ in range(int(rng.integers(1, 6))):
                    op = self.random_op()
                    if op.name in ("translate", "rotate", "scale") and len(extra) < 4 and not any(e.name == "upload_sel" and e.who == op.who for e in extra):
                        extra.append(self.sel(op.who))            # something to move
                    if len(extra) < 5:
                        extra.append(op)
                if rng.random() < 0.5:
                    extra.append(self.export(self.who()))
                elif rng.random() < 0.4:
                    extra.append(self.bake(self.who()))
                self.burst(extra)
        self.burst([Op("export_all", "T", (int(rng.integers(2)),))])      # EditExportData: once per session
        return self.ops


@functools.lru_cache(maxsize=None)
def program(seed: int) -> tuple:
    """the ops of a seed, checkpoints included: a pure function of the seed"""
    return tuple(_Gen(seed).run())


def bursts_of(ops):
    """the runs of calls between two checkpoints"""
    out, cur = [], []
    for op in ops:
        if op.name in CHECKPOINTS:
            if cur:
                out.append(cur)
            cur = []
        else:
            cur.append(op)
    if cur:
        out.append(cur)
    return out


# ---- one renderer's worth of state ---------------------------------------------------------------------------------------------------------------
class RState:
    def __init__(self, asset, tr, mode=SortMode.Full, lanes=1):
        self.asset0 = asset                                        # what the renderer was created over
        self.tm = TM.TransformModel(asset)
        self.tr = tr
        self.very_high = CM.is_very_high(asset)
        self.private = False                                       # all four blobs are private: a resize or a copy-into has happened
        self.resized = False
        self.cut_name = "none"                                     # the renderer's m_Cutouts, by name
        self.cut_stale = False                                     # broken model only: the library's cutouts are not m_Cutouts until they are sent again
        self.order = np.arange(asset.splatCount, dtype=np.uint32)
        self.settings = dict(sort_mode=int(mode), lanes=lanes, limit=None, highlight=0, tile=(0, 0))
        self._dec = None

    @property
    def n(self) -> int:
        return self.tm.n

    def asset(self):
        return self.tm.current_asset()

    def dec(self) -> np.ndarray:
        """LoadSplatData of every splat of the current blobs"""
        if self._dec is None:
            self._dec = CM.decode(self.asset())
        return self._dec

    def changed(self) -> None:
        self._dec = None

    def blobs(self) -> CM.Blobs:
        b = CM.blobs_of(self.asset())
        b.deleted = None if self.tm.deleted is None else self.tm.deleted.copy()
        return b

    def tails(self):
        """the bytes behind whole records an unresized renderer's blobs carry (the asset's pads); None once resized"""
        if self.resized:
            return None
        a, n = self.asset(), self.n
        w, h = A.CalcTextureSize(n)
        return [np.ascontiguousarray(b, np.uint8)[s:].tobytes() for b, s in zip((a.posData, a.otherData, a.colorData, a.shData), (12 * n, 16 * n, w * h * 16, 192 * n))]

    def adopt(self, b: CM.Blobs) -> None:
        """the four blobs after a copy-into, behind them the pads they had"""
        t = self.tails() or [b""] * 4
        join = lambda x, tail: np.concatenate([x, np.frombuffer(tail, np.uint8)]) if tail else x.copy()
        self.tm.set_asset(dataclasses.replace(self.tm.asset, posData=join(b.pos, t[0]), otherData=join(b.other, t[1]), colorData=join(b.color, t[2]), shData=join(b.sh, t[3])))
        self.tm.deleted = b.deleted
        self.private = True
        self.changed()

    def deleted_flags(self) -> np.ndarray:
        return EM.unpack_bits(self.tm.bits()[2], self.n)

    def alive(self, ignore_cutouts=False) -> np.ndarray:
        return ~self.deleted_flags() & (~self.tm.cut if not ignore_cutouts else True)

    def cutout_array(self):
        return shader_data_array(EM.cutout_lists()[self.cut_name], self.tr.localToWorldMatrix)


@dataclasses.dataclass
class Result:
    rc: int = OK
    export: np.ndarray | None = None                               # the rows a blocking export must return
    bake: tuple | None = None                                      # (decode of the alive splats, formats, morton, cluster)
    frame: tuple | None = None                                     # (camera, compare with the oracle?, state snapshot for the oracle)
    moved: int = 0                                                 # splats a transform moved / a copy wrote
    alive: tuple | None = None                                     # (alive, N) of an export or a bake


class Session:
    def __init__(self, seed: int, broken: str | None = None):
        assert broken is None or broken in BROKEN
        self.seed, self.cfg, self.broken = seed, config(seed), broken
        c = self.cfg
        self.r: dict[str, RState] = {"T": RState(source_asset(300, "VeryHigh"), DST_TR, c.mode, c.lanes), "S": RState(source_asset(c.s_n, c.preset), SRC_TR)}
        self.last_bake = None                                      # (decode of the alive splats, formats, morton) of the last accepted bake: what make_g uses

    def live(self):
        return [k for k in "TSG" if k in self.r]

    # -- the rules ---------------------------------------------------------------------------------------------------------------------------------
    def _resize(self, st: RState, n: int) -> int:
        if not st.very_high:
            return BAD                                             # a chunked renderer is refused and left alone
        if n == st.n:
            return OK
        b = CM.set_splat_count(st.dec(), st.tm.deleted, n)        # the identity transform
        old = st.tm
        st.tm = TM.TransformModel(b.asset())
        st.tm._ensure()                                            # selection and its copy: zero
        st.tm.deleted = b.deleted
        if self.broken == "cutouts dropped by a resize":           # the library's are gone; m_Cutouts is the renderer object's and stays (REUPLOADS)
            st.cut_stale = True
        elif old._cut_args is not None:
            st.tm.set_cutouts(*old._cut_args)
        if self.broken == "selection survives a resize" and old.sel is not None:
            fit = lambda w: np.concatenate([w, np.zeros(st.tm.nw, np.uint32)])[:st.tm.nw].copy()
            st.tm.sel, st.tm.md = fit(old.sel), fit(old.md)
        if self.broken == "mouse-down copies survive a resize":
            fit = lambda blob, size: None if blob is None else np.concatenate([blob, np.zeros(size, np.uint8)])[:size].copy()
            st.tm.pos_md, st.tm.other_md = fit(old.pos_md, 12 * n), fit(old.other_md, 16 * n)
            st.tm.pos_stored, st.tm.other_stored = old.pos_stored, old.other_stored
        st.private = st.resized = True
        st.order = np.arange(n, dtype=np.uint32)
        st.changed()
        return OK

    def _copy(self, src: RState, dst: RState, src_start: int, dst_start: int, count: int) -> int:
        if not dst.very_high:
            return BAD
        idx = np.arange(count, dtype=np.int64)
        keep = (src_start + idx < src.n) & (dst_start + idx < dst.n)
        idx = idx[keep]
        if len(idx) == 0:
            return OK
        dec = src.dec()                                            # the source's CURRENT blobs and N
        if self.broken == "copy reads the source asset" and src.very_high and not src.resized:
            dec = CM.decode(src.asset0)
        if self.broken == "copy loads srcStart + idx":
            dec = dec[np.minimum(np.arange(src.n) + src_start, src.n - 1)]
        b, before = dst.blobs(), dst.blobs()
        CM.copy_splats(dec, src.tm.deleted, b, CM.copy_transform(src.tr, dst.tr), src_start, dst_start, count)
        if self.broken == "copy skips cut splats" and src.tm.cut[idx].any():
            back = dst_start + idx[src.tm.cut[idx]]                # the destinations of cut sources keep what they held
            from unitygaussiansplatting_amd import creator
            for name, width, rows in (("pos", 12, back), ("other", 16, back), ("sh", 192, back), ("color", 16, creator.SplatIndexToTextureIndex(back.astype(np.uint32)))):
                getattr(b, name).reshape(-1, width)[rows] = getattr(before, name).reshape(-1, width)[rows]
        if self.broken == "copy clears deleted bits" and b.deleted is not None:
            sw = src.tm.bits()[2]
            clear = ((sw[(src_start + idx) >> 5] >> ((src_start + idx) & 31).astype(np.uint32)) & 1) == 0
            d = dst_start + idx[clear]
            np.bitwise_and.at(b.deleted, d >> 5, ~(np.uint32(1) << (d & 31).astype(np.uint32)))
        dst.adopt(b)
        return OK

    def _reupload(self, st: RState) -> None:
        """UpdateCutoutsBuffer at the head of a call of REUPLOADS: nothing new for the true model, whose cutouts follow every move and resize"""
        if st.cut_stale:
            st.tm.set_cutouts(EM.cutout_lists()[st.cut_name], st.tr.localToWorldMatrix)
            st.cut_stale = False

    def _release(self, st: RState) -> None:
        st.tm.release()
        if self.broken == "release drops the private blobs" and not st.resized and st.very_high:
            keep = st.tm.deleted
            st.tm.set_asset(dataclasses.replace(st.tm.asset, posData=np.array(st.asset0.posData, np.uint8), otherData=np.array(st.asset0.otherData, np.uint8)))
            st.tm.deleted = keep
            st.changed()

    def _rotate(self, st: RState, q, centre) -> tuple:
        tm = st.tm
        before = tm.pos_blob.copy()
        if self.broken == "rotate reads the current pos" and tm.pos_stored and tm.other_stored and tm.pos_gate:
            keep, tm.pos_md = tm.pos_md, tm.pos_blob.copy()
            ok = tm.rotate(centre, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, q)
            tm.pos_md = keep
        else:
            ok = tm.rotate(centre, TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, q)
        return ok, before

    @staticmethod
    def _moved_rows(st: RState, before) -> int:
        if not st.tm.pos_gate or len(before) != len(st.tm.pos_blob):
            return 0
        return int((before[:12 * st.n].reshape(-1, 12) != st.tm.pos_blob[:12 * st.n].reshape(-1, 12)).any(axis=1).sum())

    def _sort(self, st: RState, cam) -> O.Oracle:
        orc = O.Oracle(st.asset())
        orc.order[:] = st.order
        orc.sort(camera.sort_matrix(cam, st.tr.localToWorldMatrix))
        st.order = orc.order.copy()
        return orc

    def oracle_frame(self, st: RState, cam, orc=None):
        """(view records, frame) of the state through a camera, from the state's order, with its deleted bits and cutouts"""
        orc = orc or self._sort(st, cam)
        P = frame_params(st.tr, cam)
        arr, cnt = st.cutout_array()
        view = orc.calc_view(P, arr, cnt, deleted_bits=st.tm.deleted).copy()
        return view, orc.draw(P, 0)

    # -- one op --------------------------------------------------------------------------------------------------------------------------------
    def apply(self, op: Op, draw: bool = False) -> Result:
        """what the op leaves in the model, and what the call must return.  draw: also compute the oracle's image of a frame op"""
        res = Result()
        name, a = op.name, op.args
        if name in CHECKPOINTS:
            if name == "twin":                                     # the twin checkpoint sorts through the three cameras: the order buffer moves on
                self._reupload(self.r[op.who])
                self.twin_frames(op.who, draw=False)
            return res
        src = self.r[op.who]
        st = self.r["T"] if name in ("copy", "merge") else src
        if name in REUPLOADS:
            self._reupload(st)
        tm = st.tm
        if name == "select_all":
            tm.select_all()
        elif name == "deselect_all":
            tm.deselect_all()
        elif name == "invert":
            tm.invert_selection()
        elif name == "store_sel":
            tm.store_selection()
        elif name == "update":
            tm.update_selection(frame_params(st.tr, RECT_CAMS[a[0]]), a[1:5], bool(a[5]))
        elif name == "delete":
            tm.delete_selected()
        elif name == "set_deleted":
            tm.set_deleted_bits(None if a[0] is None else words_of(a[0], st.n, a[1]))
        elif name == "upload_sel":
            tm.upload_selected(words_of(a[0], st.n, a[1]))
        elif name == "set_cutouts":
            st.cut_name = a[0]
            tm.set_cutouts(EM.cutout_lists()[a[0]], st.tr.localToWorldMatrix)
        elif name == "release":
            self._release(st)
        elif name == "info":
            pass
        elif name == "store_pos":
            tm.store_pos()
        elif name == "store_other":
            tm.store_other()
        elif name == "translate":
            before = tm.pos_blob.copy()
            tm.translate(np.array(a, f32))
            res.moved = self._moved_rows(st, before)
            if st.very_high:
                st.changed()
        elif name == "rotate":
            ok, before = self._rotate(st, np.array(a[:4], f32), np.array(a[4:], f32))
            res.rc, res.moved = (OK if ok else BAD), self._moved_rows(st, before)
            if st.very_high:
                st.changed()
        elif name == "scale":
            before = tm.pos_blob.copy()
            ok = tm.scale(np.array(a[3:], f32), TOOL.localToWorldMatrix, TOOL.worldToLocalMatrix, np.array(a[:3], f32))
            res.rc, res.moved = (OK if ok else BAD), self._moved_rows(st, before)
            if st.very_high:
                st.changed()
        elif name == "resize":
            res.rc = self._resize(st, a[0])
        elif name == "copy":
            n0 = len(np.flatnonzero((a[0] + np.arange(a[2]) < src.n) & (a[1] + np.arange(a[2]) < st.n)))
            res.rc, res.moved = self._copy(src, st, *a), n0
        elif name == "merge":                                      # MergeSplatObjects' two calls for one source
            n0 = st.n
            res.rc = self._resize(st, n0 + src.n)
            assert res.rc == OK and self._copy(src, st, 0, n0, src.n) == OK
            res.moved = src.n
        elif name in ("sort_mode", "lanes", "limit", "highlight"):
            st.settings[name] = a[0]
        elif name == "tile":
            st.settings["tile"] = tuple(a)
        elif name == "frame":
            cam = CAMS[a[0]]
            orc = self._sort(st, cam)
            res.frame = (cam, self.oracle_frame(st, cam, orc) if (draw and self.plain_frames(op.who)) else None)
        elif name in ("export", "export_all"):
            cut = tm.cut if self.broken != "export and bake ignore cutouts" else np.zeros(st.n, bool)
            rows = XM.export_records(st.dec(), cut, XM.transform_of(st.tr) if a[0] else None)
            alive = ~st.deleted_flags() & ~cut
            res.export = rows if name == "export_all" else rows[alive]
            res.alive = (int(alive.sum()), st.n)
        elif name in ("bake", "bake_cluster", "bake_refused"):
            alive = st.alive(ignore_cutouts=self.broken == "export and bake ignore cutouts")
            res.alive = (int(alive.sum()), st.n)
            if name == "bake_refused":
                res.rc = BAD
                res.bake = (None, BC7_TARGET if a[0] == "bc7" else CLUSTER4K, True, False)
                assert a[0] == "bc7" or res.alive[0] <= 4096
            elif res.alive[0] == 0 or (name == "bake_cluster" and res.alive[0] <= 4096):
                res.rc = BAD                                       # no alive splat / no more than table entries: a refusal whatever the program meant
                res.bake = (None, CLUSTER4K if name == "bake_cluster" else BM.FORMAT_TARGETS[a[0]], True, False)
            else:
                fmt, morton = (CLUSTER4K, bool(a[0])) if name == "bake_cluster" else (BM.FORMAT_TARGETS[a[0]], bool(a[1]))
                res.bake = (st.dec()[alive], fmt, morton, name == "bake_cluster")
                if st is self.r["T"] and name == "bake":
                    self.last_bake = res.bake
        elif name == "make_g":
            assert self.last_bake is not None, "the program makes G without an accepted bake of T"
            dec_alive, fmt, morton, _ = self.last_bake
            assert fmt != BM.VERY_HIGH                             # G is a chunked renderer
            g = RState(BM.yardstick(dec_alive, fmt, morton), DST_TR, self.cfg.mode, 1)
            self.r["G"] = g
        else:
            raise KeyError(name)
        return res

    def twin_frames(self, who: str, draw: bool = True):
        """the twin checkpoint on the model: the three cameras sorted through from the state's order; ([(view records, frame)] or None, the order at the end)"""
        st = self.r[who]
        frames = [self.oracle_frame(st, cam) if draw else self._sort(st, cam) for cam in CAMS]
        return (frames if draw else None), st.order.copy()

    def plain_frames(self, who: str) -> bool:
        """nothing of the selection is drawn: the frames are the oracle's"""
        st = self.r[who]
        return not st.settings["highlight"] or st.tm.sel is None or not st.tm.sel.any()

    # -- what a checkpoint can see, as a digest ---------------------------------------------------------------------------------------------------
    def observe(self, op: Op, res: Result) -> bytes:
        h = hashlib.sha256()
        put = lambda x: h.update(np.ascontiguousarray(x).tobytes())
        if op.name in ("state", "twin"):                           # state: every live renderer; twin: the frames of one
            for k in (self.live() if op.name == "state" else [op.who]):
                st = self.r[k]
                a = st.asset()
                put(np.array([st.n], np.uint32))
                for blob in (a.posData, a.otherData, a.colorData, a.shData):
                    put(np.asarray(blob, np.uint8))
                for w in st.tm.bits():
                    put(w)
                put(st.order)
                if op.name == "state":
                    put(st.tm.info())                              # (of the cutouts a state checkpoint sees the cut count alone)
                else:
                    put(st.tm.cut)                                 # a frame against the oracle shows which splats are cut
        elif op.name == "info":
            put(self.r[op.who].tm.info())
        elif res.export is not None:
            put(res.export.view(np.uint32))
        elif res.bake is not None:
            put(np.array([res.rc], np.int64))
            if res.bake[0] is not None:
                put(np.ascontiguousarray(res.bake[0]).view(np.uint32))
        else:
            put(np.array([res.rc], np.int64))
        return h.digest()


def run_model(seed: int, broken: str | None = None, stop_at=None):
    """the digests of everything observable, op by op.  stop_at: the digests of the true model -- stops at the first checkpoint that differs"""
    s = Session(seed, broken)
    out = []
    for k, op in enumerate(program(seed)):
        res = s.apply(op)
        out.append(s.observe(op, res))
        if stop_at is not None and out[-1] != stop_at[k] and op.name in COMPARED:
            break
    return out
