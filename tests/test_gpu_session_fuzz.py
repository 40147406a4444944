"""-m gpu: seeded edit sessions -- selection and deletion, the three transforms, resize and copy-into, export, bake and a renderer over the baked asset,
settings and frames -- run on up to three renderers and on the composed model of tests/session_model.py in lock step (its premises, and that its
programs can observe the rules they are meant to hold, are asserted on the CPU by tests/test_session_model.py).

The feature suites download and compare after every call, and every download synchronises the context: a missing ordering edge between two mutating
calls enqueued back to back cannot show there.  Here the calls of a burst are the raw, asynchronous entry points, enqueued back to back; nothing is
downloaded and no blocking call is added between two checkpoints (resize, export, bake, release and info block by themselves and are part of a burst as
they come; what a bake or a frame left is read at the next checkpoint).  Checkpoints: `state` -- for every live renderer the native count, the four
blobs (tails included), DownloadPosOther, the three bit buffers, the nine info words and the order buffer, byte for byte against the model; `twin` -- a
fresh one-at-a-time renderer over an asset made of the downloaded blobs (the same asset where nothing is private) with the same bits, cutouts and
settings: order, view records and frames of three cameras bit for bit, and against the oracle within RT_TOL where no selection is drawn; `export` and
`bake` -- the rows / the five blobs and the bounds against export_model / the yardstick of bake_model over the model's state.

GSPLAT_SESSION_SEEDS=n adds n further seeds for a campaign; the suite keeps the eight."""
import contextlib
import ctypes as C
import os
import time

import numpy as np
import pytest

import bake_model as BM
import session_model as SM
from common import RT_TOL, rt_err
from gpu_rig import assert_same_frames, check_state, download, draw_frame, edit_info, fptr, frames_of, native_count, pinned_renderer as make_renderer, yardstick as cluster_yardstick
from unitygaussiansplatting_amd import _abi, _lib, creator
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuAsset, GpuContext, RenderTarget, SortMode

pytestmark = pytest.mark.gpu
f32 = np.float32
SEEDS = list(SM.SUITE_SEEDS) + [100 + k for k in range(int(os.environ.get("GSPLAT_SESSION_SEEDS", "0")))]


def ply_body(path) -> np.ndarray:
    """the records of an exported PLY as they stand in the file, all 62 columns (creator.ReadPLY drops the normals): [count, 62] float32"""
    with open(path, "rb") as f:
        data = f.read()
    head = data[:data.index(b"end_header\n") + len(b"end_header\n")]
    assert [ln.split()[2].decode() for ln in head.splitlines() if ln.startswith(b"property float ")] == list(creator.PLY_ATTRS)
    return np.frombuffer(data, "<f4", offset=len(head)).reshape(-1, len(creator.PLY_ATTRS))


class Run:
    """the renderers of one session, the model, and what is still to be read at the next checkpoint"""

    def __init__(self, ctx, seed, tmp_path):
        self.ctx, self.seed, self.tmp_path = ctx, seed, tmp_path
        self.cfg = SM.config(seed)
        self.s = SM.Session(seed)
        self.lib = _lib.lib()
        self.ctx2 = GpuContext(ctx.device) if self.cfg.ctx2 else None      # the source on a second context of the same GPU
        self.r = {}
        self.assets = []                                           # GpuAssets alive: baked and not yet compared, or under G
        self.g_asset = self.last_t_bake = None
        self.frames, self.bakes = [], []                           # pending: (target, want, step), (GpuAsset, model's bake, step)
        self.log, self.step = [], 0
        self.ply_done = False
        self.counts = dict(calls=0, bursts=0, state=0, twin=0, export=0, bake=0, refusals=0)

    def open(self):
        c = self.cfg
        self.r["T"] = make_renderer(self.ctx, SM.source_asset(300, "VeryHigh"), SM.DST_TR, c.mode, c.lanes)
        self.r["S"] = make_renderer(self.ctx2 or self.ctx, SM.source_asset(c.s_n, c.preset), SM.SRC_TR)

    def close(self):
        for rt, _, _ in self.frames:
            rt.Dispose()
        for r in self.r.values():
            r.DisposeResourcesForAsset()
        for g in self.assets:
            g.Dispose()
        if self.ctx2 is not None:
            self.ctx2.Dispose()

    def msg(self, what=""):
        return f"seed {self.seed} step {self.step} ({what}); ops: {self.log[-12:]}"

    @contextlib.contextmanager
    def where(self, what):
        """an assertion of a shared helper, with the seed, the step and the last 12 ops in front"""
        try:
            yield
        except AssertionError as e:
            raise AssertionError(f"{self.msg(what)}: {e}") from e

    # -- one call on the GPU: the raw entry point, its return code ---------------------------------------------------------------------------------
    def gpu(self, op, res_box):
        lib, name, a = self.lib, op.name, op.args
        r = self.r[op.who]
        h = r._r_h
        n = self.s.r[op.who].n                                     # (before the model applies the op)
        if name == "select_all":
            return lib.gs_renderer_edit_select_all(h)
        if name == "deselect_all":
            return lib.gs_renderer_edit_deselect_all(h)
        if name == "invert":
            return lib.gs_renderer_edit_invert_selection(h)
        if name == "store_sel":
            return lib.gs_renderer_edit_store_selection(h)
        if name == "update":
            P = r.FrameParams(SM.RECT_CAMS[a[0]])
            return lib.gs_renderer_edit_update_selection(h, C.byref(P), fptr(a[1:5])[1], int(a[5]))
        if name == "delete":
            return lib.gs_renderer_edit_delete_selected(h)
        if name == "set_deleted":
            r.SetDeletedBits(None if a[0] is None else SM.words_of(a[0], n, a[1]))
            return 0
        if name == "upload_sel":
            w = SM.words_of(a[0], n, a[1])
            return lib.gs_renderer_edit_upload_selected_bits(h, w.ctypes.data, len(w))
        if name == "set_cutouts":
            r.m_Cutouts = SM.EM.cutout_lists()[a[0]]
            r.UpdateCutoutsBuffer()
            return 0
        if name == "release":
            return lib.gs_renderer_edit_release(h)
        if name == "info":
            info = _abi.gs_edit_info()
            rc = lib.gs_renderer_edit_info(h, C.byref(info))
            res_box["info"] = SM.EM.info_words(info)
            return rc
        if name == "store_pos":
            return lib.gs_renderer_edit_store_pos_mouse_down(h)
        if name == "store_other":
            return lib.gs_renderer_edit_store_other_mouse_down(h)
        if name == "translate":
            return lib.gs_renderer_edit_translate_selection(h, fptr(a)[1])
        if name in ("rotate", "scale"):
            (_, c), (_, m0), (_, m1) = fptr(a[-3:]), fptr(SM.TOOL.localToWorldMatrix), fptr(SM.TOOL.worldToLocalMatrix)
            if name == "rotate":
                return lib.gs_renderer_edit_rotate_selection(h, c, m0, m1, fptr(a[:4])[1])
            return lib.gs_renderer_edit_scale_selection(h, c, m0, m1, fptr(a[:3])[1])
        if name == "resize":
            return self.resize(r, a[0])
        if name == "copy":
            dst = self.r["T"]
            p = r.CopyParams(dst)
            return lib.gs_renderer_edit_copy_splats_into(h, dst._r_h, C.byref(p), a[0], a[1], a[2])
        if name == "merge":                                        # MergeSplatObjects' two calls
            dst = self.r["T"]
            n0 = self.s.r["T"].n
            rc = self.resize(dst, n0 + n)
            p = r.CopyParams(dst)
            return rc or lib.gs_renderer_edit_copy_splats_into(h, dst._r_h, C.byref(p), 0, n0, n)
        if name == "sort_mode":
            r.SetSortMode(SortMode(a[0]))
            return 0
        if name == "lanes":
            r.SetFramesInFlight(a[0])
            return 0
        if name == "limit":
            r.SetSortHistoryLimit(a[0])
            return 0
        if name == "highlight":
            r.SetSelectionHighlight(bool(a[0]))
            return 0
        if name == "tile":
            r.SetTileShape(*a)
            return 0
        if name == "frame":
            cam = SM.CAMS[a[0]]
            rt = RenderTarget(r.ctx, cam.pixelWidth, cam.pixelHeight)
            draw_frame(r, cam, rt)
            res_box["rt"] = rt
            return 0
        if name == "export":
            if self.seed == 0 and not self.ply_done:               # one seed also takes the PLY route and reads the file back
                path = str(self.tmp_path / "session.ply")
                res_box["ply"] = (r.ExportPlyFile(path, bool(a[0])), creator.ReadPLY(path), ply_body(path))
                self.ply_done = True
            res_box["rows"] = r.ExportAlive(bool(a[0]))
            return 0
        if name == "export_all":
            res_box["rows"] = r.EditExportData(bool(a[0]))
            return 0
        if name in ("bake", "bake_cluster", "bake_refused"):
            if name == "bake":
                formats, morton = BM.FORMAT_TARGETS[a[0]], bool(a[1])
            elif name == "bake_cluster":
                formats, morton = SM.CLUSTER4K, bool(a[0])
            else:
                formats, morton = (SM.BC7_TARGET if a[0] == "bc7" else SM.CLUSTER4K), True
            fmt = r.BakeFormats(formatPos=formats[0], formatScale=formats[1], formatColor=formats[2], formatSH=formats[3], morton=morton)
            out, alive = C.c_void_p(0x1234), C.c_uint32(0)
            bmin, bmax = (C.c_float * 3)(), (C.c_float * 3)()
            rc = lib.gs_renderer_edit_bake_asset(h, C.byref(fmt), C.byref(out), C.byref(alive), bmin, bmax)
            if rc == 0:
                g = GpuAsset(r.ctx, out, alive.value, (fmt.pos_format, fmt.scale_format, fmt.color_format, fmt.sh_format), tuple(bmin), tuple(bmax))
                self.assets.append(g)
                res_box["asset"] = g
            else:
                res_box["out"] = out.value
            return rc
        if name == "make_g":
            return 0                                               # (made after the model: the renderer's host mirror is the model's asset)
        raise KeyError(name)

    def resize(self, r, n) -> int:
        rc = self.lib.gs_renderer_edit_set_splat_count(r._r_h, n, None)
        now = native_count(r)
        if rc == 0 and now != r.m_SplatCount:                      # what GaussianSplatRenderer.EditSetSplatCount keeps of the host mirror
            r.m_SplatCount, r.m_Resized = now, True
            r.m_GpuEditPosMouseDown = r.m_GpuEditOtherMouseDown = False
        return rc

    def make_g(self):
        """a renderer over the asset the last bake of T produced; an earlier G goes first"""
        if "G" in self.r:
            self.r.pop("G").DisposeResourcesForAsset()
        if self.g_asset is not None and self.g_asset is not self.last_t_bake and not any(g is self.g_asset for g, _, _ in self.bakes):
            self.assets.remove(self.g_asset)
            self.g_asset.Dispose()
        self.g_asset = self.last_t_bake
        g = GaussianSplatRenderer(self.ctx, None, SM.DST_TR)
        g.sortMode, g.framesInFlight = self.cfg.mode, 1
        g.CreateResourcesForGpuAsset(self.g_asset)
        g.m_Asset = self.s.r["G"].asset0                          # the host mirror: the model's yardstick, whose bytes the bake is held to at the checkpoint
        self.r["G"] = g

    # -- one op on both sides ----------------------------------------------------------------------------------------------------------------------
    def call(self, op):
        box = {}
        rc = self.gpu(op, box)
        res = self.s.apply(op, draw=True)
        self.counts["calls"] += 1
        assert rc == res.rc, self.msg(f"return code {rc}, the model's {res.rc}; {self.lib.gs_last_error_string()}")
        if op.name == "make_g":
            self.make_g()
        elif op.name == "info":
            want = self.s.r[op.who].tm.info()
            assert np.array_equal(box["info"], want), self.msg(f"info {box['info'].tolist()} != {want.tolist()}")
        elif op.name == "frame":
            self.frames.append((box["rt"], res.frame[1], self.step))
        elif op.name in ("export", "export_all"):
            self.counts["export"] += 1
            got, want = box["rows"], res.export
            assert got.shape == want.shape, self.msg(f"{got.shape[0]} rows exported, the model's {want.shape[0]}")
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), self.msg(f"exported rows differ at {np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:6].tolist()}")
            if "ply" in box:
                count, back, body = box["ply"]
                assert count == len(want) == len(back) and body.shape == want.shape, self.msg(f"the PLY holds {count} / {len(back)} / {len(body)} splats, the model's rows are {len(want)}")
                assert np.array_equal(body.view(np.uint32), want.view(np.uint32)), self.msg(f"the PLY's 62 columns differ at {np.argwhere(body.view(np.uint32) != want.view(np.uint32))[:6].tolist()}")
                cols = dict(pos=want[:, 0:3], dc0=want[:, 6:9], sh=want[:, 9:54].reshape(-1, 3, 15).transpose(0, 2, 1), opacity=want[:, 54], scale=want[:, 55:58], rot=want[:, 58:62])
                for name, w in cols.items():                      # what creator.ReadPLY makes of them (the normals it drops; sh: ReorderSHs)
                    g = np.ascontiguousarray(getattr(back, name), f32)
                    assert g.shape == w.shape and np.array_equal(g.view(np.uint32), np.ascontiguousarray(w, f32).view(np.uint32)), self.msg(f"the PLY read back: {name}")
        elif op.name in ("bake", "bake_cluster", "bake_refused"):
            if res.rc != 0:
                self.counts["refusals"] += 1
                assert not box["out"], self.msg("a refused bake left *out set")
            else:
                self.bakes.append((box["asset"], res.bake, self.step))
                if op.name == "bake" and op.who == "T":
                    self.last_t_bake = box["asset"]

    def settle(self):
        """what the burst left to be read: the frames drawn and the assets baked"""
        for rt, want, step in self.frames:
            img = rt.Download()
            rt.Dispose()
            if want is not None:
                e = rt_err(img, want[1])
                assert e <= RT_TOL, self.msg(f"the frame of step {step} against the oracle: {e}")
        self.frames = []
        for g, (dec_alive, formats, morton, cluster), step in self.bakes:
            self.counts["bake"] += 1
            want = cluster_yardstick(dec_alive, formats, morton) if cluster else BM.yardstick(dec_alive, formats, morton)
            assert g.splatCount == len(dec_alive), self.msg(f"the bake of step {step}: {g.splatCount} alive, the model's {len(dec_alive)}")
            with self.where(f"the bake of step {step}"):
                BM.assert_same_asset(g.Download(), want, step)
        kept = [g for g in self.assets if g is self.g_asset or g is self.last_t_bake]
        for g in self.assets:
            if not any(g is k for k in kept):
                g.Dispose()
        self.assets, self.bakes = kept, []

    def state(self):
        self.settle()
        self.counts["state"] += 1
        for who in self.s.live():
            r, st = self.r[who], self.s.r[who]
            sel, md, deleted = st.tm.bits()
            with self.where(f"state of {who}"):
                if st.very_high:
                    check_state(r, st.blobs(), who, st.tails(), selected=(sel, md), order=st.order)
                else:
                    assert native_count(r) == st.n == r.splatCount
                    a = st.asset()
                    for name, g, w in zip(("pos", "other", "color", "sh"), r.DownloadSplatData(), (a.posData, a.otherData, a.colorData, a.shData)):
                        assert np.array_equal(g, np.ascontiguousarray(w, np.uint8)), (name, "blob")
                    for name, g, w in zip(("selected", "mouse-down", "deleted"), r.DownloadEditBits(), (sel, md, deleted)):
                        assert np.array_equal(g, w), (name, np.flatnonzero(g != w)[:8])
                    assert np.array_equal(r.DownloadOrder(), st.order), "order"
                pos, other = r.DownloadPosOther()
                wp, wo = st.tm.blobs()
                assert SM.TM.blobs_equal(pos, wp, floats=st.tm.pos_gate) and SM.TM.blobs_equal(other, wo, floats=False), "DownloadPosOther"
                info = edit_info(r)
                assert np.array_equal(SM.EM.info_words(info), st.tm.info()), ("info", SM.EM.info_words(info).tolist(), st.tm.info().tolist())

    def twin(self, who):
        self.counts["twin"] += 1
        r, st = self.r[who], self.s.r[who]
        twin = None
        try:
            if who == "G":
                twin = GaussianSplatRenderer(self.ctx, None, st.tr)
                twin.sortMode = SortMode(st.settings["sort_mode"])
                twin.CreateResourcesForGpuAsset(self.g_asset)
                twin.m_Asset = st.asset0
            else:
                twin = make_renderer(self.ctx, download(r).asset() if st.very_high else st.asset0, st.tr, SortMode(st.settings["sort_mode"]))
            if st.tm.deleted is not None:
                twin.SetDeletedBits(st.tm.deleted)
            if st.tm.sel is not None:
                twin.UploadSelectedBits(st.tm.sel)
            twin.m_Cutouts = SM.EM.cutout_lists()[st.cut_name]
            twin.SetSelectionHighlight(bool(st.settings["highlight"]))
            if st.settings["limit"] is not None:
                twin.SetSortHistoryLimit(st.settings["limit"])
            twin.SetTileShape(*st.settings["tile"])
            twin.UploadOrder(st.order)                             # (the state checkpoint before this one held the renderer's order to the model's)
            plain = self.s.plain_frames(who)
            mine, theirs = frames_of(r, r.ctx, SM.CAMS), frames_of(twin, self.ctx, SM.CAMS)
            want = self.s.twin_frames(who, draw=plain)
            with self.where(f"twin of {who}"):
                assert_same_frames(mine, theirs, (who, "twin"))
                if plain:
                    assert_same_frames(mine, want, (who, "oracle"), bits=False)
                else:
                    assert np.array_equal(mine[1], want[1]), "order"
        finally:
            if twin is not None:
                twin.DisposeResourcesForAsset()


@pytest.mark.parametrize("seed", SEEDS)
def test_edit_sessions(gpu_ctx, seed, tmp_path):
    t0 = time.perf_counter()
    run = Run(gpu_ctx, seed, tmp_path)
    ops = SM.program(seed)
    try:
        run.open()
        in_burst = False
        for k, op in enumerate(ops):
            run.step = k
            run.log.append(str(op))
            assert len(run.r) <= 3
            if op.name == "state":
                run.state()
            elif op.name == "twin":
                run.twin(op.who)
            else:
                run.counts["bursts"] += int(not in_burst)
                run.call(op)
            in_burst = op.name not in SM.CHECKPOINTS
    finally:
        run.close()
    print(f"seed {seed}: {run.counts}, {time.perf_counter() - t0:.2f} s")
    assert seed != 0 or run.ply_done
    assert run.counts["state"] >= 10 and run.counts["twin"] >= 2 and run.counts["bake"] >= 2 and run.counts["export"] >= 1 and not run.frames and not run.bakes
