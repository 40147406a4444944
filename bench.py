#!/usr/bin/env python3
"""bench.py -- frames/s of the splat render hot path on MI355X (BASELINE.json metric).

One "step" = one frame of the reference's per-camera path for one GaussianSplatRenderer:
    SortPoints (CSCalcDistances + device radix sort)  ->  CalcViewData (CSCalcViewData)
    ->  clear RT  ->  draw all splats front-to-back  ->  composite (GaussianComposite)
on the configuration BASELINE.json quotes its metric on: bicycle-*sized* synthetic scene, 6,131,954 splats,
Medium asset (296 MB), 1200x797 (SURVEY.md section 8d "C2"; the real INRIA model is not available offline).
All inputs are resident in HBM before the timed region.  The camera orbits by 0.25 degrees per frame.

    python bench.py [--gpus N --steps K --warmup W] [--config C2] [--blend exact|fast] [--dump-outputs DIR] [--full] [--cpu-baseline auto|off] [--sort-mode both|full|visible]
(--config C2d: C2 with bicycle-like overdraw, ~18 tiles per visible splat -- a non-headline stress of the composite stage.)

A plain run does what the headline figure needs and nothing else: it builds the scene, uploads the asset, warms up W frames, times exactly K
frames of the headline mode (visible_in_flight, or --headline) in ONE region, and prints the result line (`ms_per_step` = that region / K).
--dump-outputs DIR then writes what the last timed step computed on rank 0 (bench_outputs/ is the conventional DIR; last_step_outputs).
--full adds everything below: every sort mode, five regions per mode (median), the per-stage and per-kernel timing passes, the roofline with
its rocprofv3 counters and the VALU probe, the copy ceiling, the GPU-internal cross-check, the oracle's end-of-orbit check and the CPU baseline.

Sort modes: `full` = SortPoints as the reference runs it (all N splats keyed and sorted every frame; SH only for visible splats, m_GpuView on
demand); `reference_shaped` = the same plus gs_renderer_set_view_buffer_mode(every_frame): the reference's whole per-frame work (sort all N,
CSCalcViewData's colour + 40-byte record for every splat in front of the camera); `visible` = GS_SORT_VISIBLE, cull first and sort the splats
that are drawn (same frame, same order among the drawn splats: include/gsplat_c.h).  With --full all of them are measured back to back over the
SAME frames; `modes` carries all, and the headline (`value`, `ms_per_step`, `config.sort_mode`) is the visible-only mode IF this run's end-of-orbit
check holds: at N = 1 the CPU oracle replays EVERY SortPoints of the whole measurement (warm-up + every timed and instrumented region: a stable
sort of all N per call, sequentially) and, on the last frame, the order the mode drew from must be the visible subsequence of the oracle's order
buffer, the library's consolidated buffer (gs_renderer_download_order) the oracle's whole buffer, and the frame within the framebuffer bar of the
oracle's; at N > 1 (no oracle) the consolidated buffer must equal the buffer the full mode built with its own sorts over the same frames and the
two frames must be the same bits.  Otherwise the headline is the full mode and the line says why.  --headline full|visible pins it.

Counters (--full): at N = 1 the run spawns three short children of itself (the headline mode, the same frames) under `rocprofv3 --pmc FETCH_SIZE`,
`--pmc WRITE_SIZE`, `--pmc SQ_INSTS_VALU` (separate passes), so `roofline.traffic` and `roofline.valu` are measured in THIS run on THIS box
(--pmc off skips them).

N > 1: view-parallel, one rank per GPU.  Launched either by the driver (python -m torch.distributed.run ... bench.py --gpus N:
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment) or bare (`python bench.py --gpus N`: the script re-executes
itself under torch.distributed.run on 127.0.0.1 and fails loudly if the box has fewer than N GPUs).  Rank 0 builds the
asset and uploads it; the five blobs are broadcast once with the library's own RCCL communicator (gs_comm_create /
gs_asset_broadcast: ncclBroadcast per blob over xGMI; the 128-byte unique id travels through torch.distributed); every
rank then renders its own camera (azimuth rank*45 deg) with no per-frame collective.  torch.distributed (backend
"nccl" = RCCL) provides the barriers and the max-over-ranks reduction of the timed region.
value = all ranks' splats*frames / max-over-ranks time.  --config C5: the C2 asset, 8 cameras at 1920x1080 dealt
round-robin to the ranks (view k -> rank k % N), a step = every rank renders each of its views once.

Prints ONE JSON line on rank 0 (see DESIGN.md "measurement" for the byte formulas behind `roofline`).
"""
from __future__ import annotations

import argparse
import ctypes as C
import gc
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md
HBM_ACHIEVABLE_GBS = 6300.0   # the same guide's measured float4-copy rate (79 % of the spec peak)
STEADY_S = 1.0                # a plain run: seconds of untimed passes over the timed frames before they are timed (steady_state)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="C2", choices=["C1", "C2", "C2d", "C3", "C4", "C5"])
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (debugging only; result is labelled)")
    ap.add_argument("--blend", default="exact", choices=["exact", "fast"])
    ap.add_argument("--cpu-baseline", default=None, choices=["auto", "off"], help="the oracle's end-of-orbit replay + the CPU baseline (default: auto with --full, else off)")
    ap.add_argument("--sort-nth-frame", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=None, help="the timed region (exactly --steps frames) is run this many times back to back; ms_per_step / value are the MEDIAN region "
                                                              "(default: 5 with --full, else 1)")
    ap.add_argument("--broadcast", action="store_true", help="go through gs_comm_create / gs_asset_broadcast even with one rank")
    ap.add_argument("--sort-mode", default=None, choices=["all", "both", "full", "visible", "reference_shaped", "visible_in_flight"],
                    help="which modes to measure (both = full + visible; default: all with --full, else the headline mode alone)")
    ap.add_argument("--headline", default="auto", choices=["auto", "full", "visible", "visible_in_flight", "reference_shaped"],
                    help="which measured mode `value` reports (auto: the fastest of visible_in_flight / visible whose end-of-orbit check holds, else full)")
    ap.add_argument("--in-flight", type=int, default=2, help="renderers (contexts = streams) the visible_in_flight mode deals its frames / views to")
    ap.add_argument("--in-flight-impl", default="library", choices=["library", "host"],
                    help="library: ONE renderer on one context, gs_renderer_set_frames_in_flight deals the frames to lanes inside the library (the reference's calls unchanged); "
                         "host: the host holds --in-flight renderers on contexts of their own over one asset and deals the frames itself")
    ap.add_argument("--in-flight-targets", type=int, default=1, help="library lanes: sets of targets the host draws into in rotation (1: every frame into the same target, as the "
                                                                         "sequential modes do -- the library double-buffers a target's pixels itself while it has lanes)")
    ap.add_argument("--pmc", default=None, choices=["auto", "off"], help="auto: at N = 1 spawn rocprofv3 --pmc children of this script for HBM traffic and VALU instruction counts "
                                                                        "(default: auto with --full, else off)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline figure: every sort mode, the per-stage / per-kernel timing passes, the roofline and its "
                                                        "counters, the copy ceiling, the GPU-internal cross-check, the oracle's end-of-orbit check and the CPU baseline")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write what the headline mode's last step computed to DIR/<name>.npy "
                                                                       "(float32 / float64, at most 64 MB in all; larger outputs as a fixed, seeded sample)")
    ap.add_argument("--pmc-child", default="", help="(internal) path of the pickled asset: run the frames of one mode and exit -- what the rocprofv3 children execute")
    ap.add_argument("--child-mode", default="visible", help="(internal) mode of a --pmc-child run")
    ap.add_argument("--child-first", type=int, default=0, help="(internal) first frame of the timed region of a --pmc-child run")
    ap.add_argument("--dry-run", action="store_true", help="no GPU work: the rank / view / reduction logic and the JSON schema only (CPU test of the N > 1 path, gloo)")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    if args.cpu_baseline is None:
        args.cpu_baseline = "auto" if args.full else "off"
    if args.pmc is None:
        args.pmc = "auto" if args.full else "off"
    if args.sort_mode is None:
        args.sort_mode = "all" if args.full else ("visible_in_flight" if args.headline == "auto" else args.headline)
    return args


def stage_bytes(n, P, vis, W, H, asset, passes_pair, mode="full", tie_fix=True, depth_passes=4):
    """ALGORITHMIC bytes per launch of each stage (DESIGN.md "measurement"): the compulsory
    traffic of the algorithm as shipped, every buffer counted once per pass over it."""
    from unitygaussiansplatting_amd.asset import GetVectorSize, GetOtherSizeNoSHIndex, GetColorSize
    b_pos = GetVectorSize(asset.posFormat)
    sh_item = {0: 192, 1: 96, 2: 60, 3: 32}.get(int(asset.shFormat), 96)
    chunk = 64.0 / 256.0 if asset.chunkCount else 0.0
    b_asset = b_pos + GetOtherSizeNoSHIndex(asset.scaleFormat) + GetColorSize(asset.colorFormat) + sh_item + chunk
    out = {
        # pos/rot/scale/colour/chunk of every splat in, 8-B tile rect + 1 visibility bit out; the SH record is read and the
        # 32-B blend record written only for splats that reach the screen (the 40-B m_GpuView record is materialised on demand)
        "calc_view": n * (b_asset - sh_item + 8 + 0.125 + 1.0 / 64) + vis * (sh_item + 32),   # (+ 1 flag byte per wave of 64 splats for the binning)
        "pair_sort": P * 16 * passes_pair + P * 4,               # Onesweep passes over the pairs + tile-range scan of the keys
        "blend": P * (4 + 32) + W * H * 8,                       # pair index + record per pair, RT write (a cleared target is not read: the blend writes every pixel)
        "resolve": W * H * (8 + 16),                             # RGBA16F in, float RGBA out (the 8-bit sRGB image is written only on request)
    }
    if mode == "full":
        out["calc_distances"] = n * (b_pos + chunk + 4)          # CSCalcDistances' arithmetic in index order: pos in, key out (+ the digit histograms)
        out["sort"] = n * (16 * 4 - 4)                           # 4 Onesweep passes x 16 B/key (the first reads prev order + gathered key instead of key + payload;
                                                                 # the last writes only the order: the sorted keys are materialised on demand)
        out["bin"] = n * (4 + 1.0 / 64) + vis * 8 + P * 8        # order + the wave's visibility byte per position, rect per visible splat, (tile, splat) pairs out
    else:
        # GS_SORT_VISIBLE: only the V visible splats are keyed, sorted and binned
        out["calc_distances"] = n / 8.0 + vis * (b_pos + chunk + 8)     # visibility bits of all N; position in, (key, index) out per visible splat
        out["sort"] = vis * 16 * depth_passes + (vis * 4 if tie_fix else 0)       # 3 or 4 plain passes x 16 B/key over V (+ the fix-up's pass over the sorted keys)
        # vis_count: order + the rectangle gather in, rectangle + local offset by position out; vis_offsets: offsets in / out; vis_emit: offset, index,
        # rectangle in, (tile, splat) pairs out
        out["bin"] = vis * (4 + 8 + 12) + vis * 8 + vis * 16 + P * 8
    return out


def respawn_under_torchrun(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: run N ranks of this script under torch.distributed.run on this node."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


# VALU issue roofs, G wave-instructions / s, whole chip.  SPEC: 256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles per wave64 fp32 instruction (the guide's
# issue rate) = the 157.3 TFLOP/s fp32 vector peak / 128 flops per wave-level FMA.  MEASURED: plain v_fma_f32 streams, 8 waves per SIMD, on this
# part under its own power management (scripts/probes/valu_issue.hip; the bench runs the probe itself when the binary is there, else the stored figure).
VALU_SPEC_GWI = 256 * 4 * 2.4 / 2.0
VALU_MEASURED_GWI_STORED = 687.0          # profiles/r05_valu_issue.txt


def run_valu_probe():
    """scripts/probes/valu_issue --quick: the sustained plain-VALU issue rate of THIS box (one JSON line), or None."""
    import subprocess
    exe = os.path.join(ROOT, "scripts", "probes", "valu_issue")
    if not os.path.exists(exe):
        return None
    try:
        out = subprocess.run([exe, "--quick"], capture_output=True, text=True, timeout=60).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                return json.loads(line)
    except Exception:
        return None
    return None


def short_kernel(name):
    import re
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    name = re.sub(r"\(.*", "", name).replace("gs::", "")
    return re.sub(r"<.*", "", name)


def fold_counter_rows(kernels, rows, counter, frames_total, steps):
    """rows: rocprofv3's *_counter_collection.csv records of ONE --pmc pass (one per dispatch).  Per kernel (template arguments folded), the mean over
    the dispatches of the LAST `steps` frames of the `frames_total` the child ran -- its timed region, not its warm-up -- into kernels[name]."""
    per = {}
    for r_ in rows:
        if r_.get("Counter_Name", counter) != counter:
            continue
        per.setdefault(short_kernel(r_["Kernel_Name"]), []).append((int(r_.get("Dispatch_Id", 0) or 0), float(r_["Counter_Value"])))
    for k, v in per.items():
        v.sort()
        per_frame = max(1, round(len(v) / frames_total))
        tail = [x[1] for x in v[-min(len(v), per_frame * steps):]]
        e = kernels.setdefault(k, {})
        e[counter if counter == "SQ_INSTS_VALU" else counter + "_KiB"] = sum(tail) / len(tail)
        e["dispatches"] = len(tail)
    return kernels


def pmc_children(args, asset, mode, first, frames_warm):
    """HBM traffic and VALU instruction counts of the run's own frames: three children of this script (--pmc-child: no torch, the asset handed over
    through /dev/shm, `mode`, the same warm-up and the same K frames) under rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE / SQ_INSTS_VALU -- separate passes
    with --kernel-trace only, as the guide prescribes.  Returns {"kernels": {base name: {"FETCH_SIZE_KiB", "WRITE_SIZE_KiB", "SQ_INSTS_VALU", "dispatches"}}, ...}:
    per-launch means over the dispatches of the last K frames."""
    import csv, glob, pickle, shutil, subprocess, tempfile
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return {"kernels": {}, "error": "rocprofv3 not found"}
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    apath = os.path.join(shm, f"gsplat_bench_asset_{os.getpid()}.pkl")
    out_root = tempfile.mkdtemp(prefix="gs_pmc_", dir="/tmp")
    res = {"kernels": {}, "passes": {}, "mode": mode}
    t0 = time.perf_counter()
    try:
        with open(apath, "wb") as f:
            pickle.dump(asset, f, protocol=pickle.HIGHEST_PROTOCOL)
        env = dict(os.environ, TMPDIR="/tmp", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        child = [sys.executable, os.path.abspath(__file__), "--pmc-child", apath, "--child-mode", mode, "--child-first", str(first), "--config", args.config,
                 "--steps", str(args.steps), "--warmup", str(frames_warm), "--blend", args.blend, "--sort-nth-frame", str(args.sort_nth_frame)] + \
                (["--splats", str(args.splats)] if args.splats else [])
        for counter in ("FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU"):
            d = os.path.join(out_root, counter)
            tp = time.perf_counter()
            pr = subprocess.run([rocprof, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "--"] + child, cwd="/tmp", env=env,
                                capture_output=True, text=True, timeout=120)
            rows = []
            for fcsv in glob.glob(os.path.join(d, "*", "*_counter_collection.csv")):
                rows += list(csv.DictReader(open(fcsv)))
            res["passes"][counter] = {"rc": pr.returncode, "dispatch_rows": len(rows), "seconds": round(time.perf_counter() - tp, 1)}
            if pr.returncode != 0 or not rows:
                res["passes"][counter]["stderr_tail"] = (pr.stderr or "")[-300:]
                continue
            fold_counter_rows(res["kernels"], rows, counter, frames_warm + args.steps, args.steps)
    except Exception as ex:                                  # counters are evidence, not the product: never fail the bench line over them
        res["error"] = f"{type(ex).__name__}: {ex}"
    finally:
        try:
            os.remove(apath)
        except OSError:
            pass
        shutil.rmtree(out_root, ignore_errors=True)
    res["seconds"] = round(time.perf_counter() - t0, 1)
    return res


def pmc_child_main(args):
    """What the rocprofv3 children run: the library only (no torch), `--child-mode` frames: the warm-up of measure() and then the K frames of its timed region, once."""
    import pickle
    from unitygaussiansplatting_amd import camera, scenes
    from unitygaussiansplatting_amd import _lib
    from unitygaussiansplatting_amd._lib import GsError, check
    from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext, RenderTarget, SortMode
    with open(args.pmc_child, "rb") as f:
        asset = pickle.load(f)
    cfg = scenes.CONFIGS[args.config]
    ctx = GpuContext(0)
    r = GaussianSplatRenderer(ctx, asset)
    r.m_SortNthFrame = args.sort_nth_frame
    r.CreateResourcesForAsset()
    r.blendMode = 0 if args.blend == "exact" else 1
    check(_lib.lib().gs_renderer_set_blend_mode(r._r_h, int(r.blendMode)), "gs_renderer_set_blend_mode")
    W, H = cfg.width, cfg.height
    rt = RenderTarget(ctx, W, H)
    bg = np.asarray((0.0, 0.0, 0.0, 1.0), np.float32)
    bgp = bg.ctypes.data_as(C.POINTER(C.c_float))
    views = list(range(8)) if args.config == "C5" else [0]

    def frame(i):
        for v in views:
            cam = camera.Camera(position=scenes.orbit_eye(cfg.eye_radius, cfg.eye_elev_deg, v * 45.0 + 0.25 * i), pixelWidth=W, pixelHeight=H, fieldOfView=cfg.fov_y)
            if i % r.m_SortNthFrame == 0:
                r.SortPointsPrepared(r.SortMatrix(cam))
            p = r.FrameParams(cam)
            r.CalcViewDataPrepared(p)
            rt.Clear()
            r.DrawPrepared(p, rt)
            check(_lib.lib().gs_target_resolve(rt._h, bgp, None, None), "gs_target_resolve")

    r.ResetOrder()
    r.SetSortMode(SortMode.Visible if args.child_mode == "visible" else SortMode.Full)
    r.SetViewBufferMode(args.child_mode == "reference_shaped")
    for i in range(max(args.warmup, 1)):
        frame(i)
        try:
            r.FrameStats()
        except GsError as e:
            if e.code != -6:
                raise
            frame(i)
            r.FrameStats()
    st = r.FrameStats()
    r.ReservePairs(int(st.tile_pairs * 1.5) + (1 << 20))
    for k in range(args.steps):
        frame(args.child_first + k)
    ctx.Synchronize()
    r.FrameStats()
    print(json.dumps({"pmc_child": args.child_mode, "frames": max(args.warmup, 1) + args.steps, "tile_pairs_P": int(r.FrameStats().tile_pairs)}), flush=True)


def dry_run(args, rank, world):
    """--dry-run: the N > 1 control flow without a GPU -- gloo group, view assignment, max-over-ranks reduction, per-rank gather, the JSON
    line's schema -- so that a CPU test can hold bench.py's multi-rank path (tests/test_parallel.py)."""
    import torch
    import torch.distributed as dist
    from unitygaussiansplatting_amd import parallel, scenes
    cfg = scenes.CONFIGS[args.config]
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    num_views = 8 if args.config == "C5" else world
    my_views = parallel.assign_views(num_views, world)[rank]
    el = 1e-3 * (1 + rank) * args.steps                       # a pretend region: rank k takes (1 + k) ms per step
    t = torch.tensor([el], dtype=torch.float64)
    per_rank = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
    views = [None] * world
    if world > 1:
        dist.barrier()
        dist.all_gather(per_rank, t)
        dist.all_gather_object(views, my_views)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    else:
        per_rank, views = [t.clone()], [my_views]
    if rank == 0:
        n = args.splats or cfg.n
        print(json.dumps({"metric": f"Msplats/s rendered (sort+view+composite+resolve), {cfg.label}; ms/frame in ms_per_step", "dry_run": True,
                          "value": round(n * args.steps * num_views / float(t.item()) / 1e6, 2), "unit": "Msplats/s", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": round(float(t.item()) / args.steps * 1e3, 4),
                          "ms_per_step_per_rank": [round(float(x.item()) / args.steps * 1e3, 4) for x in per_rank], "views_per_rank": views,
                          "higher_is_better": True, "scaling": "strong" if args.config == "C5" else "weak", "vs_baseline": None, "dtype": "f32",
                          "data": "synthetic", "config": {"workload": cfg.label, "views": num_views, "rccl_ranks": 0, "host_group": "gloo"},
                          "modes": None, "end_of_orbit_check": None, "roofline": None, "roofline_blend": None, "roofline_streaming": None, "cpu_baseline": None}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    args = parse()
    if args.pmc_child:
        return pmc_child_main(args)
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(respawn_under_torchrun(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world > 1:
            args.gpus = world
        else:
            raise SystemExit(f"bench.py --gpus {args.gpus}: WORLD_SIZE is {world}; launch {args.gpus} ranks (or run it bare, it spawns them itself)")
    if args.dry_run:
        return dry_run(args, rank, world)

    # torch is plumbing here (barrier, the max-over-ranks reduction, moving the 128-byte RCCL id); its first import on a
    # fresh box takes a minute or two, so it is overlapped with building the synthetic scene.
    holder = {}

    def _imp():
        import torch
        holder["torch"] = torch
    th = threading.Thread(target=_imp)
    th.start()

    from unitygaussiansplatting_amd import camera, creator, scenes
    from unitygaussiansplatting_amd import _lib
    from unitygaussiansplatting_amd._lib import GsError, check
    from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext, RenderTarget, SortMode

    cfg = scenes.CONFIGS[args.config]
    t_build = time.perf_counter()
    asset = None
    if rank == 0:
        raw = scenes.make_config_splats(cfg, args.splats)
        asset = creator.CreateAssetFromSplatsNative(raw, cfg.quality, name=cfg.key)      # gs_import_encode: same bytes as the numpy importer, ~8x faster
        del raw
    th.join()
    torch = holder["torch"]
    t_build = time.perf_counter() - t_build
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    if torch.cuda.device_count() < world or local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py --gpus {world}: this box exposes {torch.cuda.device_count()} GPU(s); refusing to report a multi-GPU number")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        # The host-side group is GLOO: it carries the barriers, the max-over-ranks reduction and the 128-byte RCCL id.  The ONE RCCL
        # communicator of the process is the library's own (gs_comm_create: ncclCommInitRank), so RCCL sees exactly `world` ranks once.
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)

    # ---- asset residency: rank 0 uploads the blobs (gs_asset_create); with N > 1 they are broadcast once through the
    #      library's own RCCL communicator (gs_comm_create + gs_asset_broadcast; only the unique id goes through torch) ----
    from unitygaussiansplatting_amd import parallel
    ctx = GpuContext(local_rank)
    r = GaussianSplatRenderer(ctx, asset)
    r.m_SortNthFrame = args.sort_nth_frame
    t0 = time.perf_counter()
    comm = None
    rccl_ranks = 0
    if world > 1 or args.broadcast:
        uid = [parallel.Comm.UniqueId() if rank == 0 else None]
        if dist is not None:
            dist.broadcast_object_list(uid, src=0)
        comm = parallel.Comm(ctx, world, rank, uid[0])
        comm.BroadcastAsset(r, root=0)                 # gs_asset_create on rank 0, ncclBroadcast per blob, gs_renderer_create everywhere
        nr, rk = C.c_int32(), C.c_int32()
        check(_lib.lib().gs_comm_info(comm._h, C.byref(nr), C.byref(rk)), "gs_comm_info")      # what the communicator itself says
        rccl_ranks = int(nr.value)
    else:
        r.CreateResourcesForAsset()
    ctx.Synchronize()
    t_bcast = time.perf_counter() - t0
    r.blendMode = 0 if args.blend == "exact" else 1
    W, H = cfg.width, cfg.height
    n = r.splatCount
    asset_bytes = sum(int(len(getattr(r.m_Asset, nm))) for nm in parallel.BLOB_NAMES if getattr(r.m_Asset, nm) is not None) if rank == 0 else 0

    # views of this rank: one camera per rank (azimuth rank*45 deg), or C5's 8 cameras dealt round-robin
    num_views = 8 if args.config == "C5" else world
    my_views = parallel.assign_views(num_views, world)[rank]
    rts = [RenderTarget(ctx, W, H) for _ in my_views]
    rt = rts[0]

    def cam_at(frame, view=None):
        az = (my_views[0] if view is None else view) * 45.0 + 0.25 * frame
        return camera.Camera(position=scenes.orbit_eye(cfg.eye_radius, cfg.eye_elev_deg, az), pixelWidth=W, pixelHeight=H,
                             fieldOfView=cfg.fov_y)

    # Per-camera constants (the sort matrix and gs_frame_params) are built before the loops, as a host engine has them from
    # its camera; the loop body is the five C-ABI calls of one frame.  (Building them in numpy costs ~0.5 ms per frame,
    # which would make this Python harness, not the GPU, the bottleneck.)
    total_frames = max(args.warmup, 1) + args.steps + 2
    prepared = []
    for i in range(total_frames):
        per_view = []
        for v in my_views:
            cam = cam_at(i, v)
            per_view.append((r.SortMatrix(cam), r.FrameParams(cam)))
        prepared.append(per_view)
    r.UpdateCutoutsBuffer()
    check(_lib.lib().gs_renderer_set_blend_mode(r._r_h, int(r.blendMode)), "gs_renderer_set_blend_mode")
    bg = np.asarray((0.0, 0.0, 0.0, 1.0), np.float32)
    bgp = bg.ctypes.data_as(C.POINTER(C.c_float))
    lib_ = _lib.lib()

    sort_log = []                                            # every SortPoints matrix of the measurement in progress, in call order (the oracle replays it)

    # A lane = a renderer on a context (= a HIP stream) of its own with its own targets; lane 0 is `r`.  The sequential modes use lane 0 only.  The
    # visible_in_flight mode deals its frames (C5: its views) round-robin to --in-flight lanes that SHARE the asset's device blobs: in GS_SORT_VISIBLE
    # gs_renderer_sort is bookkeeping, so every lane is told every matrix and each draws its frames from the reference's order -- the same frames, one
    # lane's streaming / latency-bound kernels under another's VALU-bound blend.
    class Lane:
        def __init__(self, ctx_, r_, rts_):
            self.ctx, self.r, self.rts = ctx_, r_, rts_
            self.rt_sets, self.last_rt = None, rts_[-1]
    lanes = [Lane(ctx, r, rts)]
    active = [lanes[0]]

    def lane(k):
        while len(lanes) <= k:
            c2 = GpuContext(local_rank)
            r2 = GaussianSplatRenderer(c2, r.m_Asset)
            r2.m_SortNthFrame = r.m_SortNthFrame
            r2.sortMode = SortMode.Visible
            r2.ShareResourcesOf(r)
            r2.blendMode = r.blendMode
            r2.UpdateCutoutsBuffer()
            check(_lib.lib().gs_renderer_set_blend_mode(r2._r_h, int(r2.blendMode)), "gs_renderer_set_blend_mode")
            lanes.append(Lane(c2, r2, [RenderTarget(c2, W, H) for _ in my_views]))
        return lanes[k]

    def frame(i, cam=None):
        nl = len(active)
        for vi, (m16, p) in enumerate(prepared[i]):
            if i % r.m_SortNthFrame == 0:
                for X in active:
                    X.r.SortPointsPrepared(m16)
                sort_log.append(m16)
            X = active[(i * len(my_views) + vi) % nl]
            # (lanes inside the library, --in-flight-targets > 1: the host alternates sets of targets, a swap chain)
            t = (X.rt_sets[(i * len(my_views) + vi) % len(X.rt_sets)] if X.rt_sets else X.rts)[vi]
            X.last_rt = t
            X.r.CalcViewDataPrepared(p)
            t.Clear()
            X.r.DrawPrepared(p, t)
            check(lib_.gs_target_resolve(t._h, bgp, None, None), "gs_target_resolve")

    def sync_lanes():
        for X in active:
            X.ctx.Synchronize()

    def full_sync():
        sync_lanes()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    # ---- timed region: exactly K frames, nothing but the frame's C-ABI calls between the barriers ----------------
    per_rank_s = []

    def run_region(first, gather=False):
        full_sync()
        t0 = time.perf_counter()
        for k in range(args.steps):
            frame(first + k)
        sync_lanes()                                        # every kernel of the region (the contexts' own streams)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el = time.perf_counter() - t0
        if dist is not None:
            tmax = torch.tensor([el], dtype=torch.float64)
            if gather:
                parts = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
                dist.all_gather(parts, tmax)
                per_rank_s[:] = [float(x.item()) for x in parts]
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            el = float(tmax.item())
        return el

    # a device-to-device copy ceiling measured on this GPU BEFORE the timed regions (SURVEY.md section 8d asks for it next to the 8 TB/s
    # spec; boxes differ by up to 8 %): 512 MiB read + 512 MiB written, 10 times
    copy_ceiling = None
    if rank == 0 and args.full:
        try:
            src = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            dst.copy_(src); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                dst.copy_(src)
            e1.record(); torch.cuda.synchronize()
            copy_ceiling = round(10 * 2 * src.numel() / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
            del src, dst
        except Exception:
            copy_ceiling = None

    frames_warm = max(args.warmup, 1)

    def steady_state(first):
        """A plain run's single timed region must not carry the ramp of a first pass over its frames (the freshly reserved pair buffers, the lanes'
        first overlap, the clocks): the timed frames first .. first+K-1, in order and pipelined as the timed region runs them, cycled untimed for
        STEADY_S seconds (a pair buffer that overflows here is grown here).  Nothing they compute changes: the order a sequence of sorts leaves
        depends only on the order of the LAST occurrences of its distinct matrices (a stable sort through the previous order; GS_SORT_VISIBLE keeps
        exactly that chain), and the timed pass repeats every one of them last."""
        full_sync()
        logged = len(sort_log)                               # (these sorts change nothing the oracle's replay would see: not logged)
        t0 = time.perf_counter()
        k = 0
        while True:
            frame(first + k % args.steps)
            k += 1
            if k % 16 == 0:
                sync_lanes()
                if time.perf_counter() - t0 >= STEADY_S:
                    break
        del sort_log[logged:]
        for X in active:
            try:
                X.r.FrameStats()
            except GsError as e:
                if e.code != -6:                             # (-6: the last of these frames overflowed; the buffer has been grown)
                    raise

    def measure(mode, repeats, instrument=True):
        """One mode: warm-up (sizes the pair buffer: an overflowing frame grows it and is re-run), `repeats` un-instrumented regions of
        exactly K frames, then (--full only) the same K frames with the per-stage hipEvents, then once more with the Onesweep launches' own timestamps.
        Afterwards the renderer is left as the last frame left it (the end-of-orbit state the checks read)."""
        lean = not args.full                                 # a plain run: the warm-up and the timed regions, nothing else
        piped = mode == "visible_in_flight"
        lib_lanes = piped and args.in_flight_impl == "library"
        active[:] = [lane(k) for k in range(max(1, args.in_flight))] if (piped and not lib_lanes) else [lanes[0]]
        r.SetFramesInFlight(max(1, args.in_flight) if lib_lanes else 1)      # the lanes live inside the library, behind r
        if lib_lanes and args.in_flight_targets > 1 and lanes[0].rt_sets is None:
            lanes[0].rt_sets = [rts] + [[RenderTarget(ctx, W, H) for _ in my_views] for _ in range(args.in_flight_targets - 1)]
        if not lib_lanes and lanes[0].rt_sets is not None:
            lanes[0].rt_sets = None
        for X in active:
            X.r.SetSortMode(SortMode.Full)
            X.r.ResetOrder()                                 # every mode starts from CSSetIndices' order
            X.r.SetSortMode(SortMode.Visible if mode in ("visible", "visible_in_flight") else SortMode.Full)
        r.SetViewBufferMode(mode == "reference_shaped")     # the reference's CSCalcViewData: colour + 40-byte record of every splat in front of the camera, every frame
        del sort_log[:]
        fi = 0
        first_frame_ms = first_again_ms = None
        for _ in range(frames_warm):
            if fi == 0 and not lean:          # the very first frame (identity order: keys in Morton order, cold buffers), timed on its own
                sync_lanes()
                t_first = time.perf_counter()
            frame(fi)
            if fi == 0 and not lean:
                sync_lanes()
                first_frame_ms = (time.perf_counter() - t_first) * 1e3
                # ... and the same frame once more (same matrix: the sort changes nothing, the history does not grow): what is left of the
                # "first frame" once the code objects are loaded, the pair buffer sized and every buffer touched
                t_first = time.perf_counter()
                frame(fi)
                sync_lanes()
                first_again_ms = (time.perf_counter() - t_first) * 1e3
            for X in active:
                try:
                    X.r.FrameStats()
                except GsError as e:
                    if e.code != -6:
                        raise
                    frame(fi)
                    X.r.FrameStats()
            fi += 1
        # the orbit over the timed region may need more pairs than the warm-up saw: leave 50 % headroom
        st = r.FrameStats()
        for X in active:
            X.r.ReservePairs(int(st.tile_pairs * 1.5) + (1 << 20))
        if lean:
            steady_state(fi)
        # The un-instrumented region -- exactly K frames between barrier + synchronize -- is run `repeats` times back to back over the same
        # frames; ms_per_step and value are the MEDIAN region's (min / max / every region reported next to them): one 14 ms region alone is a
        # coin-flip inside +-4 % on these boxes.
        # Python's cyclic collector is off while frames are timed (as timeit does): with torch imported a full collection walks a few hundred
        # thousand objects -- tens of milliseconds -- and when it strikes at the head of a region, while the queue is still empty, the GPU waits
        # for the host (measured: the fifth 50-frame region of C2 / C3 took 10-40 ms longer in five of six runs; profiles/r04_bench_regions_c2.json).
        gc.collect()
        gc.disable()
        regions = [run_region(fi, gather=True) for _ in range(max(repeats, 1))]
        per_rank = list(per_rank_s)
        if piped or lean:                                    # frames in flight side by side: per-kernel brackets mean nothing; the sequential visible mode has them
            if not lean:
                run_region(fi); run_region(fi)               # (the two instrumented passes of the other modes, as plain regions: every mode logs the SAME sequence of sorts)
            gc.enable()
            for X in active:
                X.r.FrameStats()
            # the lane that drew the orbit's last frame (view) holds the end-of-orbit state
            last_lane = active[((fi + args.steps - 1) * len(my_views) + len(my_views) - 1) % len(active)]
            rows, limit, cons = last_lane.r.SortHistory()
            return dict(mode=mode, fi=fi, regions=regions, per_rank=per_rank, elapsed=float(np.median(regions)), elapsed_instr=None, resolve_ms=None, st=last_lane.r.FrameStats(),
                        frame_ms=None, stage=None, stage_k=None, first_frame_ms=first_frame_ms, first_again_ms=first_again_ms, sorts=list(sort_log),
                        history=dict(rows=int(rows), limit=int(limit), consolidations=int(cons)), lane=last_lane, lanes=(max(1, args.in_flight) if lib_lanes else len(active)),
                        impl=(("library" if lib_lanes else "host") if piped else None))
        # ---- the same K frames again with the per-stage hipEvents recorded (14 per frame, on the stream each kernel is
        #      launched on).  The events themselves cost ~50 us of a 0.6 ms frame (every record is a barrier + signal packet
        #      between two kernels), so the headline time comes from the regions above and the per-kernel durations from this one.
        r.SetProfiling(min((args.steps + 1) * len(my_views), 1024))       # a ring: one spare slot so that the first frame's events are not recycled
        rt.SetProfiling(True)                           # the composite is a target method: its own event pairs on the same stream
        elapsed_instr = run_region(fi)
        resolve_ms, _ = rt.ResolveTime()
        rt.SetProfiling(False)
        st = r.FrameStats()                   # raises if the last frame overflowed / a sort spin expired
        frame_ms = r.FrameTimes()             # per-frame GPU durations of the instrumented pass
        stage = r.StageTimes()
        stage_k = stage
        if instrument:
            # ---- and a third pass in which every Onesweep launch carries its OWN start / stop timestamps (hipExtLaunchKernelGGL events = the
            #      dispatch packet's completion signal, what rocprofv3 --kernel-trace reports): the streaming kernel's launch duration without
            #      kernel boundaries or event packets.  A pass of its own because the timestamped launches perturb the stage brackets.
            r.SetProfiling(min((args.steps + 1) * len(my_views), 1024))
            r.SetKernelTiming(True)
            run_region(fi)
            r.FrameStats()
            stage_k = r.StageTimes()
            r.SetKernelTiming(False)
        gc.enable()
        r.SetProfiling(0)
        rows, limit, cons = r.SortHistory()
        return dict(mode=mode, fi=fi, regions=regions, per_rank=per_rank, elapsed=float(np.median(regions)), elapsed_instr=elapsed_instr, resolve_ms=resolve_ms, st=st,
                    frame_ms=frame_ms, stage=stage, stage_k=stage_k, first_frame_ms=first_frame_ms, first_again_ms=first_again_ms, sorts=list(sort_log),
                    history=dict(rows=int(rows), limit=int(limit), consolidations=int(cons)))

    def end_state(x):
        """What the mode's last frame left: the target, the order buffer the reference would hold (GS_SORT_VISIBLE: the recorded sorts carried out on
        all N by the library), and in the visible-only modes the order the frame was drawn from."""
        L = x.get("lane", lanes[0])
        x["img"] = L.last_rt.Download()
        if x["mode"] in ("visible", "visible_in_flight"):
            x["vis_order"] = L.r.DownloadVisibleOrder()
            x["vis_stats"] = L.r.FrameStats()
        x["order"] = L.r.DownloadOrder()
        if args.dump_outputs and rank == 0:
            x["outputs"] = last_step_outputs(x)

    def last_step_outputs(x):
        """--dump-outputs: what the mode's last step handed its caller -- per view the splat target (RGBA16F, as float32) and its composite onto the
        bench's background (linear RGBA float32), the order the last frame was drawn from and the order buffer (seeded samples), the frame's tile
        pairs and visible splats.  Read after the timed steps; within DUMP_BYTES (cap_outputs)."""
        i = x["fi"] + args.steps - 1
        out = {}
        for vi, v in enumerate(my_views):
            X = active[(i * len(my_views) + vi) % len(active)]          # the target frame() drew this view of the last step into
            t = (X.rt_sets[(i * len(my_views) + vi) % len(X.rt_sets)] if X.rt_sets else X.rts)[vi]
            sfx = "" if len(my_views) == 1 else f"_view{v}"
            out["framebuffer" + sfx] = t.Download().view(np.float16).astype(np.float32)
            out["resolved" + sfx] = t.Resolve(tuple(float(c) for c in bg), want8=False)[0]
        if "vis_order" in x:
            out["visible_order"] = seeded_sample(x["vis_order"], DUMP_ORDER_SAMPLE, "visible_order").astype(np.float64)
        out["order"] = seeded_sample(x["order"], DUMP_ORDER_SAMPLE, "order").astype(np.float64)
        out["frame_stats"] = np.asarray([x["st"].tile_pairs, x["st"].visible_splats], np.float64)
        return cap_outputs(out)

    modes = {"all": ["full", "reference_shaped", "visible", "visible_in_flight"], "both": ["full", "visible"]}.get(args.sort_mode, [args.sort_mode])
    if args.full and "visible_in_flight" in modes and "visible" not in modes:
        modes.insert(modes.index("visible_in_flight"), "visible")                  # the per-kernel figures come from one frame at a time
    res = {}
    for m in modes:
        res[m] = measure(m, args.repeats if m != "reference_shaped" else min(args.repeats, 3), instrument=(m != "reference_shaped"))
        if args.full or args.dump_outputs or args.cpu_baseline == "auto":
            end_state(res[m])
    active[:] = [lanes[0]]
    r.SetFramesInFlight(1)
    r.SetViewBufferMode(False)

    # ---- GPU-internal end-of-orbit cross-check: the visible-only mode and the full mode ran the SAME sequence of SortPoints (warm-up + every region);
    #      the full mode carried every one of them out as a real stable sort of all N, the visible-only mode recorded them and carried them out on
    #      demand (consolidation: one sort + the chain fix-up) -- two independent code paths that must end in the same order buffer, and in the same frame
    cross = None
    if args.full and "visible" in res and "full" in res:
        V_, F_ = res["visible"], res["full"]
        same_log = same_sorts(V_["sorts"], F_["sorts"])
        gmask = np.zeros(n, bool)
        gmask[V_["vis_order"]] = True                        # the visible set of the last frame
        cross = {"same_sort_sequence": bool(same_log), "sorts_replayed": len(V_["sorts"]),
                 "consolidated_order_equals_full_mode_order": bool(np.array_equal(V_["order"], F_["order"])),
                 "visible_order_is_subsequence_of_full_mode_order": bool(np.array_equal(V_["vis_order"], F_["order"][gmask[F_["order"]]])),
                 "frames_bit_identical": bool(np.array_equal(V_["img"], F_["img"])), "visible": int(len(V_["vis_order"])),
                 "tie_long_runs": int(V_["vis_stats"].tie_long_runs), "history": V_["history"],
                 "note": "GPU-internal: GS_SORT_VISIBLE's consolidated buffer against the buffer GS_SORT_FULL built with its own sorts over the same frames (the oracle's replay is end_of_orbit_check)"}
        cross["ok"] = all(cross[k] for k in ("same_sort_sequence", "consolidated_order_equals_full_mode_order", "visible_order_is_subsequence_of_full_mode_order", "frames_bit_identical"))
        if "reference_shaped" in res:
            cross["reference_shaped_frame_bit_identical"] = bool(np.array_equal(res["reference_shaped"]["img"], F_["img"]))
        if "visible_in_flight" in res:
            X_ = res["visible_in_flight"]
            cross["in_flight"] = {"lanes": X_["lanes"], "same_sort_sequence": bool(same_sorts(X_["sorts"], F_["sorts"])), "consolidated_order_equals_full_mode_order": bool(np.array_equal(X_["order"], F_["order"])),
                                  "visible_order_identical_to_sequential": bool(np.array_equal(X_["vis_order"], V_["vis_order"])),
                                  "frame_bit_identical": bool(np.array_equal(X_["img"], F_["img"]))}
            cross["in_flight"]["ok"] = all(v for k, v in cross["in_flight"].items() if k != "lanes")
    if world > 1 and cross is not None:
        ok = [None] * world
        dist.all_gather_object(ok, (bool(cross["ok"]), bool(cross.get("in_flight", {}).get("ok", True))))
        cross["ok_all_ranks"] = all(a for a, _ in ok)
        if "in_flight" in cross:
            cross["in_flight"]["ok_all_ranks"] = all(b for _, b in ok)

    # ---- the oracle's end-of-orbit check + the CPU baseline (rank 0, N = 1): the oracle replays EVERY SortPoints of the measurement
    cpu = parity = None
    if rank == 0 and world == 1 and args.cpu_baseline == "auto" and n <= 10_000_000:
        last = res[modes[-1]]["fi"] + args.steps - 1
        cpu, parity = cpu_baseline_and_replay(asset, r, res, cam_at(last, my_views[-1]), n, W, H, r.blendMode)

    headline, headline_reason, failed = pick_headline(args.headline, {m: x["elapsed"] for m, x in res.items()}, parity, cross, modes)
    if failed and rank == 0:
        print(f"bench.py: WARNING: the end-of-orbit check FAILED for {failed}; the headline is the {headline} mode", file=sys.stderr, flush=True)
    if headline not in res:
        headline = modes[0]
    if not args.full and args.headline == "auto":
        headline_reason = ("a plain run measures the default headline mode alone and checks nothing; --full measures every mode, lets the oracle replay the "
                           "orbit and reports the fastest visible-only mode that passes")
    R = res[headline]
    # per-kernel durations, stage brackets and counters are taken with ONE frame at a time: with frames in flight side by side a kernel's bracket
    # holds other frames' kernels too
    K = res["visible"] if headline == "visible_in_flight" and "visible" in res else R
    stage, stage_k, st, resolve_ms, frame_ms = K["stage"], K["stage_k"], R["st"], K["resolve_ms"], K["frame_ms"]
    elapsed = R["elapsed"]
    ms_per_step = elapsed / args.steps * 1e3
    msplats = n * args.steps * num_views / elapsed / 1e6
    ref_msplats = 6_131_954 / 6.8e-3 / 1e6      # 6.8 ms/frame, RTX 3080 Ti, real bicycle scene
    regions = R["regions"]
    vsb = lambda x: round(n * args.steps * num_views / x["elapsed"] / 1e6 / num_views / ref_msplats, 3) if args.config == "C2" and not args.splats else None

    if rank == 0 and args.dump_outputs:
        write_outputs(args.dump_outputs, R["outputs"])

    if rank == 0 and not args.full:
        # a plain run: the headline figure and what it was measured on (everything else: --full)
        out = {
            "metric": f"Msplats/s rendered (sort+view+composite+resolve), {cfg.label}; ms/frame in ms_per_step",
            "value": round(msplats, 2), "unit": "Msplats/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "ms_per_step_regions": [round(x / args.steps * 1e3, 4) for x in regions],
            "ms_per_step_per_rank": [round(x / args.steps * 1e3, 4) for x in R["per_rank"]] if R["per_rank"] else None,
            "higher_is_better": True, "scaling": "strong" if args.config == "C5" else "weak",
            "vs_baseline": vsb(R), "dtype": "f32", "data": "synthetic", "full": False,
            "config": {"workload": cfg.label + (f" [splat count overridden to {n}]" if args.splats else ""),
                       "sort_mode": headline, "headline_reason": headline_reason,
                       "frames_in_flight": (R.get("lanes", 1) if headline == "visible_in_flight" else 1),
                       "frames_in_flight_impl": (R.get("impl") if headline == "visible_in_flight" else None),
                       "splats": n, "resolution": [W, H], "asset_MB": round(asset_bytes / 1e6, 1), "views": num_views, "views_per_rank": len(my_views),
                       "blend": args.blend, "sort_nth_frame": args.sort_nth_frame, "tile_pairs_P": int(st.tile_pairs), "tile": f"{st.tile_w}x{st.tile_h}",
                       "visible_splats": int(st.visible_splats),
                       "parallelism": (f"view-parallel x{world} (one camera per GPU, asset broadcast once by gs_asset_broadcast = ncclBroadcast per blob)" if world > 1 else "single GPU"),
                       "rccl_ranks": rccl_ranks, "host_group": ("gloo" if world > 1 else None),
                       "baseline_note": "vs_baseline = per-view Msplats/s / 901.8 (reference: 6.8 ms/frame on RTX 3080 Ti with the REAL INRIA bicycle, whose overdraw is far higher than this synthetic scene's: context only)"},
            "modes": {m: {"ms_per_step": round(x["elapsed"] / args.steps * 1e3, 4), "value_Msplats_s": round(n * args.steps * num_views / x["elapsed"] / 1e6, 2)}
                      for m, x in res.items()},
            "setup_s": {"scene_build": round(t_build, 1), "asset_broadcast": round(t_bcast, 3)},
        }
        print(json.dumps(out), flush=True)

    if rank == 0 and args.full:
        P = int(st.tile_pairs)
        numTiles = st.tiles_x * st.tiles_y
        passes_pair = 1 if numTiles <= 256 else (2 if numTiles <= 65536 else 3)
        vis = int(st.visible_splats)
        vmode = headline in ("visible", "visible_in_flight")
        sb = stage_bytes(n, P, vis, W, H, r.m_Asset, passes_pair, "visible" if vmode else "full", depth_passes=(int(stage.onesweep_depth_launches) or 4))
        times = {"calc_distances": stage.calc_distances_ms, "sort": stage.sort_ms, "calc_view": stage.calc_view_ms,
                 "bin": stage.bin_ms, "pair_sort": stage.pair_sort_ms, "blend": stage.blend_ms, "resolve": resolve_ms}
        stages = {}
        for k, ms in times.items():
            gbs = sb[k] / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
            stages[k] = {"ms": round(ms, 4), "alg_MB": round(sb[k] / 1e6, 2), "GBps": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}
        # Kernels by total time per frame.  The Onesweep launches of a frame (4 depth-sort passes + the pair-sort passes) are one kernel, timed by
        # the launches' OWN start / stop timestamps (gs_stage_times.onesweep_*_kernel_ms = what rocprofv3 --kernel-trace reports; the hipEventRecord
        # brackets around them include kernel boundaries and barrier packets and read 8-10 % high).  The other kernels are one launch (or, for the
        # visible-only binning, three) per stage bracket.
        key_kernel = "visible_keys_kernel" if vmode else "sort_keys_kernel"
        bin_kernel = "vis_count+vis_offsets+vis_emit" if vmode else "bin_emit_kernel"
        depth_launches = int(stage.onesweep_depth_launches) or 4
        launches = {"onesweep_kernel": depth_launches + int(stage.onesweep_pair_launches), "blend_kernel": 1, "calc_view_kernel": 1, bin_kernel: 3 if vmode else 1, key_kernel: 1}
        sweep_ms = stage_k.onesweep_depth_kernel_ms + stage_k.onesweep_pairs_kernel_ms
        if not sweep_ms > 0:
            sweep_ms = stage.onesweep_depth_ms + stage.onesweep_pairs_ms
        ktime = {"onesweep_kernel": sweep_ms, "blend_kernel": stage.blend_ms, "calc_view_kernel": stage.calc_view_ms, bin_kernel: stage.bin_ms, key_kernel: stage.calc_distances_ms}
        depth_keys = vis if vmode else n
        kbytes = {"onesweep_kernel": depth_keys * (16 * depth_launches - (0 if vmode else 4)) + P * 16 * passes_pair, "blend_kernel": sb["blend"], "calc_view_kernel": sb["calc_view"],
                  bin_kernel: sb["bin"], key_kernel: sb["calc_distances"]}
        frame_bytes = sum(sb.values())

        # ---- counters of THIS run: rocprofv3 --pmc children over the headline mode's own frames
        pmc = None
        if args.pmc == "auto" and world == 1:
            pmc = pmc_children(args, asset, "visible" if vmode else headline, R["fi"], frames_warm)
        pk = (pmc or {}).get("kernels", {})
        probe = run_valu_probe()
        valu_measured = float(probe["gwi_per_s"]) if probe and probe.get("gwi_per_s") else VALU_MEASURED_GWI_STORED

        def counted(k):
            """HBM bytes per launch of kernel k from this run's FETCH_SIZE / WRITE_SIZE children, corrected as the guide prescribes for gfx950:
            FETCH_SIZE tallies a coalesced stream at half its bytes (x 2.0; WRITE_SIZE at face value: calibrated on 1-GiB kernels, profiles/hbm_traffic.json).
            Kernels whose reads are lone random gathers (a request is tallied at ~42 B, face value) are given as the lower end, the x 2.0 figure beside it."""
            parts = [x for x in k.split("+")]
            es = [pk.get(x if x.endswith("_kernel") else x + "_kernel") for x in parts]
            if not es or any(e is None or "FETCH_SIZE_KiB" not in e or "WRITE_SIZE_KiB" not in e for e in es):
                return None, None
            gather = any(x.startswith(("vis_count", "bin_emit")) for x in parts)
            lo = sum((e["FETCH_SIZE_KiB"] * (1.0 if x.startswith(("vis_count", "bin_emit")) else 2.0) + e["WRITE_SIZE_KiB"]) * 1024 for e, x in zip(es, parts))
            hi = sum((e["FETCH_SIZE_KiB"] * 2.0 + e["WRITE_SIZE_KiB"]) * 1024 for e in es)
            return int(lo / (launches[k] if k == bin_kernel else 1)), (int(hi / (launches[k] if k == bin_kernel else 1)) if gather else None)

        traffic_source = ("measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE children of this script over the same frames (per-launch mean over the last "
                          f"{args.steps} frames; FETCH_SIZE x 2.0 as the guide prescribes for gfx950 streams, gather-dominated kernels at face value)") if pk else \
                         ("not collected: " + ((pmc or {}).get("error") or ("--pmc off" if args.pmc == "off" else "N > 1" if world > 1 else "the rocprofv3 children returned no counters")))

        def roof_hbm(k):
            """HBM roofline of kernel k as the contract states it: algorithmic bytes per launch / its mean launch duration against the 8 TB/s spec peak."""
            k_ms = ktime[k] / launches[k]
            k_bytes = kbytes[k] / launches[k]
            ach = k_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
            traffic, traffic_hi = counted(k)
            out = {"bound": "hbm", "kernel": k, "launches_per_frame": launches[k], "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                   "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                   "traffic_over_algorithmic": round(traffic / k_bytes, 3) if traffic else None,
                   "achievable_peak": HBM_ACHIEVABLE_GBS, "frac_of_achievable": round(ach / HBM_ACHIEVABLE_GBS, 4),
                   "alg_bytes_per_launch": int(k_bytes), "avg_launch_ms": round(k_ms, 4)}
            if traffic_hi:
                out["traffic_upper"] = traffic_hi
            return out

        def roof(k):
            """`frac` is the contract's: algorithmic HBM bytes / launch duration / 8 TB/s.  The blend and calc_view are VALU-bound (SQ counters, profiles/), so
            their wave-level VALU instruction count -- SQ_INSTS_VALU of this run's child pass -- is priced under `valu` against BOTH issue roofs: the spec
            (2 cycles per wave64 instruction at 2.4 GHz: 1,229 G/s) and the rate plain v_fma_f32 streams sustain on this part (scripts/probes/valu_issue.hip)."""
            h = roof_hbm(k)
            if k not in ("blend_kernel", "calc_view_kernel"):
                return h
            wi = pk.get(k, {}).get("SQ_INSTS_VALU")
            k_ms = ktime[k] / launches[k]
            ach = (wi / (k_ms * 1e-3) / 1e9) if (wi and k_ms > 0) else None
            h["valu"] = {"wave_insts_per_launch": int(wi) if wi else None,
                         "insts_source": ("measured in this run: rocprofv3 --pmc SQ_INSTS_VALU child of this script over the same frames" if wi else "not collected"),
                         "achieved": round(ach, 1) if ach else None, "unit": "G wave-instructions/s",
                         "roof_spec": round(VALU_SPEC_GWI, 1), "frac_of_spec": round(ach / VALU_SPEC_GWI, 4) if ach else None,
                         "roof_measured": round(valu_measured, 1), "frac_of_measured": round(ach / valu_measured, 4) if ach else None,
                         "roof_measured_source": (("measured in this run: scripts/probes/valu_issue --quick (v_fma_f32, 8 waves per SIMD, whole chip; shader clock under that load "
                                                   f"{probe.get('mhz_under_load')} MHz of {probe.get('mhz_light')} MHz with one wave per SIMD)") if probe else
                                                  "STORED: profiles/r05_valu_issue.txt (the probe binary was not built)"),
                         "roof_spec_source": "256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles per wave64 fp32 instruction (MI355X_MICROARCH.md) = 157.3 TFLOP/s fp32 vector / 128"}
            return h

        # `roofline` = the kernel with the largest total time per frame, as the contract asks; `roofline_blend` and `roofline_streaming` (the
        # bandwidth-type kernel with the largest time: the Onesweep launches) are ALWAYS emitted under fixed keys so that rounds can be compared.
        dom = max(ktime, key=lambda k: ktime[k])
        roofline = roof(dom)
        roofline_blend = roof("blend_kernel")
        stream_dom = max((k for k in ktime if k not in ("blend_kernel", "calc_view_kernel")), key=lambda k: ktime[k])
        roofline_streaming = roof(stream_dom)
        roofline.update({"frames_averaged": int(stage.frames),
                    "instrumented_ms_per_step": round(K["elapsed_instr"] / args.steps * 1e3, 4),
                    "instrumented_frame_gpu_ms": ({"median": round(float(np.median(frame_ms)), 4), "p95": round(float(np.percentile(frame_ms, 95)), 4),
                                                   "max": round(float(frame_ms.max()), 4), "frames": int(len(frame_ms))} if len(frame_ms) else None),
                    "timing": "onesweep_kernel: the launches' own start/stop timestamps (hipExtLaunchKernelGGL events = rocprofv3's kernel durations) from a third pass over the same K frames; `stages` and the other kernels: hipEventRecord brackets on the launching stream from a second pass (the events add ~50 us/frame, so ms_per_step is timed without either)",
                    "onesweep_bracketed_ms_per_frame": round(stage.onesweep_depth_ms + stage.onesweep_pairs_ms, 4),
                    "kernel_ms_per_frame": {k: round(v, 4) for k, v in ktime.items()},
                    "counters_per_launch": {k: {kk: (round(vv, 1) if isinstance(vv, float) else vv) for kk, vv in v.items()} for k, v in pk.items()} or None,
                    "pmc_passes": (pmc or {}).get("passes"), "pmc_seconds": (pmc or {}).get("seconds"),
                    # (a step renders every view of this rank once: C5 on one GPU = 8 frames per step)
                    "whole_frame": {"alg_MB": round(frame_bytes / 1e6, 1), "frames_per_step": len(my_views),
                                    "GBps": round(frame_bytes * len(my_views) / (ms_per_step * 1e-3) / 1e9, 1),
                                    "hbm_frac": round(frame_bytes * len(my_views) / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                    "survey_8d_formula": None}})
        # SURVEY.md section 8(d)'s own whole-frame formula, N B_s + P B_p + W H B_px (the reference-shaped path moves it; the visible-only path moves less)
        b_s = 212.5 if r.m_Asset.chunkCount else 408.0
        survey_bytes = n * b_s + P * 40.0 + W * H * 20.0
        roofline["whole_frame"]["survey_8d_formula"] = {"MB": round(survey_bytes / 1e6, 1), "hbm_frac_at_this_ms_per_step": round(survey_bytes * len(my_views) / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                                        "note": "N x B_s + P x 40 + W x H x 20 with B_s = 212.5 (Medium) / 408 (fp32): what the reference-shaped path moves; the headline mode's own bytes are alg_MB"}
        roofline["measured_copy_ceiling_GBps"] = copy_ceiling             # measured before the timed regions

        def mode_summary(x):
            s_, k_ = x["stage"], x["stage_k"]
            if s_ is None:
                return {"ms_per_step": round(x["elapsed"] / args.steps * 1e3, 4), "value_Msplats_s": round(n * args.steps * num_views / x["elapsed"] / 1e6, 2),
                        "regions_ms_per_step": [round(v / args.steps * 1e3, 4) for v in x["regions"]], "renderers_in_flight": x["lanes"],
                        "in_flight_impl": ("library: ONE renderer on one context and the reference's calls; gs_renderer_set_frames_in_flight deals the frames to lanes inside the library"
                                           if x.get("impl") == "library" else "host: the host holds the renderers (one context each) and deals the frames itself"),
                        "tile_pairs_P": int(x["st"].tile_pairs), "visible_splats": int(x["st"].visible_splats), "sort_history": x["history"],
                        "note": "GS_SORT_VISIBLE with the frames (C5: the views) dealt round-robin to this many renderers on contexts (streams) of their own over ONE copy of the asset; "
                                "every renderer is told every SortPoints matrix, each draws its frames from the reference's order (checked: sort_mode_cross_check.in_flight, end_of_orbit_check); "
                                "throughput with frames in flight, not the latency of one frame"}
            return {"ms_per_step": round(x["elapsed"] / args.steps * 1e3, 4), "value_Msplats_s": round(n * args.steps * num_views / x["elapsed"] / 1e6, 2),
                    "regions_ms_per_step": [round(v / args.steps * 1e3, 4) for v in x["regions"]],
                    "tile_pairs_P": int(x["st"].tile_pairs), "visible_splats": int(x["st"].visible_splats),
                    "stages_ms": {"calc_distances": round(s_.calc_distances_ms, 4), "sort": round(s_.sort_ms, 4), "calc_view": round(s_.calc_view_ms, 4),
                                  "bin": round(s_.bin_ms, 4), "pair_sort": round(s_.pair_sort_ms, 4), "blend": round(s_.blend_ms, 4), "resolve": round(x["resolve_ms"], 4)},
                    "onesweep_depth_kernel_ms": round(k_.onesweep_depth_kernel_ms, 4), "onesweep_pairs_kernel_ms": round(k_.onesweep_pairs_kernel_ms, 4),
                    "first_frame_ms": round(x["first_frame_ms"], 3) if x["first_frame_ms"] is not None else None,
                    "first_frame_again_ms": round(x["first_again_ms"], 3) if x["first_again_ms"] is not None else None,
                    "sort_history": x["history"]}

        out = {
            "metric": f"Msplats/s rendered (sort+view+composite+resolve), {cfg.label}; ms/frame in ms_per_step",
            "value": round(msplats, 2), "unit": "Msplats/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "ms_per_step_regions": {"median": round(ms_per_step, 4), "min": round(min(regions) / args.steps * 1e3, 4), "max": round(max(regions) / args.steps * 1e3, 4),
                                    "all": [round(x / args.steps * 1e3, 4) for x in regions],
                                    "note": f"{len(regions)} back-to-back regions of exactly {args.steps} steps each (barrier + synchronize on both sides); value and ms_per_step are the median region"},
            "ms_per_step_per_rank": [round(x / args.steps * 1e3, 4) for x in R["per_rank"]] if R["per_rank"] else None,
            "higher_is_better": True, "scaling": "strong" if args.config == "C5" else "weak",
            # BASELINE.md's only number (6.8 ms/frame, RTX 3080 Ti) is for the REAL bicycle scene; this is the synthetic stand-in of
            # the same size, so the ratio is context, not a like-for-like comparison (config.baseline_note)
            "vs_baseline": vsb(R),
            "vs_baseline_by_mode": {m: vsb(x) for m, x in res.items()},
            "dtype": "f32", "data": "synthetic", "full": True,
            "config": {"workload": cfg.label + (f" [splat count overridden to {n}]" if args.splats else ""),
                       "sort_mode": headline, "headline_reason": headline_reason,
                       "frames_in_flight": (R.get("lanes", 1) if headline == "visible_in_flight" else 1),
                       "frames_in_flight_impl": (R.get("impl") if headline == "visible_in_flight" else None),
                       "one_frame_at_a_time_ms": (round(res["visible"]["elapsed"] / args.steps * 1e3, 4) if "visible" in res else None),
                       "sort_mode_note": ("visible_in_flight = GS_SORT_VISIBLE with the frames (C5: the views) dealt round-robin to --in-flight renderers on contexts (streams) of their own over ONE copy of "
                                          "the asset: one frame's latency-bound sort / binning kernels run under another's VALU-bound blend; throughput, each frame the same bits; per-kernel figures "
                                          "(`roofline`, `stages`) are taken one frame at a time (modes.visible); visible = GS_SORT_VISIBLE: cull first, key + sort + bin the V visible splats only, ties ordered by the chain of every recorded sort matrix and the base "
                                          "order -- the same frame and the same order among the drawn splats as the reference's full sort (tests/test_gpu_vissort.py; this run: `end_of_orbit_check`, "
                                          "`sort_mode_cross_check`); full = SortPoints as the reference runs it (all N), colours only for visible splats; reference_shaped = full + the reference's "
                                          "whole CSCalcViewData (colour + 40-byte view record of every splat in front of the camera) every frame: the like-for-like figure; all are in `modes`"),
                       "splats": n, "resolution": [W, H], "asset_MB": round(asset_bytes / 1e6, 1), "views": num_views, "views_per_rank": len(my_views),
                       "blend": args.blend, "sort_nth_frame": args.sort_nth_frame, "view_buffer": "on demand (gs_renderer_download_view); every frame in modes.reference_shaped",
                       "sort_queue_overlap": os.environ.get("GSPLAT_OVERLAP", "0") == "1", "tile_pairs_P": P, "tile": f"{st.tile_w}x{st.tile_h}", "visible_splats": int(st.visible_splats),
                       "parallelism": (f"view-parallel x{world} (one camera per GPU, asset broadcast once by gs_asset_broadcast = ncclBroadcast per blob)" if world > 1 else "single GPU"),
                       "rccl_ranks": rccl_ranks, "host_group": ("gloo" if world > 1 else None),
                       "baseline_note": "vs_baseline = per-view Msplats/s / 901.8 (reference: 6.8 ms/frame on RTX 3080 Ti with the REAL INRIA bicycle, whose overdraw is far higher than this synthetic scene's: context only)"},
            "modes": {m: mode_summary(x) for m, x in res.items()},
            "sort_mode_cross_check": cross,
            "end_of_orbit_check": (parity or {}).get("visible_mode"),
            "first_frame_ms": round(R["first_frame_ms"], 3) if R["first_frame_ms"] is not None else None,
            "first_frame_note": "first_frame_ms: the mode's very first frame after CSSetIndices, host-timed incl. the launch of ~15 kernels for the first time (code-object load), the pair-buffer's first sizing and first-touch of every buffer; modes.*.first_frame_again_ms: the same frame again",
            "roofline": roofline, "roofline_blend": roofline_blend, "roofline_streaming": roofline_streaming, "stages": stages, "cpu_baseline": cpu, "parity_vs_oracle": parity,
            "setup_s": {"scene_build": round(t_build, 1), "asset_broadcast": round(t_bcast, 3)},
        }
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
    if comm is not None:
        comm.Dispose()
    if dist is not None:
        dist.destroy_process_group()


def pick_headline(want, elapsed, parity, cross, modes):
    """Which measured mode `value` reports.  want: --headline.  elapsed: {mode: seconds of its median region}.  A visible-only mode qualifies only if its
    end-of-orbit check holds -- the oracle's replay when this run has it (parity), else the GPU-internal cross-check against the full mode (cross) -- and the
    fastest qualifying one wins; if none qualifies the headline is the reference-shaped full sort.  Returns (mode, reason, modes whose check FAILED)."""
    if want != "auto":
        return (want if want in elapsed else modes[0]), "pinned by --headline", []

    def verified(mode):
        key = "visible_mode" if mode == "visible" else "visible_in_flight"
        if parity is not None and key in parity:
            return bool(parity[key]["ok"]), "the oracle's end-of-orbit replay"
        if cross is not None:
            c = cross if mode == "visible" else cross.get("in_flight")
            if c is not None:
                return bool(c.get("ok_all_ranks", c["ok"])), "the GPU-internal end-of-orbit cross-check against the full mode (no oracle in this run)"
        return True, "no check in this run (only this mode was measured)"
    cands = [m for m in ("visible_in_flight", "visible") if m in elapsed]
    checked = [(m,) + verified(m) for m in cands]
    failed = [m for m, ok, _ in checked if not ok]
    good = [(m, how) for m, ok, how in checked if ok]
    if good:
        mode, how = min(good, key=lambda t: elapsed[t[0]])
        return mode, f"the fastest mode that draws the reference's frame from the reference's order; verified by {how}", failed
    mode = "full" if "full" in elapsed else modes[0]
    return mode, ("the visible-only modes were not measured" if not cands else "THE END-OF-ORBIT CHECK OF THE VISIBLE-ONLY MODES FAILED"), failed


def same_sorts(a, b):
    """Two SortPoints logs describe the same sequence of sorts: equal once immediate repetitions of a matrix are dropped (a stable sort of a
    sequence already sorted by that matrix changes nothing -- a warm-up frame that is drawn again after a pair-buffer overflow logs its matrix twice)."""
    def dedup(log):
        out = []
        for m in log:
            if not out or not (out[-1] is m or np.array_equal(out[-1], m)):
                out.append(m)
        return out
    a, b = dedup(a), dedup(b)
    return len(a) == len(b) and all(x is y or np.array_equal(x, y) for x, y in zip(a, b))


DUMP_BYTES = 63_000_000        # --dump-outputs: at most this much in all (64 MB with the .npy headers and some room)
DUMP_ORDER_SAMPLE = 1 << 20    # entries kept of an order buffer (millions of splats)


def seeded_sample(a, k, name):
    """A fixed subset of k elements of `a` (flattened), in index order; the positions depend only on the name and the size."""
    a = np.asarray(a).reshape(-1)
    if a.size <= k:
        return a
    import zlib
    idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, k, replace=False))
    return a[idx]


def cap_outputs(arrays):
    """{name: float32 / float64 array} within DUMP_BYTES: when the whole set is larger, every array becomes the same fraction of its elements
    (seeded_sample, flattened)."""
    total = sum(v.nbytes for v in arrays.values())
    if total <= DUMP_BYTES:
        return arrays
    f = DUMP_BYTES / total * 0.99
    return {k: seeded_sample(v, max(1, int(v.size * f)), k) for k, v in arrays.items()}


def write_outputs(out_dir, arrays):
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)


def cpu_baseline_and_replay(asset, r, res, cam, n, W, H, blend_mode):
    """The oracle (CPU restatement of the reference shaders, oracle/gs_oracle.cpp) as the run's checker and as the reported CPU baseline.

    Checker: it REPLAYS every SortPoints of the measurement -- the warm-up and every timed / instrumented region, the same sequence in every
    mode -- as what the reference does: a stable sort of all N splats through the previous order, one after the other.  At the end of that orbit
      * full / reference_shaped mode: the library's order buffer == the oracle's, its last frame within the framebuffer bar of the oracle's;
      * visible-only mode: the order its last frame was drawn from == the visible subsequence of the oracle's buffer, its consolidated buffer
        (gs_renderer_download_order: the recorded sorts carried out on all N) == the oracle's whole buffer, its frame within the bar.
    Baseline: one whole frame (sort + view + composite + resolve) of the same workload on the host cores, timed at the last camera."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    from common import RT_TOL, rt_diff, rt_err
    orc = O.Oracle(asset)
    cores = int(O.lib().gso_num_threads())
    P = r.FrameParams(cam)
    ref_mode = next((m for m in ("visible", "full", "reference_shaped", "visible_in_flight") if m in res), None)
    sorts = res[ref_mode]["sorts"]
    t_replay = time.perf_counter()
    replayed = 0
    prev = None
    t_sort = None
    for m16 in sorts:
        if prev is not None and np.array_equal(prev, m16):
            continue                                         # the same matrix again: a stable sort of a sequence already sorted by it changes nothing
        t0 = time.perf_counter()
        orc.sort(m16)
        t_sort = time.perf_counter() - t0
        prev = m16
        replayed += 1
    t_replay = time.perf_counter() - t_replay
    t1 = time.perf_counter()
    orc.calc_view(P)
    t2 = time.perf_counter()
    ref = orc.draw(P, blend_mode)
    t3 = time.perf_counter()
    O.resolve(ref, (0, 0, 0, 1))
    t4 = time.perf_counter()
    total = (t_sort or 0.0) + (t4 - t1)
    _, _, vbits = orc.raster_records(P)
    mask = np.unpackbits(vbits.view(np.uint8), bitorder="little")[:n].astype(bool)

    def frame_check(img):
        a, b = O.f16_to_f32(img), O.f16_to_f32(ref)
        d = np.abs(a - b)
        e = rt_diff(img, ref).max(axis=-1)
        return {"rt_max_abs": float(d.max()), "rt_mean_abs": float(d.mean()), "rt_pixels_bit_equal": float((img == ref).all(axis=2).mean()),
                "rt_max_rel": float(e.max()), "rt_pixels_over_2^-9": int((e > RT_TOL).sum()), "within_bar": bool(rt_err(img, ref) <= RT_TOL)}      # every pixel, no outlier allowance

    parity = {"oracle_sorts_replayed": replayed, "sort_calls_in_the_measurement": len(sorts), "replay_seconds": round(t_replay, 1),
              "what": "the oracle replayed every SortPoints of the measurement (warm-up + every region) as a stable sort of all N through the previous order; compared on the orbit's last frame"}
    fm = "full" if "full" in res else ("reference_shaped" if "reference_shaped" in res else None)
    if fm:
        x = res[fm]
        same = same_sorts(x["sorts"], sorts)
        parity.update({"order_bit_exact": bool(same and np.array_equal(x["order"], orc.order)), **frame_check(x["img"]),
                       "tile_pairs_equal": bool(int(x["st"].tile_pairs) == int(orc.pairs(P, x["st"])))})
    if "visible" in res:
        x = res["visible"]
        v = {"order_is_visible_subsequence_of_oracle_order": bool(np.array_equal(x["vis_order"], orc.order[mask[orc.order]])),
             "consolidated_order_equals_oracle_order": bool(np.array_equal(x["order"], orc.order)),
             "visible": int(len(x["vis_order"])), "sort_history": x["history"], **frame_check(x["img"]),
             "tile_pairs_equal": bool(int(x["st"].tile_pairs) == int(orc.pairs(P, x["st"])))}
        if fm:
            v["frame_bit_identical_to_full_mode"] = bool(np.array_equal(x["img"], res[fm]["img"]))
        v["ok"] = bool(v["order_is_visible_subsequence_of_oracle_order"] and v["consolidated_order_equals_oracle_order"] and v["within_bar"] and v["tile_pairs_equal"])
        parity["visible_mode"] = v
    if "visible_in_flight" in res:
        x = res["visible_in_flight"]
        same = same_sorts(x["sorts"], sorts)
        v = {"renderers_in_flight": x["lanes"], "same_sort_sequence": bool(same),
             "order_is_visible_subsequence_of_oracle_order": bool(np.array_equal(x["vis_order"], orc.order[mask[orc.order]])),
             "consolidated_order_equals_oracle_order": bool(np.array_equal(x["order"], orc.order)), **frame_check(x["img"]),
             "tile_pairs_equal": bool(int(x["st"].tile_pairs) == int(orc.pairs(P, x["st"])))}
        v["ok"] = bool(same and v["order_is_visible_subsequence_of_oracle_order"] and v["consolidated_order_equals_oracle_order"] and v["within_bar"] and v["tile_pairs_equal"])
        parity["visible_in_flight"] = v
    cpu = {"value": round(n / total / 1e6, 3), "unit": "Msplats/s", "cores": cores, "kind": "port",
           "sample": f"1 whole frame of the same workload ({n} splats, {W}x{H}): sort {t_sort or 0.0:.2f}s + view {t2 - t1:.2f}s + "
                     f"composite {t3 - t2:.2f}s + resolve {t4 - t3:.2f}s = {total:.2f}s on {cores} OpenMP threads (the sort = the last of the {replayed} replayed)",
           "ms_per_frame": round(total * 1e3, 1)}
    return cpu, parity


if __name__ == "__main__":
    main()
