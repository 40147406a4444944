#!/usr/bin/env python3
"""What pick output (gs_target_set_pick_output) costs the blend of bench.py's C2 frame, in both blend modes.

    timeout 900 python scripts/pick_timing.py [--config C2] [--draws 7] [--out profiles/pick_timing.json]

One GPU, one call.  Every leg is a fresh child process (one per blend mode): sort + calc_view once, a warm-up, then `draws` draws (clear + draw of the same
view) with pick output off and `draws` with it on, each bracketed by the renderer's own hipEvents; reported: the median blend_ms of each set.  The blend
bracket of a draw with pick output on holds splat_depth_kernel too (the draw launches it for the records' depth), so each leg is run a second time under
`rocprofv3 --kernel-trace` -- a run of its own, no counters -- and the medians of the kernels' own durations are read from its csv: blend_kernel with
and without PICK, and splat_depth_kernel.  Where the tracer is not installed that part is recorded as missing.  The extra traffic is arithmetic: 16 bytes per
pixel of records, 4 bytes per splat of recW written and one 4-byte gather per staged record.
A record: the script asserts nothing about the times.  A leg that fails ends the run: nothing more is started on the GPU."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(blend: int, draws: int, config: str) -> dict:
    from unitygaussiansplatting_amd import _lib, camera, creator, scenes
    from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext, RenderTarget, SortMode

    cfg = scenes.CONFIGS[config]
    raw = scenes.make_config_splats(cfg, 0)
    asset = creator.CreateAssetFromSplatsNative(raw, cfg.quality, name=cfg.key)
    del raw
    ctx = GpuContext(0)
    r = GaussianSplatRenderer(ctx, asset)
    r.sortMode = SortMode.Visible
    r.blendMode = blend
    r.OnEnable()
    rt = RenderTarget(ctx, cfg.width, cfg.height)
    cam = camera.Camera(position=scenes.orbit_eye(cfg.eye_radius, cfg.eye_elev_deg, 30.0), pixelWidth=cfg.width, pixelHeight=cfg.height, fieldOfView=cfg.fov_y)
    r.SortPoints(cam); r.CalcViewData(cam)
    stats = None
    for _ in range(8):                                             # warm-up: the pair buffers grow to what the frame needs, the tile schedule settles
        rt.Clear(); r.Draw(cam, rt)
        try:
            stats = r.FrameStats()
        except _lib.GsError as ex:
            if ex.code != -6:
                raise
            stats = None
    if stats is None:
        raise SystemExit("the pair buffers did not settle")
    r.SetProfiling(2)

    def measure():
        ms = []
        for _ in range(3):                                         # the kernels of this setting once more before the clock counts
            rt.Clear(); r.Draw(cam, rt)
        r.StageTimes()
        for _ in range(draws):
            rt.Clear(); r.Draw(cam, rt)
            ms.append(float(r.StageTimes().blend_ms))
        return ms

    off = measure()
    rt.SetPickOutput(True, 0.5)
    on = measure()
    rec = rt.DownloadPick()
    crossed = float((rec["splat"] != 0xFFFFFFFF).mean())
    out = {"blend_mode": "exact" if blend == 0 else "fast", "splats": asset.splatCount, "width": cfg.width, "height": cfg.height, "tile": [int(stats.tile_w), int(stats.tile_h)],
           "tile_pairs": int(stats.tile_pairs), "visible_splats": int(stats.visible_splats), "draws": draws,
           "blend_ms_pick_off": {"median": statistics.median(off), "all": off}, "blend_ms_pick_on_with_depth_kernel": {"median": statistics.median(on), "all": on},
           "crossed_share_at_0.5": crossed}
    r.OnDisable(); rt.Dispose(); ctx.Dispose()
    return out


def kernel_medians(trace_dir: str, draws: int):
    """medians of the last `draws` durations (ms) of splat_depth_kernel and of the blend_kernel instantiations without / with PICK, from a kernel-trace csv"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    dur = {"splat_depth_kernel": [], "blend_kernel_pick_off": [], "blend_kernel_pick_on": []}
    for x in rows:
        name, ms = x["Kernel_Name"], (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e6
        if "splat_depth_kernel" in name:
            dur["splat_depth_kernel"].append(ms)
        elif "blend_kernel<" in name:
            args = name[name.index("blend_kernel<") + len("blend_kernel<"):].split(">")[0].replace(" ", "").split(",")
            pick = len(args) >= 6 and args[5] in ("true", "1", "(bool)1")
            dur["blend_kernel_pick_on" if pick else "blend_kernel_pick_off"].append(ms)
    return {k: {"median_ms": statistics.median(v[-draws:]), "launches": len(v)} if v else None for k, v in dur.items()}


def run_leg(blend: int, args, traced: bool):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", str(blend), "--draws", str(args.draws), "--config", args.config]
    tmp = None
    if traced:
        tmp = tempfile.mkdtemp(prefix="pick_trace_")
        cmd = [shutil.which("rocprofv3"), "--kernel-trace", "--output-format", "csv", "-d", tmp, "--"] + cmd
    try:
        p = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=420)
        line = next((l for l in p.stdout.splitlines() if l.startswith("{")), None)
        if p.returncode != 0 or line is None:                      # whatever it was, nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"leg blend={blend} traced={traced} failed with exit status {p.returncode}")
        return json.loads(line), (kernel_medians(tmp, args.draws) if traced else None)
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--draws", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pick_timing.json"))
    ap.add_argument("--leg", type=int, choices=(0, 1), help="(internal) run one blend mode in this process and print its JSON line")
    args = ap.parse_args()
    if args.leg is not None:
        print(json.dumps(leg(args.leg, args.draws, args.config)))
        return 0
    legs = []
    for blend in (0, 1):
        res, _ = run_leg(blend, args, False)
        print(json.dumps(res), flush=True)
        if shutil.which("rocprofv3"):
            _, res["kernel_trace"] = run_leg(blend, args, True)
        else:
            res["kernel_trace"] = None
        off, on = res["blend_ms_pick_off"]["median"], res["blend_ms_pick_on_with_depth_kernel"]["median"]
        res["pick_on_minus_off_ms"] = on - off
        res["pick_on_over_off"] = on / off if off else None
        px, n = res["width"] * res["height"], res["splats"]
        res["extra_traffic_bytes_per_draw"] = {"records_16B_per_pixel": 16 * px, "recW_written_at_most_4B_per_splat": 4 * n,
                                               "recW_gathered_4B_per_staged_record": 4 * res["tile_pairs"]}
        legs.append(res)
        print(json.dumps({k: res[k] for k in ("blend_mode", "pick_on_minus_off_ms", "pick_on_over_off", "kernel_trace")}), flush=True)
    out = {"what": "scripts/pick_timing.py: the blend of one C2 view with pick output off and on, medians of the draws' blend_ms (hipEvents) and, from a kernel trace "
                   "of a second run, of the kernels' own durations; recorded, no threshold",
           "config": args.config, "legs": legs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
