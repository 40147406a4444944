#!/usr/bin/env python3
"""What the selection highlight (gs_renderer_set_selection_highlight) costs a frame of bench.py's C2, and that it costs nothing while it is off.

    timeout 900 python scripts/highlight_timing.py --parent-lib PATH [--frames 30] [--out profiles/highlight_timing.json]

One GPU, one call.  Every leg is a fresh child process (a library is chosen per process, through GSPLAT_LIB): the PARENT commit's library and this one
alternate, as scripts/ab_rounds.sh alternates two builds --
    (a) parent, off, parent, off: the frame without highlight against the parent, with the spread of the two parent runs next to the difference;
    (b) highlight on with nothing selected, with every 100th splat selected, with everything selected: reported, not bounded.
A leg renders the same orbit (sort + calc_view + clear + draw per frame, GS_SORT_VISIBLE) three times after a warm-up and reports, per frame, the wall time
of the un-instrumented loop (min and median of the three regions) and the hipEvent stage means of a fourth, profiled region.  A leg that fails ends the run:
nothing more is started on the GPU.  A record: the script asserts nothing about the times (the reader compares (a)'s difference with the parent's spread)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("parent", "off", "on_nothing_selected", "on_1_percent_selected", "on_all_selected")


def leg(name: str, frames: int, config: str) -> dict:
    import numpy as np

    from unitygaussiansplatting_amd import _lib, camera, creator, scenes
    from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext, RenderTarget, SortMode

    cfg = scenes.CONFIGS[config]
    raw = scenes.make_config_splats(cfg, 0)
    asset = creator.CreateAssetFromSplatsNative(raw, cfg.quality, name=cfg.key)
    del raw
    n = asset.splatCount
    ctx = GpuContext(0)
    r = GaussianSplatRenderer(ctx, asset)
    r.sortMode = SortMode.Visible
    r.OnEnable()
    rt = RenderTarget(ctx, cfg.width, cfg.height)
    cams = [camera.Camera(position=scenes.orbit_eye(cfg.eye_radius, cfg.eye_elev_deg, 30.0 + 0.5 * k), pixelWidth=cfg.width, pixelHeight=cfg.height, fieldOfView=cfg.fov_y)
            for k in range(frames)]
    prepared = [(r.SortMatrix(c), r.FrameParams(c)) for c in cams]
    selected = 0
    if name.startswith("on_"):
        r.SetSelectionHighlight(True)
        if name == "on_nothing_selected":
            r.EditDeselectAll()                                    # the edit buffers exist: the highlight kernels run, over no mark
        elif name == "on_1_percent_selected":
            m = np.zeros(((n + 31) // 32) * 32, np.uint8)
            m[:n:100] = 1
            r.UploadSelectedBits(np.packbits(m.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1))
        else:
            r.EditSelectAll()
        selected = int(r.editSelectedSplats)

    def region():
        for m16, p in prepared:
            r.SortPointsPrepared(m16); r.CalcViewDataPrepared(p); rt.Clear(); r.DrawPrepared(p, rt)

    stats = None
    for k in range(8):                                             # warm-up, two regions at least: the pair buffers grow to what the frames need
        region()
        try:
            stats = r.FrameStats()
        except _lib.GsError as ex:                                 # the last frame was truncated (the buffers have been grown): once more
            if ex.code != -6:
                raise
            stats = None
        if stats is not None and k >= 1:
            break
    if stats is None:
        raise SystemExit("the pair buffers did not settle")
    wall = []
    for _ in range(3):
        ctx.Synchronize()
        t0 = time.perf_counter()
        region()
        ctx.Synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / frames)
    r.SetProfiling(frames)
    region()
    ctx.Synchronize()
    st = r.StageTimes()
    out = {"leg": name, "library": "the parent commit's (GSPLAT_LIB)" if os.environ.get("GSPLAT_LIB") else "this commit's", "splats": n, "selected": selected, "frames_per_region": frames,
           "wall_ms_per_frame": {"min": min(wall), "median": statistics.median(wall), "regions": wall},
           "stage_ms": {k: round(float(getattr(st, k)), 4) for k in ("calc_distances_ms", "sort_ms", "calc_view_ms", "bin_ms", "pair_sort_ms", "blend_ms", "total_ms")},
           "tile_pairs_last_frame": int(stats.tile_pairs), "visible_splats_last_frame": int(stats.visible_splats), "pair_capacity": int(stats.pair_capacity)}
    r.OnDisable(); rt.Dispose(); ctx.Dispose()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libgsplat_hip.so built from the parent commit")
    ap.add_argument("--config", default="C2")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "highlight_timing.json"))
    ap.add_argument("--leg", choices=LEGS, help="(internal) run one leg in this process and print its JSON line")
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.leg, args.frames, args.config)))
        return 0
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("highlight_timing.py needs --parent-lib: the parent commit's libgsplat_hip.so")
    runs = []
    for name in ("parent", "off", "parent", "off", "on_nothing_selected", "on_1_percent_selected", "on_all_selected"):
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop("GSPLAT_LIB", None)
        if name == "parent":
            env["GSPLAT_LIB"] = os.path.abspath(args.parent_lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--frames", str(args.frames), "--config", args.config],
                           env=env, capture_output=True, text=True, timeout=420)
        line = next((l for l in p.stdout.splitlines() if l.startswith("{")), None)
        if p.returncode != 0 or line is None:                      # whatever it was, nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"leg {name} failed with exit status {p.returncode}")
        runs.append(json.loads(line))
        print(line, flush=True)
    med = lambda name: [x["wall_ms_per_frame"]["median"] for x in runs if x["leg"] == name]
    blend = lambda name: [x["stage_ms"]["blend_ms"] for x in runs if x["leg"] == name]
    view = lambda name: [x["stage_ms"]["calc_view_ms"] for x in runs if x["leg"] == name]
    par, off = med("parent"), med("off")
    base = statistics.mean(off)
    out = {
        "what": "scripts/highlight_timing.py: C2 frames with and without the selection highlight; wall ms per frame = median of three un-instrumented regions",
        "config": args.config, "frames_per_region": args.frames,
        "a_off_vs_parent": {"parent_ms": par, "off_ms": off, "parent_spread_ms": abs(par[0] - par[1]), "off_minus_parent_ms": statistics.mean(off) - statistics.mean(par),
                            "parent_calc_view_ms": view("parent"), "off_calc_view_ms": view("off"), "parent_blend_ms": blend("parent"), "off_blend_ms": blend("off"),
                            "note": "the kernels a frame without highlight launches are instruction for instruction the parent's (compared by disassembly)"},
        "b_on": {name: {"wall_ms": med(name)[0], "times_off": med(name)[0] / base, "calc_view_ms": view(name)[0], "blend_ms": blend(name)[0],
                        "selected": next(x["selected"] for x in runs if x["leg"] == name), "tile_pairs": next(x["tile_pairs_last_frame"] for x in runs if x["leg"] == name)}
                 for name in LEGS[2:]},
        "off_tile_pairs": next(x["tile_pairs_last_frame"] for x in runs if x["leg"] == "off"),
        "runs": runs,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_off_vs_parent", "b_on")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
