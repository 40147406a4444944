#!/usr/bin/env python3
"""GPU time of the bake (csrc/gs_bake.hip) on the bench asset (bench.py --config C2: 6,131,954 splats) if memory allows, else
of --splats; the count is written into the file.  Two sources, both baked to Medium with the Morton reorder:

  * the Medium asset as imported;
  * the same scene as a VeryHigh asset after EditSetSplatCount (N + 256 and back: private blobs in the fixed VeryHigh layout).

For each, in one call after a warm-up, medians of --runs:

  * the event-bracketed time of each stage -- count + scan, alive list + bounds, Morton codes + the two sorts, encode -- through the library's
    undeclared hook gs_bake_stage_times_for_scripts, bound here;
  * the wall time of a whole EditBakeAsset (the call blocks: synchronise, count, allocate, zero-fill, the kernels, read the bounds back);
  * the encode kernel's bytes: read = the source's bytes per splat + 8 (alive, order), written = the target's bytes per splat + 64 per chunk, and the
    rate at the median, to be read against the streaming rate profiles/hbm_traffic.json holds for this box;
  * once (--host-runs), the host route the call replaces: ExportAlive + CreateAssetFromSplatsNative + the upload of gs_asset_create.

A record, not a gate: nothing is asserted about the times.

    timeout 1100 python scripts/bake_timing.py [--config C2] [--splats N] [--out profiles/bake_timing.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unitygaussiansplatting_amd import _lib, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd._abi import gs_import_formats  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext  # noqa: E402

VEC, COL, SH = (12, 6, 4, 2), (16, 8, 4, 1), {0: 192, 1: 96, 2: 60, 3: 32}


def splat_bytes(fp, fs, fc, fsh) -> int:
    return VEC[fp] + 4 + VEC[fs] + COL[fc] + SH[fsh]


def columns(rows) -> creator.InputSplatData:
    """ExportAlive's [M, 62] records as the importer's input (the PLY vertex: pos, nor, dc0, 15 R + 15 G + 15 B, opacity, scale, rot)"""
    n = len(rows)
    return creator.InputSplatData(pos=rows[:, 0:3].copy(), dc0=rows[:, 6:9].copy(), sh=rows[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1).copy(),
                                  opacity=rows[:, 54].copy(), scale=rows[:, 55:58].copy(), rot=rows[:, 58:62].copy())


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_timing.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bake_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    stream = torch.cuda.Stream()
    ctx = GpuContext(0, stream=stream.cuda_stream)
    lib = _lib.lib()
    hook = lib.gs_bake_stage_times_for_scripts                     # a measurement aid outside the ABI of gsplat_c.h: bound here, nowhere else
    hook.restype = C.c_int32
    hook.argtypes = [C.c_void_p, C.POINTER(gs_import_formats), C.c_float * 4, C.POINTER(C.c_uint32)]
    target = (2, 2, 2, 3)                                          # Medium
    out = {}
    for label, quality in (("medium_source", "Medium"), ("resized_veryhigh_source", "VeryHigh")):
        asset = creator.CreateAssetFromSplatsNative(raw, quality, name=cfg.key + "_" + quality)
        n = asset.splatCount
        src = (int(asset.posFormat), int(asset.scaleFormat), int(asset.colorFormat), int(asset.shFormat))
        r = GaussianSplatRenderer(ctx, asset)
        r.CreateResourcesForAsset()
        if quality == "VeryHigh":
            r.EditSetSplatCount(n + 256); r.EditSetSplatCount(n)
        print(label, "ready:", n, "splats", flush=True)
        fmt = r.BakeFormats("Medium")
        ms, alive = (C.c_float * 4)(), C.c_uint32(0)

        def stages_once():
            _lib.check(hook(r._r_h, C.byref(fmt), ms, C.byref(alive)), "gs_bake_stage_times_for_scripts")
            return [float(v) for v in ms]

        def call_once():
            t0 = time.perf_counter()
            g = r.EditBakeAsset("Medium")
            dt = (time.perf_counter() - t0) * 1e3
            g.Dispose()
            return dt

        for _ in range(args.warmup):
            stages_once(); call_once()
        st = [stages_once() for _ in range(args.runs)]
        wall = [call_once() for _ in range(args.runs)]
        med = [statistics.median(x[k] for x in st) for k in range(4)]
        chunks = (alive.value + 255) // 256
        rd, wr = alive.value * (splat_bytes(*src) + 8), alive.value * splat_bytes(*target) + chunks * 64
        rec = {"splats": n, "alive": alive.value, "source_formats": src, "target_formats": target,
               "count_scan_ms": med[0], "alive_bounds_ms": med[1], "sort_ms": med[2], "encode_ms": med[3], "stages_sum_ms": sum(med),
               "call_wall_ms": statistics.median(wall), "call_wall_min_ms": min(wall), "call_wall_max_ms": max(wall),
               "encode_bytes_read": rd, "encode_bytes_written": wr, "encode_read_plus_write_gb_per_s_at_median": (rd + wr) / (med[3] * 1e-3) / 1e9}
        print(label, json.dumps(rec), flush=True)
        host = []
        for _ in range(args.host_runs):
            t0 = time.perf_counter()
            rows = r.ExportAlive()
            t1 = time.perf_counter()
            back = creator.CreateAssetFromSplatsNative(columns(rows), "Medium", name="host_route")
            t2 = time.perf_counter()
            r2 = GaussianSplatRenderer(ctx, back)
            r2.CreateResourcesForAsset()
            ctx.Synchronize()
            t3 = time.perf_counter()
            r2.DisposeResourcesForAsset()
            host.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
            del rows, back
        if host:
            rec["host_route_ms"] = {"export_alive": statistics.median(h[0] for h in host), "import_encode": statistics.median(h[1] for h in host),
                                    "asset_and_renderer_create": statistics.median(h[2] for h in host), "total": statistics.median(sum(h) for h in host),
                                    "runs": len(host), "note": "the importer linearises the exported PLY-domain records again: not the same bytes as the bake"}
        out[label] = rec
        r.DisposeResourcesForAsset()
        del asset
    name, cus, _ = ctx.DeviceInfo()
    out.update(device=name, cus=cus, config=cfg.key, label=cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), runs=args.runs, warmup=args.warmup,
               timing="stages: events on the context's stream inside one call; wall: time.perf_counter around EditBakeAsset; thresholds: none (a record)")
    ctx.Dispose()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
