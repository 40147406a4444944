#!/usr/bin/env python3
"""GPU time of the bake to a Cluster* SH target (csrc/gs_bake.hip + the device-resident Lloyd loop of csrc/gs_cluster.hip; DESIGN.md sections 4.6 and
4.10): the bench asset (bench.py --config C2: 6,131,954 splats, imported as Medium) baked to Low -- Norm11 / Norm6 / Norm8x4 / Cluster16k.  Medians of
--runs calls after a warm-up:

  * the event-bracketed time of each stage through the library's undeclared hook gs_bake_cluster_stage_times_for_scripts, bound here: everything
    before the palette (count, alive list, bounds, Morton sorts), the SH rows (+ the gathers of the seeds and the subset), the assignment and the mean
    update (its sort included) of each of the four Lloyd passes on the 200,000-row subset, the final assignment over all splats, the table + encode;
  * the final assignment's fraction of the fp64 issue roof profiles/import_cluster_timing.json measured on this kind of box (2 n K 45 / time against
    that file's roof, if the file is there);
  * the wall time of a whole EditBakeAsset("Low");
  * once (--host-runs), the host route the call replaces: ExportAlive, CreateAssetFromSplatsNative("Low", context=ctx), the upload;
  * the case the mean update is bounded by, one long cluster: 200,000 splats of which 80,000 share one SH row, baked to Cluster4k (all 200,000 rows
    are the training subset), the same stage brackets.

A record, not a gate: nothing is asserted about the times.

    timeout 1100 python scripts/bake_cluster_timing.py [--config C2] [--splats N] [--out profiles/bake_cluster_timing.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bake_timing import columns  # noqa: E402
from unitygaussiansplatting_amd import _lib, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd._abi import gs_import_formats  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext  # noqa: E402

STAGES = ["sh_rows_ms"] + [f"pass{p}_{w}_ms" for p in range(4) for w in ("assign", "mean_update")] + ["final_assign_ms", "table_encode_ms", "before_palette_ms"]


def fp64_roof():
    """the measured fp64 mul + add issue roof of profiles/import_cluster_timing.json in multiply-adds per second, or None"""
    try:
        with open(os.path.join(ROOT, "profiles", "import_cluster_timing.json")) as f:
            return float(json.load(f)["roof_gmadds_per_s_mul_add_3_waves_per_simd"]) * 1e9
    except (OSError, KeyError, ValueError):
        return None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_cluster_timing.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bake_cluster_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    stream = torch.cuda.Stream()
    ctx = GpuContext(0, stream=stream.cuda_stream)
    lib = _lib.lib()
    hook = lib.gs_bake_cluster_stage_times_for_scripts             # a measurement aid outside the ABI of gsplat_c.h: bound here, nowhere else
    hook.restype = C.c_int32
    hook.argtypes = [C.c_void_p, C.POINTER(gs_import_formats), C.c_float * 12, C.POINTER(C.c_uint32)]
    asset = creator.CreateAssetFromSplatsNative(raw, "Medium", name=cfg.key + "_Medium")
    n = asset.splatCount
    r = GaussianSplatRenderer(ctx, asset)
    r.CreateResourcesForAsset()
    print("ready:", n, "splats", flush=True)
    fmt = r.BakeFormats("Low")
    K = 16384
    ms, alive = (C.c_float * 12)(), C.c_uint32(0)

    def stages_once():
        _lib.check(hook(r._r_h, C.byref(fmt), ms, C.byref(alive)), "gs_bake_cluster_stage_times_for_scripts")
        return [float(v) for v in ms]

    def call_once():
        t0 = time.perf_counter()
        g = r.EditBakeAsset("Low")
        dt = (time.perf_counter() - t0) * 1e3
        g.Dispose()
        return dt

    for _ in range(args.warmup):
        stages_once(); call_once()
    st = [stages_once() for _ in range(args.runs)]
    wall = [call_once() for _ in range(args.runs)]
    med = [statistics.median(x[k] for x in st) for k in range(12)]
    rec = {"splats": n, "alive": alive.value, "target": "Low", "table_entries": K, "subset_rows": min(alive.value, 200000)}
    rec.update(dict(zip(STAGES, med)))
    rec["stages_sum_ms"] = sum(med)
    rec.update(call_wall_ms=statistics.median(wall), call_wall_min_ms=min(wall), call_wall_max_ms=max(wall))
    madds = float(alive.value) * K * 45
    rec["final_assign_gmadds_per_s"] = madds / (med[9] * 1e-3) / 1e9
    roof = fp64_roof()
    if roof:
        rec["fp64_mul_add_roof_gmadds_per_s"] = roof / 1e9
        rec["final_assign_fraction_of_fp64_mul_add_roof"] = madds / (med[9] * 1e-3) / roof
        rec["subset_assign_fraction_of_fp64_mul_add_roof"] = float(rec["subset_rows"]) * K * 45 / (statistics.median(med[1:9:2]) * 1e-3) / roof
    print(json.dumps(rec), flush=True)
    host = []
    for _ in range(args.host_runs):
        t0 = time.perf_counter()
        rows = r.ExportAlive()
        t1 = time.perf_counter()
        back = creator.CreateAssetFromSplatsNative(columns(rows), "Low", name="host_route", context=ctx)
        t2 = time.perf_counter()
        r2 = GaussianSplatRenderer(ctx, back)
        r2.CreateResourcesForAsset()
        ctx.Synchronize()
        t3 = time.perf_counter()
        r2.DisposeResourcesForAsset()
        host.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        del rows, back
    if host:
        rec["host_route_ms"] = {"export_alive": statistics.median(h[0] for h in host), "import_encode_assignment_on_gpu": statistics.median(h[1] for h in host),
                                "asset_and_renderer_create": statistics.median(h[2] for h in host), "total": statistics.median(sum(h) for h in host),
                                "runs": len(host), "note": "the importer linearises the exported PLY-domain records again: not the same bytes as the bake"}
    r.DisposeResourcesForAsset()
    del asset, raw

    # one long cluster: every pass sums 80,000 rows in one wave, in order
    import numpy as np
    from unitygaussiansplatting_amd.asset import ColorFormat
    n_long, shared = 200_000, 80_000
    raw = scenes.make_splats(n_long, 3, 3.0)
    rows = np.random.default_rng(5).permutation(n_long)[:shared]
    raw.sh[rows] = raw.sh[rows[0]]
    r = GaussianSplatRenderer(ctx, creator.CreateAssetFromSplatsNative(raw, "VeryHigh", name="long_cluster"))
    r.CreateResourcesForAsset()
    fmt = r.BakeFormats("VeryLow", formatColor=ColorFormat.Norm8x4)
    for _ in range(args.warmup):
        stages_once()
    st = [stages_once() for _ in range(args.runs)]
    med = [statistics.median(x[k] for x in st) for k in range(12)]
    long_rec = {"splats": n_long, "alive": alive.value, "rows_sharing_one_sh": shared, "table_entries": 4096,
                "note": "the shared rows are one cluster in every pass: its wave sums at least 80,000 rows in point order"}
    long_rec.update(dict(zip(STAGES, med)))
    print(json.dumps(long_rec), flush=True)
    r.DisposeResourcesForAsset()
    name, cus, _ = ctx.DeviceInfo()
    out = {"bake_to_low": rec, "long_cluster": long_rec, "device": name, "cus": cus, "config": cfg.key, "label": cfg.label + (f" [--splats {args.splats}]" if args.splats else ""),
           "runs": args.runs, "warmup": args.warmup,
           "timing": "stages: events on the context's stream inside one call; wall: time.perf_counter around EditBakeAsset; thresholds: none (a record)"}
    ctx.Dispose()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
