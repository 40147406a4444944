#!/usr/bin/env python3
"""GPU time of the SPZ export (csrc/gs_export.hip) at the bench asset's size (bench.py --config C2: 6,131,954 splats, Medium):

  * its kernels -- export_count + export_scan, the alive list + its bounds, export_spz over every alive splat into the transient column
    buffer -- bracketed by events on the context's stream (the library's undeclared hook gs_export_spz_kernel_times_for_scripts, bound here),
    medians of --runs after --warmup, and the rate at which export_spz writes the body;
  * the wall time of ExportSpzBody (the kernels + the columns through the two pinned slices into host memory) and of ExportSpzFile at gzip levels
    1 and -1, beside ExportPlyFile of the same renderer in the same run, each ending in the call's own synchronise.

A record, not a gate: nothing is asserted about the times.

    timeout 1500 python scripts/export_spz_timing.py [--config C2] [--splats N] [--out profiles/export_spz_timing.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unitygaussiansplatting_amd import _abi, _lib, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--file-runs", type=int, default=2, help="repetitions of every file export (deflate of the whole body: seconds each)")
    ap.add_argument("--dir", default="", help="where the files are written (and removed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_spz_timing.json"))
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        raise SystemExit("export_spz_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    say = lambda *a: print(*a, file=sys.stderr, flush=True)
    say("building the asset ...")
    raw = scenes.make_config_splats(cfg, args.splats)
    asset = creator.CreateAssetFromSplatsNative(raw, cfg.quality, name=cfg.key)
    del raw
    ctx = GpuContext(0)
    r = GaussianSplatRenderer(ctx, asset)
    r.CreateResourcesForAsset()
    lib = _lib.lib()
    p, s = r.ExportParams(False), r.SpzParams()
    ms, alive, size = (C.c_float * 3)(), C.c_uint32(0), C.c_uint64(0)
    hook = lib.gs_export_spz_kernel_times_for_scripts              # a measurement aid outside the ABI of gsplat_c.h: bound here, nowhere else
    hook.restype = C.c_int32
    hook.argtypes = [C.c_void_p, C.POINTER(_abi.gs_export_params), C.POINTER(_abi.gs_spz_params), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]

    def once():
        _lib.check(hook(r._r_h, C.byref(p), C.byref(s), ms, C.byref(alive), C.byref(size)), "gs_export_spz_kernel_times_for_scripts")
        return list(ms)

    say("kernels ...")
    for _ in range(args.warmup):
        once()
    t = [once() for _ in range(args.runs)]
    med = [statistics.median(x[k] for x in t) for k in range(3)]
    out = {"count_scan_ms": med[0], "alive_bounds_ms": med[1], "pack_ms": med[2], "pack_min_ms": min(x[2] for x in t), "pack_max_ms": max(x[2] for x in t),
           "alive": int(alive.value), "body_bytes": int(size.value), "pack_body_gb_per_s_at_median": int(size.value) / (med[2] * 1e-3) / 1e9}

    def wall(fn, runs):
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        return ts, res

    say("body ...")
    walls, (body, _, fract) = wall(lambda: r.ExportSpzBody(), 3)
    out["body"] = {"wall_s": walls, "bytes": int(len(body)), "fract_bits": fract, "gb_per_s_best": len(body) / min(walls) / 1e9}
    del body
    d = args.dir or tempfile.gettempdir()
    files = {}
    for level in (1, -1):
        path = os.path.join(d, f"export_spz_timing_{level}.spz")
        say("file, level", level, "...")
        walls, count = wall(lambda: r.ExportSpzFile(path, level=level), args.file_runs)
        files[f"spz_level_{level}"] = {"wall_s": walls, "alive": count, "file_bytes": os.path.getsize(path), "body_mb_per_s_best": int(size.value) / min(walls) / 1e6}
        os.remove(path)
    path = os.path.join(d, "export_spz_timing.ply")
    walls, count = wall(lambda: r.ExportPlyFile(path), 3)
    files["ply"] = {"wall_s": walls, "alive": count, "file_bytes": os.path.getsize(path)}
    os.remove(path)
    out["files"] = files
    name, cus, _ = ctx.DeviceInfo()
    out.update(device=name, cus=cus, config=cfg.key, label=cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), splats=asset.splatCount,
               runs=args.runs, warmup=args.warmup,
               timing="kernels: events on the context's stream around each group of launches; walls: a host clock around calls that block; thresholds: none (a record)")
    r.DisposeResourcesForAsset()
    ctx.Dispose()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
