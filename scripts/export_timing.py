#!/usr/bin/env python3
"""GPU time of the export (csrc/gs_export.hip) at the bench asset's size (bench.py --config C2: 6,131,954 splats, Medium):

  * the three kernels -- export_count, export_scan, export_records over the whole asset into device memory -- bracketed by events on the context's
    stream (the library's undeclared hook gs_export_kernel_times_for_scripts, bound here), medians of --runs after --warmup, and the write rate export_records achieves (N x 248 bytes),
    to be read against the streaming rate profiles/hbm_traffic.json holds for this box;
  * the wall time of ExportPlyFile (count + scan + batches through the pinned buffers + fwrite) into --ply-dir;
  * the same kernel times for the build in which every lane stores its own record (-DGS_EXPORT_DIRECT, unitygaussiansplatting_amd/variants/
    export_direct.so, built on demand), measured by a fresh child process of this script in the same run.

A record, not a gate: nothing is asserted about the times.

    timeout 1500 python scripts/export_timing.py [--config C2] [--splats N] [--out profiles/export_timing.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unitygaussiansplatting_amd import _lib, build, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext  # noqa: E402

RECORD = 248


def measure(args) -> dict:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("export_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    asset = creator.CreateAssetFromSplatsNative(raw, cfg.quality, name=cfg.key)
    del raw
    n = asset.splatCount
    stream = torch.cuda.Stream()
    ctx = GpuContext(0, stream=stream.cuda_stream)
    r = GaussianSplatRenderer(ctx, asset)
    r.CreateResourcesForAsset()
    lib = _lib.lib()
    p = r.ExportParams(False)
    dev = torch.empty(n * RECORD // 4, dtype=torch.float32, device="cuda")
    ms, alive = (C.c_float * 3)(), C.c_uint32(0)

    hook = lib.gs_export_kernel_times_for_scripts                  # a measurement aid outside the ABI of gsplat_c.h: bound here, nowhere else
    hook.restype = C.c_int32
    hook.argtypes = [C.c_void_p, C.POINTER(type(p)), C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]

    def once():
        _lib.check(hook(r._r_h, C.byref(p), dev.data_ptr(), n * RECORD, ms, C.byref(alive)), "gs_export_kernel_times_for_scripts")
        return list(ms)

    for _ in range(args.warmup):
        once()
    t = [once() for _ in range(args.runs)]
    med = [statistics.median(x[k] for x in t) for k in range(3)]
    out = {"count_ms": med[0], "scan_ms": med[1], "records_ms": med[2], "records_min_ms": min(x[2] for x in t), "records_max_ms": max(x[2] for x in t),
           "alive": int(alive.value), "bytes_written": int(alive.value) * RECORD,
           "records_write_gb_per_s_at_median": int(alive.value) * RECORD / (med[2] * 1e-3) / 1e9}
    if not args.child:
        path = os.path.join(args.ply_dir or tempfile.gettempdir(), "export_timing.ply")
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            count = r.ExportPlyFile(path)
            walls.append(time.perf_counter() - t0)
        size = os.path.getsize(path)
        os.remove(path)
        out["ply"] = {"wall_s": walls, "alive": count, "file_bytes": size, "gb_per_s_best": size / min(walls) / 1e9,
                      "GSPLAT_EXPORT_BATCH": os.environ.get("GSPLAT_EXPORT_BATCH", "unset: the library's default batch")}
        name, cus, _ = ctx.DeviceInfo()
        out.update(device=name, cus=cus, config=cfg.key, label=cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), splats=n)
    del dev
    r.DisposeResourcesForAsset()
    ctx.Dispose()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ply-dir", default="")
    ap.add_argument("--child", action="store_true", help="(internal) measure the library GSPLAT_LIB names and print the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_timing.json"))
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args)))
        return 0
    variant = os.path.join(os.path.dirname(build.LIB), "variants", "export_direct.so")
    deps = [os.path.join(build.CSRC, f) for f in build.SOURCES + build.HEADERS]
    if not os.path.exists(variant) or any(os.path.getmtime(d) > os.path.getmtime(variant) for d in deps):
        build.build_variant("export_direct", ["GS_EXPORT_DIRECT"])
    out = {"staged_in_lds": measure(args)}
    for k in ("device", "cus", "config", "label", "splats"):
        out[k] = out["staged_in_lds"].pop(k)
    # the variant in a fresh process of its own (a process loads one build of the library)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", args.config, "--splats", str(args.splats), "--runs", str(args.runs), "--warmup", str(args.warmup)]
    res = subprocess.run(cmd, env=dict(os.environ, GSPLAT_LIB=variant), capture_output=True, text=True, timeout=900)
    line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
    if res.returncode != 0 or not line:
        raise SystemExit(f"the variant's run failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    out["every_lane_stores_its_own_record"] = json.loads(line[0][7:])
    out["runs"], out["warmup"] = args.runs, args.warmup
    out["timing"] = "events on the context's stream between the three launches; thresholds: none (a record)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
