#!/usr/bin/env python3
"""GPU time of the import on the GPU (gs_import_encode_to_asset, csrc/gs_bake.hip) on the bench scene (bench.py --config C2:
6,131,954 splats) if memory allows, else of --splats; the count is written into the file.  Targets Medium and VeryLow, each from host arrays
(memory_kind 0) and from device tensors (memory_kind 1).  For each, after a warm-up, medians of --runs:

  * the event-bracketed time of each stage -- upload, bounds, Morton codes + the two sorts, palette (SH rows + the Lloyd loop; VeryLow only),
    encode (+ the SH table) -- through the library's undeclared hook gs_import_gpu_stage_times_for_scripts, bound here;
  * the wall time of a whole CreateGpuAssetFromSplats (the call blocks: synchronise, allocate, upload, zero-fill, the kernels, read the bounds back);

and once per target (--host-runs) the host route it replaces: CreateAssetFromSplatsNative plus the upload of gs_asset_create.

A record, not a gate: nothing is asserted about the times.

    timeout 1100 python scripts/import_gpu_timing.py [--config C2] [--splats N] [--out profiles/import_gpu_timing.json]"""
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
from unitygaussiansplatting_amd._abi import gs_import_formats, gs_import_input  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext  # noqa: E402

STAGES = ("upload_ms", "bounds_ms", "sort_ms", "palette_ms", "encode_ms")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "import_gpu_timing.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("import_gpu_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    n = len(raw)
    stream = torch.cuda.Stream()
    ctx = GpuContext(0, stream=stream.cuda_stream)
    lib = _lib.lib()
    hook = lib.gs_import_gpu_stage_times_for_scripts               # a measurement aid outside the ABI of gsplat_c.h: bound here, nowhere else
    hook.restype = C.c_int32
    hook.argtypes = [C.c_void_p, C.POINTER(gs_import_input), C.c_uint32, C.POINTER(gs_import_formats), C.c_float * 5]
    host = [np.ascontiguousarray(a, np.float32) for a in (raw.pos, raw.dc0, raw.sh.reshape(n, 45), raw.opacity, raw.scale, raw.rot)]
    dev = [torch.from_numpy(a).to("cuda:0") for a in host]
    torch.cuda.synchronize()
    out = {}
    for quality in ("Medium", "VeryLow"):
        fp, fs, fc, fsh = (int(v) for v in creator.QUALITY[quality])
        fmt = gs_import_formats(fp, fs, fc, fsh, 1, 1)
        for kind, arrays in ((0, host), (1, dev)):
            label = f"{quality.lower()}_memory_kind_{kind}"
            inp = gs_import_input(n, *[a.ctypes.data if kind == 0 else a.data_ptr() for a in arrays])
            source = raw if kind == 0 else creator.InputSplatData(*dev)
            ms = (C.c_float * 5)()

            def stages_once():
                _lib.check(hook(ctx._h, C.byref(inp), kind, C.byref(fmt), ms), "gs_import_gpu_stage_times_for_scripts")
                return [float(v) for v in ms]

            def call_once():
                t0 = time.perf_counter()
                g = creator.CreateGpuAssetFromSplats(source, quality, context=ctx)
                dt = (time.perf_counter() - t0) * 1e3
                g.Dispose()
                return dt

            for _ in range(args.warmup):
                stages_once(); call_once()
            st = [stages_once() for _ in range(args.runs)]
            wall = [call_once() for _ in range(args.runs)]
            rec = {"splats": n, "target_formats": (fp, fs, fc, fsh), "memory_kind": kind}
            rec.update({name: statistics.median(x[k] for x in st) for k, name in enumerate(STAGES)})
            rec.update(stages_sum_ms=sum(rec[name] for name in STAGES), call_wall_ms=statistics.median(wall), call_wall_min_ms=min(wall), call_wall_max_ms=max(wall))
            print(label, json.dumps(rec), flush=True)
            out[label] = rec
        hosts = []
        for _ in range(args.host_runs):
            t0 = time.perf_counter()
            a = creator.CreateAssetFromSplatsNative(raw, quality, name="host_route", context=ctx if fsh > 3 else None)     # a palette's assignment passes on the GPU: the faster host route
            t1 = time.perf_counter()
            r = GaussianSplatRenderer(ctx, a)
            r.CreateResourcesForAsset()
            ctx.Synchronize()
            t2 = time.perf_counter()
            r.DisposeResourcesForAsset()
            hosts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
            del a
        if hosts:
            out[f"{quality.lower()}_host_route_ms"] = {"import_encode": statistics.median(h[0] for h in hosts), "asset_and_renderer_create": statistics.median(h[1] for h in hosts),
                                                       "total": statistics.median(sum(h) for h in hosts), "runs": len(hosts),
                                                       "note": "CreateAssetFromSplatsNative (multi-threaded host C++; a Cluster* palette's assignment passes on the GPU, "
                                                               "gs_import_encode_on) + gs_asset_create and gs_renderer_create: the same bytes"}
            print(quality, "host route", json.dumps(out[f"{quality.lower()}_host_route_ms"]), flush=True)
    name, cus, _ = ctx.DeviceInfo()
    out.update(device=name, cus=cus, config=cfg.key, label=cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), runs=args.runs, warmup=args.warmup,
               timing="stages: events on the context's stream inside one call; wall: time.perf_counter around CreateGpuAssetFromSplats; thresholds: none (a record)")
    ctx.Dispose()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
