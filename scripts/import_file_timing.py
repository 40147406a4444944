#!/usr/bin/env python3
"""Wall time from a file on disk to a device asset: the bench scene (bench.py --config C2: 6,131,954 splats; --splats N where
scratch disk is short, the count is written into the file) is written to a temporary PLY and SPZ, and in one process, for the targets Medium and
VeryLow, two routes are timed over each file, the file in the page cache:

  * arrays: the readers' route -- creator.ReadPLYNative / ReadSPZNative (gs_ply_open / gs_spz_open: the six arrays on the host, copied out) +
    creator.CreateGpuAssetFromSplats (gs_import_encode_to_asset, host arrays);
  * file:   creator.CreateGpuAssetFromFile (gs_splat_file_open + gs_import_file_to_asset: the file's own bytes are the source).

Each is the median of --runs after --warmup.  Next to the wall times, the event-bracketed stages of both imports -- upload, bounds, Morton codes + the
two sorts, palette (VeryLow only), encode -- through the library's undeclared hooks gs_import_gpu_stage_times_for_scripts and
gs_import_file_stage_times_for_scripts, bound here: the encode from rows / columns is to be read next to the six-array encode of the same run.

A record, not a gate: nothing is asserted about the times.

    timeout 900 python scripts/import_file_timing.py [--config C2] [--splats N] [--tmp DIR] [--out profiles/import_file_timing.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unitygaussiansplatting_amd import _lib, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd._abi import gs_import_formats, gs_import_input, gs_splat_file_info  # noqa: E402
from unitygaussiansplatting_amd.renderer import GpuContext  # noqa: E402

STAGES = ("upload_ms", "bounds_ms", "sort_ms", "palette_ms", "encode_ms")


def wall_ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slice-bytes", type=int, default=0)
    ap.add_argument("--tmp", default=None, help="where the two files are written (default: the system's temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "import_file_timing.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("import_file_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    n = len(raw)
    stream = torch.cuda.Stream()
    ctx = GpuContext(0, stream=stream.cuda_stream)
    lib = _lib.lib()
    array_hook, file_hook = lib.gs_import_gpu_stage_times_for_scripts, lib.gs_import_file_stage_times_for_scripts      # measurement aids outside the ABI: bound here
    array_hook.restype = file_hook.restype = C.c_int32
    array_hook.argtypes = [C.c_void_p, C.POINTER(gs_import_input), C.c_uint32, C.POINTER(gs_import_formats), C.c_float * 5]
    file_hook.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(gs_import_formats), C.c_uint32, C.c_float * 5]
    out = {}
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        paths = {"ply": os.path.join(tmp, "scene.ply"), "spz": os.path.join(tmp, "scene.spz")}
        creator.WritePLY(paths["ply"], raw)
        creator.WriteSPZ(paths["spz"], raw)
        del raw
        out["file_bytes"] = {k: os.path.getsize(p) for k, p in paths.items()}
        for kind, path in paths.items():
            read = creator.ReadPLYNative if kind == "ply" else creator.ReadSPZNative
            linearize = kind == "ply"
            # the stages of both imports, once per target: the arrays of the reader on the host, and the open file
            arrays = read(path)
            host = [np.ascontiguousarray(a, np.float32) for a in (arrays.pos, arrays.dc0, arrays.sh.reshape(n, 45), arrays.opacity, arrays.scale, arrays.rot)]
            inp = gs_import_input(n, *[a.ctypes.data for a in host])
            fh, info = C.c_void_p(), gs_splat_file_info()
            _lib.check(lib.gs_splat_file_open(path.encode(), C.byref(fh), C.byref(info)), "gs_splat_file_open")
            for quality in ("Medium", "VeryLow"):
                fp, fs, fc, fsh = (int(v) for v in creator.QUALITY[quality])
                fmt = gs_import_formats(fp, fs, fc, fsh, int(linearize), 1)
                ms = (C.c_float * 5)()

                def array_stages():
                    _lib.check(array_hook(ctx._h, C.byref(inp), 0, C.byref(fmt), ms), "gs_import_gpu_stage_times_for_scripts")
                    return [float(v) for v in ms]

                def file_stages():
                    _lib.check(file_hook(ctx._h, fh, C.byref(fmt), args.slice_bytes, ms), "gs_import_file_stage_times_for_scripts")
                    return [float(v) for v in ms]

                for route, stages_once in (("arrays", array_stages), ("file", file_stages)):
                    for _ in range(args.warmup):
                        stages_once()
                    st = [stages_once() for _ in range(args.runs)]
                    rec = {name: statistics.median(x[k] for x in st) for k, name in enumerate(STAGES)}
                    rec["stages_sum_ms"] = sum(rec[name] for name in STAGES)
                    out[f"{kind}_{quality.lower()}_{route}_stages"] = rec
                    print(kind, quality, route, "stages", json.dumps(rec), flush=True)
            lib.gs_splat_file_close(fh)
            del arrays, host, inp
            # the wall time from the path to the asset
            for quality in ("Medium", "VeryLow"):
                def arrays_route():
                    creator.CreateGpuAssetFromSplats(read(path), quality, linearize=linearize, context=ctx).Dispose()

                def file_route():
                    creator.CreateGpuAssetFromFile(path, quality, slice_bytes=args.slice_bytes, context=ctx).Dispose()

                rec = {"splats": n, "stride": info.stride, "body_bytes": info.body_bytes}
                for route, fn in (("arrays", arrays_route), ("file", file_route)):
                    for _ in range(args.warmup):
                        fn()
                    wall = [wall_ms(fn) for _ in range(args.runs)]
                    rec.update({f"{route}_wall_ms": statistics.median(wall), f"{route}_wall_min_ms": min(wall), f"{route}_wall_max_ms": max(wall)})
                out[f"{kind}_{quality.lower()}_wall"] = rec
                print(kind, quality, "wall", json.dumps(rec), flush=True)
    name, cus, _ = ctx.DeviceInfo()
    out.update(device=name, cus=cus, config=cfg.key, label=cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), splats=n, runs=args.runs,
               warmup=args.warmup, slice_bytes=args.slice_bytes,
               timing="wall: time.perf_counter around the whole route, path in, asset out, the file in the page cache; stages: events on the context's "
                      "stream inside one import (the file route's upload includes the reads of the file it overlaps); thresholds: none (a record)")
    ctx.Dispose()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
