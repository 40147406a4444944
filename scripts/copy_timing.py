#!/usr/bin/env python3
"""GPU time of the merge (csrc/gs_copy.hip) on a VeryHigh asset of the bench asset's count (bench.py --config C2:
6,131,954 splats) if memory allows, else of --splats; the count is written into the file:

  * the copy kernel -- every splat of one renderer into another of the same size, the exact identity -- bracketed by events on the context's
    stream (the library's undeclared hook gs_copy_kernel_time_for_scripts, bound here), medians of --runs after --warmup, with the bytes it
    reads (236 per splat) and writes (224 per splat: 12 + 16 + 16 + 180) and the write rate, to be read against the streaming rate
    profiles/hbm_traffic.json holds for this box;
  * a whole EditSetSplatCount (N -> N + 256 -> N -> ...): events on the context's stream around the call, and its wall time (the call
    synchronises, allocates a whole renderer state, zero-fills the new blobs and copies).

A record, not a gate: nothing is asserted about the times.

    timeout 1500 python scripts/copy_timing.py [--config C2] [--splats N] [--out profiles/copy_timing.json]"""
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

from unitygaussiansplatting_amd import _lib, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext  # noqa: E402

READ, WRITTEN = 12 + 16 + 16 + 192, 12 + 16 + 16 + 180


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_timing.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("copy_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    asset = creator.CreateAssetFromSplatsNative(raw, "VeryHigh", name=cfg.key + "_veryhigh")
    del raw
    n = asset.splatCount
    stream = torch.cuda.Stream()
    ctx = GpuContext(0, stream=stream.cuda_stream)
    src, dst = GaussianSplatRenderer(ctx, asset), GaussianSplatRenderer(ctx, asset)
    src.CreateResourcesForAsset()
    dst.ShareResourcesOf(src)                                      # one copy of the asset; dst's blobs become private at its first copy
    lib = _lib.lib()
    hook = lib.gs_copy_kernel_time_for_scripts                     # a measurement aid outside the ABI of gsplat_c.h: bound here, nowhere else
    hook.restype = C.c_int32
    hook.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    ms = C.c_float(0.0)

    def kernel_once() -> float:
        _lib.check(hook(src._r_h, dst._r_h, C.byref(ms)), "gs_copy_kernel_time_for_scripts")
        return float(ms.value)

    for _ in range(args.warmup):
        kernel_once()
    k = [kernel_once() for _ in range(args.runs)]
    med = statistics.median(k)
    out = {"copy_kernel": {"ms": med, "min_ms": min(k), "max_ms": max(k), "bytes_read": n * READ, "bytes_written": n * WRITTEN,
                           "write_gb_per_s_at_median": n * WRITTEN / (med * 1e-3) / 1e9, "read_plus_write_gb_per_s_at_median": n * (READ + WRITTEN) / (med * 1e-3) / 1e9}}

    def resize_once(count: int):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        dst.EditSetSplatCount(count)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    runs = min(args.runs, 10)
    t = [resize_once(n + 256 if i % 2 == 0 else n) for i in range(min(args.warmup, 2) + runs)][-runs:]
    out["set_splat_count"] = {"events_ms": statistics.median(x[0] for x in t), "wall_ms": statistics.median(x[1] for x in t), "runs": runs,
                              "what": "N -> N + 256 and back, alternately; the call blocks"}
    name, cus, _ = ctx.DeviceInfo()
    out.update(device=name, cus=cus, config=cfg.key, label=cfg.label + " as VeryHigh" + (f" [--splats {args.splats}]" if args.splats else ""), splats=n,
               runs=args.runs, warmup=args.warmup, timing="events on the context's stream; thresholds: none (a record)")
    dst.DisposeResourcesForAsset(); src.DisposeResourcesForAsset()
    ctx.Dispose()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
