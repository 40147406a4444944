#!/usr/bin/env python3
"""GPU time of the floater tool -- gs_renderer_edit_select_sparse with min_neighbours = 4 against gs_renderer_edit_neighbour_counts with cap = 65535 -- at
the bench scene's size (bench.py --config C2: 6,131,954 splats) as a VeryHigh renderer, at two radii: the one at which the median count of an alive
splat is nearest 16 (found here by bisection over gs_renderer_edit_neighbour_counts), and one ten times smaller.

Stage times come from events INSIDE one call (gs_neighbour_stage_times_for_scripts, a measurement aid the library exports beside its ABI, bound here):
list + origin, keys + the two sorts, the gather of the records, the count (the walk), the apply.  Medians of --runs calls after --warmup.  The whole
call's wall-clock time -- allocations, the readback of the list's length, the host's synchronisation -- is written next to them.  The walk also counts
the distance tests it makes: tests per second of the count kernel is that over its median time.  A record, not a gate: nothing is asserted about times.

    timeout 900 python scripts/neighbour_timing.py [--config C2] [--splats N] [--out profiles/neighbour_timing.json]"""
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

STAGES = ("list_and_origin_ms", "keys_and_sorts_ms", "gather_ms", "count_ms", "apply_ms")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbour_timing.json"))
    args = ap.parse_args()

    import numpy as np
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    asset = creator.CreateAssetFromSplatsNative(raw, "VeryHigh", name=cfg.key + "_fp32")
    pos = np.ascontiguousarray(raw.pos, np.float32).reshape(-1, 3)
    extent = float(np.linalg.norm(pos.max(axis=0) - pos.min(axis=0)))
    del raw
    n = asset.splatCount
    if not os.path.exists("/dev/kfd"):
        raise SystemExit("neighbour_timing.py needs a GPU; there is no CPU fallback")

    ctx = GpuContext(0)
    r = GaussianSplatRenderer(ctx, asset)
    r.CreateResourcesForAsset()
    lib, h = _lib.lib(), r._r_h
    aid = lib.gs_neighbour_stage_times_for_scripts
    aid.restype = C.c_int32
    aid.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    out_counts = np.zeros(n, np.uint32)

    def median_count(radius: float) -> float:
        c = r.EditNeighbourCounts(radius)
        return float(np.median(c[c != 0xFFFFFFFF]))

    # the radius whose median count is nearest 16: grow from a small one (a radius far too large makes every walk long), then bisect on a log scale
    lo = extent * 2.0 ** -14
    search = []
    while median_count(lo) >= 16.0:
        lo *= 0.5
    hi = lo
    while True:
        hi *= 2.0
        m = median_count(hi)
        search.append((hi, m))
        if m >= 16.0:
            break
        lo = hi
    for _ in range(10):
        mid = (lo * hi) ** 0.5
        m = median_count(mid)
        search.append((mid, m))
        lo, hi = (mid, hi) if m < 16.0 else (lo, mid)
    radius16 = min(search, key=lambda s: abs(s[1] - 16.0))[0]

    def leg(radius: float, limit: int, select: int) -> dict:
        ms = (C.c_float * 5)()
        tests, listed = C.c_uint64(0), C.c_uint32(0)
        rows, walls = [], []
        for k in range(args.warmup + args.runs):
            if select:
                r.EditDeselectAll()
                ctx.Synchronize()
            t0 = time.perf_counter()
            _lib.check(aid(h, C.c_float(radius), limit, select, out_counts.ctypes.data, ms, C.byref(tests), C.byref(listed)), "gs_neighbour_stage_times_for_scripts")
            wall = (time.perf_counter() - t0) * 1e3
            if k >= args.warmup:
                rows.append([float(v) for v in ms]); walls.append(wall)
        med = {name: statistics.median(row[i] for row in rows) for i, name in enumerate(STAGES)}
        res = dict(med, gpu_stages_sum_ms=sum(med.values()), wall_median_ms=statistics.median(walls), listed_splats=int(listed.value),
                   distance_tests=int(tests.value), distance_tests_per_s_of_the_count_kernel=float(tests.value) / (med["count_ms"] * 1e-3) if med["count_ms"] > 0 else None)
        if select:
            r.EnsureEditingBuffers()
            r.UpdateEditCountsAndBounds()
            res["selected"] = int(r.editSelectedSplats)
        else:
            alive = out_counts[out_counts != 0xFFFFFFFF]
            res["median_count"] = float(np.median(alive))
            res["counts_histogram (0, 1-3, 4-15, 16-63, 64-255, 256+)"] = [int(v) for v in np.histogram(alive, [0, 1, 4, 16, 64, 256, 1 << 32])[0]]
        return res

    legs = {}
    for label, radius in (("median count near 16", radius16), ("ten times smaller", radius16 / 10.0)):
        legs[label] = {"radius": float(np.float32(radius)), "radius / scene diagonal": radius / extent,
                       "select_sparse, min_neighbours = 4": leg(radius, 4, 1), "neighbour_counts, cap = 65535": leg(radius, 65535, 0)}
    name, cus, _ = ctx.DeviceInfo()
    out = {
        "device": name, "cus": cus, "config": cfg.key, "label": cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), "splats": n,
        "asset": "VeryHigh (fp32 positions, no chunks)", "runs": args.runs, "warmup": args.warmup,
        "radius_search (radius, median count)": [[float(a), float(b)] for a, b in search], "legs": legs,
        "timing": "events inside the call around each stage; wall = the whole blocking call; thresholds: none (a record)",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    r.DisposeResourcesForAsset()
    ctx.Dispose()
    return 0


if __name__ == "__main__":
    sys.exit(main())
