#!/usr/bin/env python3
"""GPU time of the island tools -- gs_renderer_edit_select_islands and gs_renderer_edit_grow_selection -- at the bench scene's size (bench.py --config
C2: 6,131,954 splats) as a VeryHigh renderer, at the two radii of profiles/neighbour_timing.json: the one at which the median neighbour count of an
alive splat is 16, and one ten times smaller.

Stage times come from events INSIDE one call (gs_islands_stage_times_for_scripts, a measurement aid the library exports beside its ABI, bound here):
the grid build (list, origin, keys, the two sorts, the records), cc_link, cc_flatten, the reduction with the per-index outputs, the kernels that apply.
Medians of --runs calls after --warmup.  The whole call's wall-clock time -- allocations, the readback of the list's length, the host's
synchronisation -- is written next to them, and so are the number of components and the largest one.  In the same process
gs_renderer_edit_neighbour_counts at cap 65535 is timed the same way (gs_neighbour_stage_times_for_scripts): its walk enumerates the runs cc_link
enumerates, so its count stage is what the link stage is read against.  A record, not a gate: nothing is asserted about times.

    timeout 900 python scripts/islands_timing.py [--config C2] [--splats N] [--out profiles/islands_timing.json]"""
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

STAGES = ("grid_build_ms", "link_ms", "flatten_ms", "reduce_and_outputs_ms", "apply_ms")
NB_STAGES = ("list_and_origin_ms", "keys_and_sorts_ms", "gather_ms", "count_ms", "apply_ms")
RADII = (("median count 16", 0.10995174199342728), ("ten times smaller", 0.010995173826813698))     # profiles/neighbour_timing.json


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "islands_timing.json"))
    args = ap.parse_args()

    import numpy as np
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    asset = creator.CreateAssetFromSplatsNative(raw, "VeryHigh", name=cfg.key + "_fp32")
    del raw
    n = asset.splatCount
    if not os.path.exists("/dev/kfd"):
        raise SystemExit("islands_timing.py needs a GPU; there is no CPU fallback")

    ctx = GpuContext(0)
    r = GaussianSplatRenderer(ctx, asset)
    r.CreateResourcesForAsset()
    lib, h = _lib.lib(), r._r_h
    aid = lib.gs_islands_stage_times_for_scripts
    aid.restype = C.c_int32
    aid.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    nb_aid = lib.gs_neighbour_stage_times_for_scripts
    nb_aid.restype = C.c_int32
    nb_aid.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    out_counts = np.zeros(n, np.uint32)

    def medians(names, call, before=None) -> dict:
        ms = (C.c_float * 5)()
        rows, walls = [], []
        for k in range(args.warmup + args.runs):
            if before:
                before()
                ctx.Synchronize()
            t0 = time.perf_counter()
            call(ms)
            wall = (time.perf_counter() - t0) * 1e3
            if k >= args.warmup:
                rows.append([float(v) for v in ms]); walls.append(wall)
        med = {name: statistics.median(row[i] for row in rows) for i, name in enumerate(names)}
        return dict(med, gpu_stages_sum_ms=sum(med.values()), wall_median_ms=statistics.median(walls))

    def selected() -> int:
        r.EnsureEditingBuffers()
        r.UpdateEditCountsAndBounds()
        return int(r.editSelectedSplats)

    legs = {}
    for label, radius in RADII:
        listed = C.c_uint32(0)
        tests = C.c_uint64(0)
        labels, sizes = r.EditComponents(radius)
        alive = labels != 0xFFFFFFFF
        leg = {"radius": float(np.float32(radius)), "components": int((labels[alive] == np.flatnonzero(alive)).sum()), "largest_component": int(sizes.max()),
               "splats in components below 16": int((sizes[alive] < 16).sum())}
        seed = np.zeros((n + 31) // 32, np.uint32)
        big = int(np.flatnonzero(sizes == sizes.max())[0])
        seed[big >> 5] = np.uint32(1) << np.uint32(big & 31)

        def islands(ms):
            _lib.check(aid(h, C.c_float(radius), 0, 16, ms, C.byref(listed)), "gs_islands_stage_times_for_scripts")

        def grow(ms):
            _lib.check(aid(h, C.c_float(radius), 1, 0, ms, C.byref(listed)), "gs_islands_stage_times_for_scripts")

        def counts(ms):
            _lib.check(nb_aid(h, C.c_float(radius), 65535, 0, out_counts.ctypes.data, ms, C.byref(tests), C.byref(listed)), "gs_neighbour_stage_times_for_scripts")

        leg["select_islands, min_size = 16"] = dict(medians(STAGES, islands, r.EditDeselectAll), selected=selected())
        leg["grow_selection, one seed in the largest component"] = dict(medians(STAGES, grow, lambda: r.UploadSelectedBits(seed)), selected=selected())
        leg["neighbour_counts, cap = 65535"] = dict(medians(NB_STAGES, counts), distance_tests=int(tests.value))
        link, count = leg["select_islands, min_size = 16"]["link_ms"], leg["neighbour_counts, cap = 65535"]["count_ms"]
        leg["link_ms / count_ms"] = link / count if count > 0 else None
        leg["listed_splats"] = int(listed.value)
        legs[label] = leg
    name, cus, _ = ctx.DeviceInfo()
    out = {
        "device": name, "cus": cus, "config": cfg.key, "label": cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), "splats": n,
        "asset": "VeryHigh (fp32 positions, no chunks)", "runs": args.runs, "warmup": args.warmup, "legs": legs,
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
