#!/usr/bin/env python3
"""Host against GPU for the importer's nearest-mean assignment (gs_import_assign_clusters: csrc/gs_import.cpp assign_clusters
against csrc/gs_cluster.hip), in one process, whole calls -- upload of the means and points, kernel, download of the indices.

Timed shapes: the training pass of a Low import (200,000 x 16,384), the same at Cluster64k (200,000 x 65,536), and the final
pass of a bicycle-sized scene (6.1 M x 16,384) on the GPU alone, its host figure EXTRAPOLATED from the first shape's host rate
and labelled so.  Every timed shape asserts equal indices: all points for the first two, every 64th point of the third (the
host loop run on that subset).  If scripts/probes/valu_issue_f64 has been built, its fp64 multiply + add issue rate is recorded
next to the calls' own rates.

    timeout 900 python scripts/import_cluster_timing.py [--out profiles/import_cluster_timing.json] [--gpu-only]

--gpu-only skips the host runs and the asserts (for a profiler run around the GPU calls, e.g. rocprofv3 --kernel-trace --stats)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unitygaussiansplatting_amd import creator  # noqa: E402
from unitygaussiansplatting_amd.renderer import GpuContext  # noqa: E402

DIM = 45


def make(n: int, k: int, seed: int):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, DIM), dtype=np.float32)
    x *= np.float32(0.1)                                              # SH coefficients of a trained scene are of this order
    means = x[(np.arange(k, dtype=np.int64) * n) // k].copy()         # the importer's own seeding: a stride sample of the points
    return x, means


def timed(fn, reps: int):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def probe_roof():
    exe = os.path.join(ROOT, "scripts", "probes", "valu_issue_f64")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    return rows if out.returncode == 0 and rows else None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "import_cluster_timing.json"))
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--big-n", type=int, default=6_100_000)
    args = ap.parse_args()

    ctx = GpuContext(0)
    name, cus, _ = ctx.DeviceInfo()
    res = {"device": name, "cus": cus, "host_threads_available": len(os.sched_getaffinity(0)), "shapes": [],
           "what_is_timed": "whole gs_import_assign_clusters calls (means + points up, kernel, indices down); wall clock of the calling thread"}
    creator.AssignClusters(*make(1024, 256, 1), context=ctx)          # loads the code object, warms the context

    host_rate = None
    for n, k in ((200_000, 16_384), (200_000, 65_536)):
        x, m = make(n, k, n + k)
        gpu, tg = timed(lambda: creator.AssignClusters(x, m, context=ctx), 3)
        row = {"n": n, "k": k, "multiply_adds": n * k * DIM, "gpu_s": tg, "gpu_best_s": min(tg),
               "gpu_gmadds_per_s": n * k * DIM / min(tg) / 1e9}
        if not args.gpu_only:
            host, th = timed(lambda: creator.AssignClusters(x, m), 1)
            assert np.array_equal(host, gpu), f"{(host != gpu).sum()} indices differ at n = {n}, K = {k}"
            row.update(host_s=th[0], host_gmadds_per_s=n * k * DIM / th[0] / 1e9, speedup=th[0] / min(tg), indices_equal=True,
                       distinct_indices=int(len(np.unique(gpu))))
            if host_rate is None:
                host_rate = n * k * DIM / th[0]
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)

    n, k = args.big_n, 16_384
    x, m = make(n, k, 3)
    gpu, tg = timed(lambda: creator.AssignClusters(x, m, context=ctx), 2)
    row = {"n": n, "k": k, "multiply_adds": n * k * DIM, "gpu_s": tg, "gpu_best_s": min(tg), "gpu_gmadds_per_s": n * k * DIM / min(tg) / 1e9}
    if not args.gpu_only:
        sub = np.arange(0, n, 64)
        host = creator.AssignClusters(x[sub], m)
        assert np.array_equal(host, gpu[sub]), f"{(host != gpu[sub]).sum()} indices differ at n = {n}, K = {k} (every 64th point)"
        row.update(host_s_EXTRAPOLATED=n * k * DIM / host_rate, host_extrapolated_from="the host rate of the first shape, same process",
                   speedup_EXTRAPOLATED=n * k * DIM / host_rate / min(tg), indices_equal_on="every 64th point (%d points)" % len(sub),
                   distinct_indices=int(len(np.unique(gpu))))
    res["shapes"].append(row)
    print(json.dumps(row), flush=True)

    roof = probe_roof()
    if roof:
        res["fp64_issue_probe"] = roof
        pair = [r for r in roof if r["kind"].startswith("v_mul_f64+") and r["waves_per_simd"] == 3]
        if pair:
            # one multiply-add of the contract = two lane-operations = 1/32 wave-instruction
            roof_madds = pair[0]["gwi_per_s"] * 1e9 * 64 / 2
            res["roof_gmadds_per_s_mul_add_3_waves_per_simd"] = roof_madds / 1e9
            for r in res["shapes"]:
                r["call_fraction_of_fp64_mul_add_roof"] = r["gpu_gmadds_per_s"] * 1e9 / roof_madds
    ctx.Dispose()
    if not args.gpu_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
