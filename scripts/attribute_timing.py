#!/usr/bin/env python3
"""GPU time of the attribute tools at the bench scene's size (bench.py --config C2: 6,131,954 splats), as a Medium and as a
VeryHigh renderer:

  - gs_renderer_edit_select_range and gs_renderer_edit_attribute_stats per attribute class (position, scale, opacity, colour), with the bytes each must
    read and the resulting GB/s; in the same run the alive count of the export (alive_count_kernel and its scan over the chunks) over the same
    renderer as the floor: it reads positions, deleted words and cutouts only
  - gs_renderer_edit_attribute_histogram at 64, 256 and 4096 bins on three value distributions -- the scene's own opacity, uniform, all equal (the last
    two: the VeryHigh asset with its opacity texels rewritten) -- in each of the contention variants the kernel has: plain LDS atomics, the wave
    fold over up to four bins or over the leader's bin only, per-wave LDS copies (where bins + 3 <= 1024), fold and copies
  - gs_renderer_edit_attribute_ranks, with the sort's share of it
  - for scale, the host route the feature replaces: gs_renderer_edit_export_data to host memory, a numpy threshold, gs_renderer_edit_upload_selected_bits

Kernel times come from events INSIDE one call on the context's stream (gs_attribute_times_for_scripts, a measurement aid the library exports beside
its ABI, bound here); call times are the wall clock around the ABI call itself.  Medians of --runs after --warmup.  A record, not a gate: nothing is
asserted about times.

    timeout 1100 python scripts/attribute_timing.py [--config C2] [--splats N] [--skip-host-route] [--out profiles/attribute_timing.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unitygaussiansplatting_amd import _lib, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext, SplatAttribute  # noqa: E402

CLASSES = (("position", SplatAttribute.PosX), ("scale", SplatAttribute.Volume), ("opacity", SplatAttribute.Opacity), ("colour", SplatAttribute.Luma))
VARIANTS = (("plain LDS atomics", 0), ("wave fold, up to four bins", 1), ("per-wave LDS copies", 2), ("wave fold of four + per-wave copies", 3), ("wave fold, the leader's bin only", 4))
VEC_BYTES = {0: 12, 1: 6, 2: 4, 3: 2}
TEXEL_BYTES = {0: 16, 1: 8, 2: 4, 3: 1}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-host-route", action="store_true", help="leave out the export-to-host comparison (it moves 248 bytes per splat)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attribute_timing.json"))
    args = ap.parse_args()

    import numpy as np
    f32 = np.float32
    if not os.path.exists("/dev/kfd"):
        raise SystemExit("attribute_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    ctx = GpuContext(0)
    lib = _lib.lib()
    aid = lib.gs_attribute_times_for_scripts
    aid.restype = C.c_int32
    aid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_uint32, C.c_int32, C.POINTER(C.c_float)]

    def kernel_ms(r, op, attr, lo=0.0, hi=1.0, bins=64, variant=-1, scope=0, before=None):
        """(median GPU ms of the call's kernels, median ms of the sort inside it) by the events inside the call"""
        ms = (C.c_float * 2)()
        rows = []
        for k in range(args.warmup + args.runs):
            if before:
                before()
            _lib.check(aid(r._r_h, op, int(attr), None, scope, lo, hi, bins, variant, ms), "gs_attribute_times_for_scripts")
            if k >= args.warmup:
                rows.append((float(ms[0]), float(ms[1])))
        return statistics.median(a for a, _ in rows), statistics.median(b for _, b in rows)

    def wall_ms(fn, before=None):
        """median wall-clock ms of fn() followed by the stream's drain"""
        out = []
        for k in range(args.warmup + args.runs):
            if before:
                before()
            ctx.Synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.Synchronize()
            if k >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    def hist_matrix(r, what):
        rows = {}
        for bins in (64, 256, 4096):
            row = {}
            for name, variant in VARIANTS:
                if (variant & 2) and bins + 3 > 1024:
                    continue                                       # the copies would not fit: the kernel runs the variant without them
                row[name] = kernel_ms(r, 2, SplatAttribute.Opacity, 0.0, 1.0, bins, variant)[0]
            row["call_ms (the library's variant)"] = wall_ms(lambda: r.EditAttributeHistogram(SplatAttribute.Opacity, 0.0, 1.0, bins))
            rows[str(bins)] = row
            print(f"[attribute_timing] histogram {what} bins={bins}: {row}", flush=True)
        return rows

    def class_bytes(asset, cls):
        """bytes per splat the class's values are decoded from (the 64-byte chunk header shared by 256 splats included where there is one)"""
        chunk = 64.0 / 256.0 if asset.chunkData is not None and len(asset.chunkData) else 0.0
        if cls == "position":
            return VEC_BYTES[int(asset.posFormat)] + chunk
        if cls == "scale":
            return VEC_BYTES[int(asset.scaleFormat)] + chunk
        return TEXEL_BYTES[int(asset.colorFormat)] + chunk

    n = 0
    presets = {}
    assets = {}
    for quality in ("Medium", "VeryHigh"):
        t0 = time.perf_counter()
        asset = creator.CreateAssetFromSplatsNative(raw, quality, name=f"{cfg.key}_{quality}")
        print(f"[attribute_timing] {quality} asset of {asset.splatCount} splats in {time.perf_counter() - t0:.1f} s", flush=True)
        assets[quality] = asset
        n = asset.splatCount
        r = GaussianSplatRenderer(ctx, asset)
        r.CreateResourcesForAsset()
        r.EnsureEditingBuffers()
        r.EditDeselectAll()
        res = {"floor: alive count of the export (positions, deleted words, cutouts)": {"kernel_ms": kernel_ms(r, 5, 0)[0], "bytes_per_splat": class_bytes(asset, "position")}}
        floor = res["floor: alive count of the export (positions, deleted words, cutouts)"]
        floor["GB_per_s"] = floor["bytes_per_splat"] * n / (floor["kernel_ms"] * 1e-3) / 1e9
        for cls, attr in CLASSES:
            st = r.EditAttributeStats(attr)
            lo, hi = float(st.vmin), float(st.vmin) + 0.5 * (float(st.vmax) - float(st.vmin))
            b = class_bytes(asset, cls)
            sel_k = kernel_ms(r, 0, attr, lo, hi, before=r.EditDeselectAll)[0]
            stats_k = kernel_ms(r, 1, attr)[0]
            row = {"attribute": attr.name, "bytes_per_splat": b,
                   "select_range": {"kernel_ms": sel_k, "GB_per_s": (b + 0.125) * n / (sel_k * 1e-3) / 1e9, "x floor": sel_k / floor["kernel_ms"],
                                    "call_ms": wall_ms(lambda: lib.gs_renderer_edit_select_range(r._r_h, int(attr), None, lo, hi, 0), before=r.EditDeselectAll)},
                   "stats": {"kernel_ms": stats_k, "GB_per_s": b * n / (stats_k * 1e-3) / 1e9, "x floor": stats_k / floor["kernel_ms"],
                             "call_ms": wall_ms(lambda: r.EditAttributeStats(attr))}}
            r.EditDeselectAll()
            res[cls] = row
            print(f"[attribute_timing] {quality} {cls}: {row}", flush=True)
        res["histogram of the scene's own opacity over [0, 1]: kernel_ms by bins and contention variant"] = hist_matrix(r, f"{quality} own opacity")
        k, s = kernel_ms(r, 3, SplatAttribute.Opacity)
        res["ranks (opacity, one rank)"] = {"kernels_ms": k, "sort_ms": s, "sort share": s / k if k else None,
                                            "call_ms": wall_ms(lambda: r.EditAttributeRanks(SplatAttribute.Opacity, [n // 2]))}
        print(f"[attribute_timing] {quality} ranks: {res['ranks (opacity, one rank)']}", flush=True)
        if quality == "VeryHigh" and not args.skip_host_route:
            # the host route, once each (the export moves 248 bytes per splat): export to host memory, a numpy threshold on the opacity column, the bit mask back
            t0 = time.perf_counter(); rec = r.EditExportData(); t1 = time.perf_counter()
            mask = np.packbits(rec[:, 54] < f32(0.0), bitorder="little"); t2 = time.perf_counter()
            words = np.zeros((n + 31) // 32, np.uint32); words.view(np.uint8)[:len(mask)] = mask
            r.UploadSelectedBits(words); ctx.Synchronize(); t3 = time.perf_counter()
            res["host route: export_data, numpy threshold, upload_selected_bits (one run)"] = {
                "export_ms": (t1 - t0) * 1e3, "numpy_ms": (t2 - t1) * 1e3, "upload_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3, "bytes_exported": int(rec.nbytes)}
            print(f"[attribute_timing] host route: {res['host route: export_data, numpy threshold, upload_selected_bits (one run)']}", flush=True)
            del rec
        presets[quality] = res
        r.DisposeResourcesForAsset()
    del raw

    # uniform and all-equal opacities: the VeryHigh asset with the alpha of every colour texel rewritten (no chunks: the texel IS the linear opacity)
    base = assets["VeryHigh"]
    distributions = {}
    for what in ("uniform", "all equal"):
        texels = np.ascontiguousarray(base.colorData).view(f32).reshape(-1, 4).copy()
        texels[:, 3] = np.random.default_rng(1).random(len(texels), dtype=f32) if what == "uniform" else f32(0.375)
        asset = dataclasses.replace(base, colorData=texels.view(np.uint8).reshape(-1))
        r = GaussianSplatRenderer(ctx, asset)
        r.CreateResourcesForAsset()
        distributions[what] = hist_matrix(r, what)
        r.DisposeResourcesForAsset()
        del texels, asset

    name, cus, _ = ctx.DeviceInfo()
    out = {"device": name, "cus": cus, "config": cfg.key, "label": cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), "splats": n, "runs": args.runs,
           "warmup": args.warmup, "presets": presets,
           "histogram of VeryHigh opacity texels rewritten, over [0, 1]: kernel_ms by bins and contention variant": distributions,
           "timing": "kernel_ms: events inside the call around its kernels on the context's stream; call_ms: wall clock of the ABI call and the stream's drain; "
                     "medians; thresholds: none (a record)"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    ctx.Dispose()
    return 0


if __name__ == "__main__":
    sys.exit(main())
