#!/usr/bin/env python3
"""GPU time of the screen mask and of the selection through it:

  - gs_mask_fill_polygon of a 4,096-vertex lasso at 1200x797 and at 3840x2160
  - gs_mask_stroke of a 1,000-segment stroke of radius 20 at both sizes
  - gs_renderer_edit_update_selection_mask through the 1200x797 lasso on the bench scene (bench.py --config C2: 6,131,954 splats, Medium), and in the
    same process and run gs_renderer_edit_update_selection with the lasso's bounding rectangle as the baseline, with their ratio

Every call is asynchronous, so two numbers per call: `call_ms`, the wall clock of one call and the stream's drain (what a host that waits for the result
sees: launch and synchronisation latency included), and `stream_ms`, the wall clock of --batch calls enqueued back to back and one drain, divided by
--batch (what the call adds to a busy stream).  Medians of --runs after --warmup.  A record, not a gate: nothing is asserted about times.

    timeout 600 python scripts/mask_timing.py [--config C2] [--splats N] [--out profiles/mask_timing.json]"""
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

from unitygaussiansplatting_amd import _lib, camera, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext  # noqa: E402

SIZES = ((1200, 797), (3840, 2160))


def lasso(w: int, h: int, count: int, seed: int):
    """a seeded star-shaped outline around the screen centre that covers about a third of the screen"""
    import numpy as np
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.random(count)) * 2 * np.pi
    rad = 0.25 + 0.2 * rng.random(count)
    return np.stack([w * (0.5 + rad * np.cos(ang)), h * (0.5 + rad * np.sin(ang))], axis=1).astype(np.float32)


def stroke(w: int, h: int, points: int, seed: int):
    """a seeded smooth scribble across the screen: `points` - 1 segments of a few pixels each"""
    import numpy as np
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, points)
    f = rng.integers(2, 7, 4)
    x = 0.5 + 0.42 * np.sin(2 * np.pi * f[0] * t + 0.3) * np.cos(2 * np.pi * f[1] * t)
    y = 0.5 + 0.42 * np.cos(2 * np.pi * f[2] * t + 1.1) * np.sin(2 * np.pi * f[3] * t + 0.2)
    return np.stack([w * x, h * y], axis=1).astype(np.float32)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_timing.json"))
    args = ap.parse_args()

    import numpy as np
    if not os.path.exists("/dev/kfd"):
        raise SystemExit("mask_timing.py needs a GPU; there is no CPU fallback")
    ctx = GpuContext(0)

    def timed(fn, before=None):
        """(call_ms, stream_ms) of fn: medians"""
        one, many = [], []
        for k in range(args.warmup + args.runs):
            if before:
                before()
            ctx.Synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.Synchronize()
            t1 = time.perf_counter()
            if before:
                before()
            ctx.Synchronize()
            t2 = time.perf_counter()
            for _ in range(args.batch):
                fn()
            ctx.Synchronize()
            t3 = time.perf_counter()
            if k >= args.warmup:
                one.append((t1 - t0) * 1e3)
                many.append((t3 - t2) * 1e3 / args.batch)
        return {"call_ms": statistics.median(one), "stream_ms": statistics.median(many)}

    drawing = {}
    for w, h in SIZES:
        m = ctx.CreateScreenMask(w, h)
        outline, scribble = lasso(w, h, 4096, 1), stroke(w, h, 1001, 2)
        row = {"fill_polygon, 4096 vertices": timed(lambda: m.FillPolygon(outline), before=m.Clear),
               "stroke, 1000 segments, radius 20": timed(lambda: m.Stroke(scribble, 20.0), before=m.Clear),
               "clear": timed(m.Clear)}
        m.Clear(); m.FillPolygon(outline)
        row["lasso covers"] = float(m.Download().mean())
        m.Clear(); m.Stroke(scribble, 20.0)
        row["stroke covers"] = float(m.Download().mean())
        drawing[f"{w}x{h}"] = row
        print(f"[mask_timing] {w}x{h}: {row}", flush=True)
        m.Dispose()

    cfg = scenes.CONFIGS[args.config]
    t0 = time.perf_counter()
    asset = creator.CreateAssetFromSplatsNative(scenes.make_config_splats(cfg, args.splats), cfg.quality, name=cfg.key)
    print(f"[mask_timing] {cfg.quality} asset of {asset.splatCount} splats in {time.perf_counter() - t0:.1f} s", flush=True)
    r = GaussianSplatRenderer(ctx, asset)
    r.CreateResourcesForAsset()
    cam = camera.Camera(position=scenes.orbit_eye(cfg.eye_radius, cfg.eye_elev_deg, 30.0), fieldOfView=cfg.fov_y, pixelWidth=cfg.width, pixelHeight=cfg.height)
    P = r.FrameParams(cam)
    w, h = cfg.width, cfg.height
    outline = lasso(w, h, 4096, 1)
    m = ctx.CreateScreenMask(w, h)
    m.FillPolygon(outline)
    r.EnsureEditingBuffers()
    r.EditDeselectAll()
    r.EditStoreSelectionMouseDown()
    lib = _lib.lib()
    x0, x1, y0, y1 = float(outline[:, 0].min()), float(outline[:, 0].max()), float(outline[:, 1].min()), float(outline[:, 1].max())
    rect = np.array([x0, h - y1, x1, h - y0], np.float32)          # y up from the bottom edge
    rect_p = rect.ctypes.data_as(C.POINTER(C.c_float))
    through_mask = timed(lambda: _lib.check(lib.gs_renderer_edit_update_selection_mask(r._r_h, C.byref(P), m._h, 0), "gs_renderer_edit_update_selection_mask"))
    sel_mask = int(np.unpackbits(r.DownloadEditBits()[0].view(np.uint8)).sum())
    through_rect = timed(lambda: _lib.check(lib.gs_renderer_edit_update_selection(r._r_h, C.byref(P), rect_p, 0), "gs_renderer_edit_update_selection"))
    sel_rect = int(np.unpackbits(r.DownloadEditBits()[0].view(np.uint8)).sum())
    composed = timed(lambda: r.EditSelectPolygon(P, outline))
    selection = {"update_selection_mask (4096-vertex lasso)": dict(through_mask, selected=sel_mask),
                 "update_selection (the lasso's bounding rectangle; baseline)": dict(through_rect, selected=sel_rect),
                 "ratio mask / rectangle": {k: through_mask[k] / through_rect[k] for k in ("call_ms", "stream_ms")},
                 "EditSelectPolygon (clear, fill, select, counts and bounds read back)": composed,
                 "mask_bytes": int(m.rowWords * 4 * h)}
    print(f"[mask_timing] selection: {selection}", flush=True)
    name, cus, _ = ctx.DeviceInfo()
    out = {"device": name, "cus": cus, "config": cfg.key, "label": cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), "splats": asset.splatCount,
           "screen": [w, h], "runs": args.runs, "warmup": args.warmup, "batch": args.batch, "drawing": drawing, "selection": selection,
           "timing": "call_ms: wall clock of one call and the stream's drain; stream_ms: wall clock of `batch` calls enqueued back to back and one drain, per call; "
                     "medians; thresholds: none (a record)"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    m.Dispose()
    r.DisposeResourcesForAsset()
    ctx.Dispose()
    return 0


if __name__ == "__main__":
    sys.exit(main())
