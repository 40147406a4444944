#!/usr/bin/env python3
"""GPU time of the edit history's calls -- gs_renderer_edit_checkpoint (GS_HIST_TRANSFORM with rigid transforms on, plus SELECTION and DELETED),
gs_renderer_edit_undo, gs_renderer_edit_redo -- at the bench scene's size (bench.py --config C2: 6,131,954 splats) as a VeryHigh renderer, for four
selections: nothing, one splat, the half-screen rectangle of profiles/edit_timing.json, everything.  In the same process: the device-to-device copy
of the whole pos + other + SH blobs, which is what the three mouse-down stores do today and what a snapshot undo would have to do per step; and the
bytes an entry holds against the bytes of that copy.

Timed with events on the context's stream (a torch stream handed to gs_context_create), one pair around every call: the median of --runs calls after
--warmup calls.  A checkpoint blocks for its 4-byte count, so its span holds one host round trip; its wall-clock time is written next to it.  Every
cycle is checkpoint, undo, redo, clear, so that the stack never holds more than one entry.  The three blobs are private before the first cycle (one
rigid rotate), so that undo and redo swap all three kinds.  A record, not a gate: nothing is asserted about the times.

    timeout 900 python scripts/undo_timing.py [--config C2] [--splats N] [--out profiles/undo_timing.json]"""
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

from unitygaussiansplatting_amd import _abi, _lib, camera, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undo_timing.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("undo_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    asset = creator.CreateAssetFromSplatsNative(raw, "VeryHigh", name=cfg.key + "_fp32")
    del raw
    n = asset.splatCount
    words = (n + 31) // 32

    stream = torch.cuda.Stream()
    ctx = GpuContext(0, stream=stream.cuda_stream)
    r = GaussianSplatRenderer(ctx, asset)
    r.rigidTransforms = True
    r.CreateResourcesForAsset()
    lib, h = _lib.lib(), r._r_h
    cam = camera.Camera(position=scenes.orbit_eye(cfg.eye_radius, cfg.eye_elev_deg, 30.0), pixelWidth=cfg.width, pixelHeight=cfg.height, fieldOfView=cfg.fov_y)
    P = r.FrameParams(cam)
    rect = (C.c_float * 4)(0.0, 0.0, 0.5 * float(cfg.width), float(cfg.height))      # the left half of the screen
    tool = camera.Transform(position=(0.2, -0.1, 0.3), rotation=(0.1, 0.2, 0.05, 0.9695))
    fp = lambda v: np.ascontiguousarray(v, np.float32).reshape(-1)
    arrs = [fp((0.3, -0.2, 0.1)), fp(tool.localToWorldMatrix), fp(tool.worldToLocalMatrix), fp((0.18257419, 0.36514837, 0.54772256, 0.73029674))]
    ptrs = [v.ctypes.data_as(C.POINTER(C.c_float)) for v in arrs]
    what = _abi.GS_HIST_TRANSFORM | _abi.GS_HIST_SELECTION | _abi.GS_HIST_DELETED

    def call(name, *a):
        _lib.check(getattr(lib, name)(h, *a), name)

    def span(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        b.record(stream)
        return a, b, wall

    def stats(ev):
        stream.synchronize()
        t = [a.elapsed_time(b) for a, b, _ in ev]
        return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}

    def store_all():
        call("gs_renderer_edit_store_pos_mouse_down"); call("gs_renderer_edit_store_other_mouse_down"); call("gs_renderer_edit_store_sh_mouse_down")

    # everything private: one rigid rotate of everything
    r.EditSelectAll()
    store_all()
    call("gs_renderer_edit_rotate_selection", *ptrs)
    ev = [span(store_all) for _ in range(args.warmup + args.runs)][args.warmup:]
    copy = stats(ev)
    copy_bytes = (12 + 16 + 192) * n
    copy.update({"bytes_copied": copy_bytes, "gb_per_s_at_median (read + write)": 2 * copy_bytes / (copy["median_ms"] * 1e-3) / 1e9})

    r.EditHistoryEnable(8 << 30)
    one = np.zeros(words, np.uint32)
    one[words // 2] = 1 << 7
    info = _abi.gs_edit_info()
    legs = {}
    for label in ("nothing selected", "one splat", "the rectangle's selection", "everything selected"):
        if label == "nothing selected":
            r.EditDeselectAll()
        elif label == "one splat":
            r.UploadSelectedBits(one)
        elif label == "everything selected":
            r.EditSelectAll()
        else:
            r.EditDeselectAll(); r.EditStoreSelectionMouseDown()
            call("gs_renderer_edit_update_selection", C.byref(P), rect, 0)
        call("gs_renderer_edit_info", C.byref(info))
        cp, un, re = [], [], []
        top = None
        for k in range(args.warmup + args.runs):
            c = span(lambda: call("gs_renderer_edit_checkpoint", what))
            top = r.EditHistoryInfo()
            u = span(lambda: call("gs_renderer_edit_undo"))
            d = span(lambda: call("gs_renderer_edit_redo"))
            stream.synchronize()
            call("gs_renderer_edit_history_clear")
            if k >= args.warmup:
                cp.append(c); un.append(u); re.append(d)
        leg = {"selected (edit_info, tail bits counted)": int(info.selected), "journalled_splats": int(top.top_splats), "entry_bytes": int(top.top_bytes),
               "entry_bytes / whole_copy_bytes": int(top.top_bytes) / copy_bytes,
               "checkpoint": dict(stats(cp), wall_median_ms=statistics.median(w for _, _, w in cp)), "undo": stats(un), "redo": stats(re)}
        swapped = 2 * (8 * words + int(top.top_splats) * (4 + 2 * (12 + 16 + 192)))
        leg["undo"]["bytes_to_move"] = swapped
        legs[label] = leg
    name, cus, _ = ctx.DeviceInfo()
    out = {
        "device": name, "cus": cus, "config": cfg.key, "label": cfg.label + (f" [--splats {args.splats}]" if args.splats else ""), "splats": n, "words": words,
        "asset": "VeryHigh (fp32 positions, scales and SH, no chunks)", "runs": args.runs, "warmup": args.warmup, "rectangle": "the left half of the screen",
        "checkpoint_what": "GS_HIST_TRANSFORM (rigid transforms on: POS | OTHER | SH) | GS_HIST_SELECTION | GS_HIST_DELETED",
        "whole_blob_copy (the three mouse-down stores: what a snapshot undo would copy per step)": copy, "legs": legs,
        "timing": "events on the context's stream around every call; a checkpoint's span holds its host round trip; thresholds: none (a record)",
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
