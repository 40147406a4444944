#!/usr/bin/env python3
"""GPU time of the calls a drag of the rotate / scale tool repeats, with gs_renderer_edit_set_rigid_transforms off and on, and of the third
mouse-down copy (gs_renderer_edit_store_sh_mouse_down), at the bench scene's size (bench.py --config C2: 6,131,954 splats) as a VeryHigh asset --
fp32 positions, scales and SH, no chunks: the only kind the transform kernels write.  Next to every time: the bytes the call must move and the
bandwidth that implies.  With the setting on a selected splat costs 180 B of SH in and 180 B out on top of its position (12 + 12), its rotation
word (4 + 4) and, for a uniform scale, its scales (12 + 12); every splat costs its selection bit.

Timed with events on the context's stream (a torch stream handed to gs_context_create), one pair around every call: the median of --runs calls
after --warmup calls, for the half-screen rectangle's selection and for everything selected.  The first rigid rotate, which makes the private
SH blob, is recorded on its own.

--compare FILE: the setting-off legs of another run of this script -- the parent commit's library through GSPLAT_LIB, in the same GPU session --
are written next to this run's, with both runs' min / max.  The setting-off kernels have the resources they had, so
the two should lie inside each other's run-to-run spread.  A library without the two entry points runs the setting-off legs only.
A record, not a gate: nothing is asserted about the times.

    timeout 900 python scripts/rigid_timing.py [--config C2] [--splats N] [--compare parent.json] [--out profiles/rigid_timing.json]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unitygaussiansplatting_amd import _abi, _lib, camera, creator, scenes  # noqa: E402
from unitygaussiansplatting_amd.renderer import GaussianSplatRenderer, GpuContext  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=list(scenes.CONFIGS))
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (the result is labelled)")
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--compare", default="", help="the JSON of another run (the parent commit's library): its setting-off legs are written next to this run's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rigid_timing.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rigid_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    asset = creator.CreateAssetFromSplatsNative(raw, "VeryHigh", name=cfg.key + "_fp32")
    del raw
    n = asset.splatCount
    words = (n + 31) // 32

    stream = torch.cuda.Stream()
    ctx = GpuContext(0, stream=stream.cuda_stream)
    r = GaussianSplatRenderer(ctx, asset)
    r.CreateResourcesForAsset()
    lib = _lib.lib()
    has_rigid = hasattr(lib, "gs_renderer_edit_set_rigid_transforms") and hasattr(lib, "gs_renderer_edit_store_sh_mouse_down")
    cam = camera.Camera(position=scenes.orbit_eye(cfg.eye_radius, cfg.eye_elev_deg, 30.0), pixelWidth=cfg.width, pixelHeight=cfg.height, fieldOfView=cfg.fov_y)
    P = r.FrameParams(cam)
    W, H = float(cfg.width), float(cfg.height)
    rect = (C.c_float * 4)(0.0, 0.0, 0.5 * W, H)                   # the left half of the screen
    info = _abi.gs_edit_info()
    tool = camera.Transform(position=(0.2, -0.1, 0.3), rotation=(0.1, 0.2, 0.05, 0.9695))
    fp = lambda v: np.ascontiguousarray(v, np.float32).reshape(-1)
    arrs = {"centre": fp((0.3, -0.2, 0.1)), "l2w": fp(tool.localToWorldMatrix), "w2l": fp(tool.worldToLocalMatrix),
            "quat": fp((0.18257419, 0.36514837, 0.54772256, 0.73029674)), "scale": fp((1.01, 1.01, 1.01))}
    ptr = {k: v.ctypes.data_as(C.POINTER(C.c_float)) for k, v in arrs.items()}

    def rotate():
        _lib.check(lib.gs_renderer_edit_rotate_selection(r._r_h, ptr["centre"], ptr["l2w"], ptr["w2l"], ptr["quat"]), "gs_renderer_edit_rotate_selection")

    def scale():
        _lib.check(lib.gs_renderer_edit_scale_selection(r._r_h, ptr["centre"], ptr["l2w"], ptr["w2l"], ptr["scale"]), "gs_renderer_edit_scale_selection")

    def store_sh():
        _lib.check(lib.gs_renderer_edit_store_sh_mouse_down(r._r_h), "gs_renderer_edit_store_sh_mouse_down")

    def set_rigid(on):
        _lib.check(lib.gs_renderer_edit_set_rigid_transforms(r._r_h, int(on)), "gs_renderer_edit_set_rigid_transforms")

    def timed(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record(stream); fn(); b.record(stream)
        stream.synchronize()
        return [a.elapsed_time(b) for a, b in ev]                  # ms

    def leg(fn, selected, per_selected, fixed):
        timed(fn, args.warmup)
        t = timed(fn, args.runs)
        med = statistics.median(t)
        moved = min(selected, n) * per_selected + fixed
        return {"selected": selected, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes_to_move": moved, "gb_per_s_at_median": moved / (med * 1e-3) / 1e9}

    r.EditDeselectAll(); r.EditStoreSelectionMouseDown()
    _lib.check(lib.gs_renderer_edit_update_selection(r._r_h, C.byref(P), rect, 0), "gs_renderer_edit_update_selection")
    r.EditStorePosMouseDown(); r.EditStoreOtherMouseDown()
    rotate(); scale()                                              # the private pos / other blobs exist from here on
    first_rigid_ms = None
    legs = {}
    for label in ("the rectangle's selection", "everything selected"):
        if label == "everything selected":
            r.EditSelectAll()
        _lib.check(lib.gs_renderer_edit_info(r._r_h, C.byref(info)), "gs_renderer_edit_info")
        sel = int(info.selected)
        out = legs.setdefault(label, {})
        out["rotate, setting off"] = leg(rotate, sel, 12 + 12 + 4 + 4, words * 4)
        out["scale, setting off"] = leg(scale, sel, 12 + 12, words * 4)
        if not has_rigid:
            continue
        out["store sh mouse down"] = leg(store_sh, 0, 0, 2 * 192 * n)      # a whole-blob copy: read and written once
        set_rigid(True)
        if first_rigid_ms is None:
            first_rigid_ms = timed(rotate, 1)[0]                   # copies the SH blob
        out["rotate, setting on"] = leg(rotate, sel, 180 + 180 + 12 + 12 + 4 + 4, words * 4)
        out["scale, setting on"] = leg(scale, sel, 12 + 12 + 12 + 12, words * 4)
        set_rigid(False)
    name, cus, _ = ctx.DeviceInfo()
    out = {
        "device": name, "cus": cus, "config": cfg.key, "label": cfg.label + (f" [--splats {args.splats}]" if args.splats else ""),
        "library": os.path.basename(_lib.LIB_PATH) if os.environ.get("GSPLAT_LIB") else "this commit's", "rigid_entry_points": has_rigid,
        "splats": n, "words": words, "asset": "VeryHigh (fp32 positions, scales and SH, no chunks)", "runs": args.runs, "warmup": args.warmup,
        "rectangle": "the left half of the screen", "legs": legs, "first_rigid_rotate_ms (copies the SH blob)": first_rigid_ms,
        "sh_bytes": 192 * n, "note": "bytes_to_move counts whole fields of the selected splats; the hardware moves the 64- / 128-byte lines they lie in",
        "timing": "events on the context's stream around every call; thresholds: none (a record)",
    }
    if args.compare:
        with open(args.compare) as f:
            other = json.load(f)
        cmp = {}
        for label, mine in legs.items():
            for key in ("rotate, setting off", "scale, setting off"):
                a, b = mine[key], other["legs"][label][key]
                cmp[f"{key}; {label}"] = {"this_median_ms": a["median_ms"], "this_min_max_ms": [a["min_ms"], a["max_ms"]],
                                          "parent_median_ms": b["median_ms"], "parent_min_max_ms": [b["min_ms"], b["max_ms"]],
                                          "this_median_inside_parent_spread": b["min_ms"] <= a["median_ms"] <= b["max_ms"]}
        out["setting_off_against_parent"] = {"parent_library": other.get("library"), "legs": cmp}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    r.DisposeResourcesForAsset()
    ctx.Dispose()
    return 0


if __name__ == "__main__":
    sys.exit(main())
