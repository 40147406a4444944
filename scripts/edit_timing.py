#!/usr/bin/env python3
"""GPU time of the two edit calls a drag of the selection rectangle repeats -- gs_renderer_edit_update_selection (CSSelectionUpdate) and
gs_renderer_edit_info (CSInitEditData + CSUpdateEditData + the 36-byte readback) -- at the bench asset's size (bench.py --config C2: 6,131,954
splats, Medium = chunked Norm11 positions), next to the bytes each kernel must move: positions + chunk headers + the words it reads and writes.

Timed with events on the context's stream (a torch stream handed to gs_context_create), one pair around every call: the median of --runs calls
after --warmup calls, and the mean of a back-to-back batch of update_selection calls between one pair (launch gaps included, host latency not).
The three calls a drag of a move / rotate / scale tool repeats -- gs_renderer_edit_translate_selection, _rotate_selection, _scale_selection -- are
timed the same way on the same splats as an fp32, chunk-less asset (VeryHigh: the only kind the reference's kernels write), with the rectangle's
selection and with everything selected; the first call, which makes the renderer's private copy of the blobs, is recorded on its own.
A record, not a gate: nothing is asserted about the times.

    timeout 900 python scripts/edit_timing.py [--config C2] [--splats N] [--out profiles/edit_timing.json]"""
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
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_timing.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("edit_timing.py needs a GPU; there is no CPU fallback")
    cfg = scenes.CONFIGS[args.config]
    raw = scenes.make_config_splats(cfg, args.splats)
    asset = creator.CreateAssetFromSplatsNative(raw, cfg.quality, name=cfg.key)
    n = asset.splatCount
    words = (n + 31) // 32

    stream = torch.cuda.Stream()
    ctx = GpuContext(0, stream=stream.cuda_stream)
    r = GaussianSplatRenderer(ctx, asset)
    r.CreateResourcesForAsset()
    lib = _lib.lib()
    cam = camera.Camera(position=scenes.orbit_eye(cfg.eye_radius, cfg.eye_elev_deg, 30.0), pixelWidth=cfg.width, pixelHeight=cfg.height, fieldOfView=cfg.fov_y)
    P = r.FrameParams(cam)
    W, H = float(cfg.width), float(cfg.height)
    rect = (C.c_float * 4)(0.25 * W, 0.25 * H, 0.75 * W, 0.75 * H)
    info = _abi.gs_edit_info()

    def update():
        _lib.check(lib.gs_renderer_edit_update_selection(r._r_h, C.byref(P), rect, 0), "gs_renderer_edit_update_selection")

    def edit_info():
        _lib.check(lib.gs_renderer_edit_info(r._r_h, C.byref(info)), "gs_renderer_edit_info")

    def timed(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record(stream); fn(); b.record(stream)
        stream.synchronize()
        return [a.elapsed_time(b) for a, b in ev]                  # ms

    r.EditSelectAll(); r.EditDeselectAll()                         # the buffers exist; nothing selected
    timed(update, args.warmup); timed(edit_info, args.warmup)
    r.EditDeselectAll(); r.EditStoreSelectionMouseDown()
    t_info_none = timed(edit_info, args.runs)                      # nothing selected: no bounds reduction, no atomics
    t_update = timed(update, args.runs)
    t_info = timed(edit_info, args.runs)                           # the rectangle's selection
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(args.batch):
        update()
    b.record(stream)
    stream.synchronize()
    t_batch = a.elapsed_time(b) / args.batch
    edit_info()
    selected = int(info.selected)
    r.EditSelectAll()
    t_info_all = timed(edit_info, args.runs)                       # everything selected: every workgroup sends its nine atomics to the same nine words
    r.EditDeselectAll()

    pos_bytes, chunk_bytes = int(len(asset.posData)), int(len(asset.chunkData)) if asset.chunkData is not None else 0
    bytes_update = pos_bytes + chunk_bytes + 2 * words * 4          # mouse-down words in, selected words out
    bytes_info = pos_bytes + chunk_bytes + words * 4                # selected words in (no deleted buffer in this run); 36 bytes out
    med_u, med_i = statistics.median(t_update), statistics.median(t_info)
    name, cus, _ = ctx.DeviceInfo()
    r.DisposeResourcesForAsset()

    # ---- the transforms, on the same splats as an fp32, chunk-less asset -----------------------------------------------------------------------
    import numpy as np
    asset32 = creator.CreateAssetFromSplatsNative(raw, "VeryHigh", name=cfg.key + "_fp32")
    del raw
    r = GaussianSplatRenderer(ctx, asset32)
    r.CreateResourcesForAsset()
    tool = camera.Transform(position=(0.2, -0.1, 0.3), rotation=(0.1, 0.2, 0.05, 0.9695), scale=(1.25, 0.75, -1.5))
    fp = lambda v: np.ascontiguousarray(v, np.float32).reshape(-1)
    arrs = {"delta": fp((0.01, -0.02, 0.005)), "centre": fp((0.3, -0.2, 0.1)), "l2w": fp(tool.localToWorldMatrix), "w2l": fp(tool.worldToLocalMatrix),
            "quat": fp((0.18257419, 0.36514837, 0.54772256, 0.73029674)), "scale": fp((1.01, 0.99, 1.0))}
    ptr = {k: v.ctypes.data_as(C.POINTER(C.c_float)) for k, v in arrs.items()}

    def translate():
        _lib.check(lib.gs_renderer_edit_translate_selection(r._r_h, ptr["delta"]), "gs_renderer_edit_translate_selection")

    def rotate():
        _lib.check(lib.gs_renderer_edit_rotate_selection(r._r_h, ptr["centre"], ptr["l2w"], ptr["w2l"], ptr["quat"]), "gs_renderer_edit_rotate_selection")

    def scale():
        _lib.check(lib.gs_renderer_edit_scale_selection(r._r_h, ptr["centre"], ptr["l2w"], ptr["w2l"], ptr["scale"]), "gs_renderer_edit_scale_selection")

    r.EditDeselectAll(); r.EditStoreSelectionMouseDown()
    _lib.check(lib.gs_renderer_edit_update_selection(r._r_h, C.byref(P), rect, 0), "gs_renderer_edit_update_selection")
    r.EditStorePosMouseDown(); r.EditStoreOtherMouseDown()
    t_first = {"translate (copies pos)": timed(translate, 1)[0], "rotate (copies other)": timed(rotate, 1)[0]}
    transforms = {}
    for label in ("the rectangle's selection", "everything selected"):
        if label == "everything selected":
            r.EditSelectAll()
        edit_info()
        sel_n = int(info.selected)
        for fn in (translate, rotate, scale):
            timed(fn, args.warmup)
            t = timed(fn, args.runs)
            # a selected splat: 12 B of pos in and out (rotate and scale read the mouse-down copy), rotate 4 B of other in and out; every splat: its selection bit
            per = 24 + (8 if fn is rotate else 0)
            transforms.setdefault(fn.__name__, {})[label] = {"selected": sel_n, "median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                                                              "bytes_to_move": min(sel_n, n) * per + words * 4}
    out = {
        "device": name, "cus": cus, "config": cfg.key, "label": cfg.label + (f" [--splats {args.splats}]" if args.splats else ""),
        "splats": n, "words": words, "pos_format": str(asset.posFormat), "runs": args.runs, "warmup": args.warmup,
        "selected_by_the_rectangle": selected,
        "update_selection": {"median_ms": med_u, "min_ms": min(t_update), "max_ms": max(t_update), "batch_of": args.batch, "batch_mean_ms": t_batch,
                             "bytes_to_move": bytes_update, "gb_per_s_at_median": bytes_update / (med_u * 1e-3) / 1e9},
        "edit_info": {"median_ms": med_i, "min_ms": min(t_info), "max_ms": max(t_info), "bytes_to_move": bytes_info,
                      "gb_per_s_at_median": bytes_info / (med_i * 1e-3) / 1e9,
                      "median_ms_nothing_selected": statistics.median(t_info_none), "median_ms_everything_selected": statistics.median(t_info_all),
                      "note": "two kernels + a 36-byte device-to-host copy + the stream synchronise inside the call; median_ms is with the rectangle's selection"},
        "transforms": {"asset": "the same splats, VeryHigh (fp32 positions, scales and SH, no chunks)", "first_call_ms": t_first, "calls": transforms,
                       "note": "bytes_to_move counts whole records of the selected splats; the hardware moves the 64- / 128-byte lines they lie in"},
        "timing": "events on the context's stream around every call; thresholds: none (a record)",
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
