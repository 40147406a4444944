#!/usr/bin/env python3
"""GPU time of the two edit calls a drag of the selection rectangle repeats -- gs_renderer_edit_update_selection (CSSelectionUpdate) and
gs_renderer_edit_info (CSInitEditData + CSUpdateEditData + the 36-byte readback) -- at the bench asset's size (bench.py --config C2: 6,131,954
splats, Medium = chunked Norm11 positions), next to the bytes each kernel must move: positions + chunk headers + the words it reads and writes.

Timed with events on the context's stream (a torch stream handed to gs_context_create), one pair around every call: the median of --runs calls
after --warmup calls, and the mean of a back-to-back batch of update_selection calls between one pair (launch gaps included, host latency not).
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
    del raw
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
