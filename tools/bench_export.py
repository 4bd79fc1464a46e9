"""Prediction export timing: B = 12 planes of 192x640 to 375x1242 (a KITTI frame) and to 352x1216 (the depth benchmark), per
product -- fp32 depth, 16-bit depth * 256, colour picture (minimum .. 95th percentile, plasma) -- on the device
(ops.disp_export, ops.plane_range + ops.colorize, preallocated outputs) and the only way these products could be made
before: copy the planes to the host, then `evaluate.export_depth` (resize_linear + numpy) or `vis.colorize` per image.

    python tools/bench_export.py [--calls 50] [--host_calls 5] [--warmup 10] [--runs 3] [--out profiles/export.json]

Prints ONE JSON line.  Device: HIP events around each call, median over `--calls` timed calls after `--warmup` untimed ones.
Host: the device-to-host copy of the [12,192,640] fp32 planes (HIP events around `.cpu()`; the same for every product) and
the host arithmetic on the copied planes (perf_counter, median over `--host_calls`; the host uses torch's default thread
count) are reported apart.  The two sides alternate, `--runs` times each; every run is kept, a figure is the median run and its
spread max - min over the runs.  The planes are seeded and synthetic (a smooth field with 8 % noise, as the tests')."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppea-depth_amd")]

B, SRC = 12, (192, 640)
TARGETS = {"375x1242": (375, 1242), "352x1216": (352, 1216)}


def planes():
    g = torch.Generator().manual_seed(0)
    y = torch.linspace(0, 1, SRC[0])[None, :, None]
    x = torch.linspace(0, 1, SRC[1])[None, None, :]
    b = torch.arange(B, dtype=torch.float32)[:, None, None]
    field = 6 + 40 * (1 - y) ** 2 + 3 * torch.sin(7 * x + b) * y + 2 * torch.cos(5 * y * x)
    depth = field * (1 + 0.08 * torch.randn(B, *SRC, generator=g)).clamp(0.5, 1.5) * 1.7
    return (1 / depth).float().contiguous()


def device_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def host_ms(fn, calls):
    fn()
    ms = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--host_calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 3, "at least three runs"
    from ppeadepth import evaluate, ops, vis
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda:0")
    pred = planes().to(dev)
    lut = vis.lut("plasma", dev)
    rng = torch.empty(B * 2, device=dev)
    copy_runs = []
    cells = {}
    for tname, (H, W) in TARGETS.items():
        f32 = torch.empty(B * H * W, device=dev)
        u16 = torch.empty(B * H * W, device=dev, dtype=torch.uint16)
        rgb = torch.empty(B * H * W * 3, device=dev, dtype=torch.uint8)

        def colour():
            ops.colorize(pred, (H, W), ops.plane_range(pred, 95.0, out=rng), lut, out=rgb)

        def host_colour(p):
            for b in range(B):
                hi = np.percentile(p[b].astype(np.float64), 95.0).astype(np.float32)
                vis.colorize(evaluate.resize_linear(p[b], W, H), p[b].min(), hi)

        products = {
            "depth_f32": (lambda: ops.disp_export(pred, (H, W), 5.4, 0.0, 80.0, out=f32),
                          lambda p: [evaluate.export_depth(p[b], (H, W), 5.4, 0.0, 80.0) for b in range(B)]),
            "depth_u16": (lambda: ops.disp_export(pred, (H, W), 5.4, 0.0, 80.0, dtype=torch.uint16, out=u16),
                          lambda p: [evaluate.export_depth(p[b], (H, W), 5.4, 0.0, 80.0, dtype=np.uint16) for b in range(B)]),
            "colour": (colour, host_colour),
        }
        host_planes = pred.cpu().numpy()
        runs = {k: {"device": [], "host_arithmetic": []} for k in products}
        for _ in range(args.runs):
            copy_runs.append(round(device_ms(lambda: pred.cpu(), args.calls, args.warmup), 4))
            for k, (dfn, hfn) in products.items():
                runs[k]["device"].append(round(device_ms(dfn, args.calls, args.warmup), 4))
                runs[k]["host_arithmetic"].append(round(host_ms(lambda: hfn(host_planes), args.host_calls), 3))
        cells[tname] = {k: {"runs_ms": v, "ms": {s: statistics.median(r) for s, r in v.items()},
                            "spread_ms": {s: round(max(r) - min(r), 4) for s, r in v.items()}} for k, v in runs.items()}
    res = {"metric": "ms per batch of 12 planes 192x640 -> target, per product (median of timed calls per run)",
           "calls": args.calls, "host_calls": args.host_calls, "warmup": args.warmup, "runs": args.runs,
           "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(),
           "host_copy_ms": {"runs_ms": copy_runs, "ms": statistics.median(copy_runs),
                            "spread_ms": round(max(copy_runs) - min(copy_runs), 4),
                            "what": "device-to-host copy of the [12,192,640] fp32 planes into pageable memory"},
           "cells": cells,
           "command": "python tools/bench_export.py --calls %d --host_calls %d --warmup %d --runs %d"
                      % (args.calls, args.host_calls, args.warmup, args.runs)}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
