"""Point-cloud timing: B = 12 planes of 192x640 to 375x1242 (a KITTI frame) and to 192x640 (the network's size, what a
`StreamMap` adds per push), stride 1 and 2, edge 0 and 0.1 -- the three launches of `ops.point_cloud` (camera-to-world pose,
uint8 colour, preallocated outputs, the cursor reset on the stream inside the timed region) against the only way to get
these points without it: `ops.disp_export` + the copy of the full-size depth to the host, then the numpy arithmetic of
`evaluate.export_points` on the copied planes.

    python tools/bench_points.py [--calls 50] [--host_calls 3] [--warmup 10] [--runs 3] [--out profiles/points.json]

Prints ONE JSON line.  Device: HIP events around each call, median over `--calls` timed calls after `--warmup` untimed ones.
Host route, its two parts apart: (a) `disp_export` into a preallocated buffer + `.cpu()` (HIP events), (b) the host arithmetic
(perf_counter, median over `--host_calls`; torch's default thread count; it resizes the disparity again itself, so (b) alone
is already the whole host computation).  The two sides alternate, `--runs` times each; every run is kept, a figure is the
median run and its spread max - min over the runs.  Bytes: what the algorithm must move per call, computed from the shapes
and the kept count (source planes read twice, 8 bytes of ballot words per 64 candidates written and read, 12 + 3 + 8 bytes
per kept point written, 3 colour bytes per kept point read), and the time the HBM would need for them at the peak rate of
the data sheet.  `captured_push_ms` quotes profiles/stream_bench.json (B = 12, F = 1) when that file exists: another run, for
scale only.  The planes are seeded and synthetic (a smooth field with 8 % noise, as the tests')."""
import argparse
import contextlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppea-depth_amd"), os.path.join(ROOT, "tools")]

from bench_export import B, SRC, device_ms, host_ms, planes  # noqa: E402

TARGETS = {"375x1242": (375, 1242), "192x640": (192, 640)}
HBM_BYTES_PER_S = 8e12               # MI355X data sheet
LO, HI = 12.0, 60.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--host_calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 3, "at least three runs"
    from ppeadepth import evaluate, ops
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda:0")
    pred = planes().to(dev)
    host_planes = pred.cpu().numpy()
    g = torch.Generator().manual_seed(1)
    cells = {}
    for tname, (H, W) in TARGETS.items():
        K = np.eye(4)
        K[0, 0], K[0, 2], K[1, 1], K[1, 2] = 0.58 * W, 0.5 * W, 1.92 * H, 0.5 * H
        inv_K = torch.from_numpy(np.linalg.inv(K).astype(np.float32)).repeat(B, 1, 1).contiguous().to(dev)
        pose = torch.eye(4).repeat(B, 1, 1)
        pose[:, :3, 3] = torch.randn(B, 3, generator=g)
        pose = pose.to(dev)
        colour = torch.randint(0, 256, (B * H * W * 3,), generator=g, dtype=torch.uint8).to(dev)
        depth = torch.empty(B * H * W, device=dev)
        host_K, host_pose, host_colour = inv_K[0].cpu().numpy(), pose.cpu().numpy(), colour.cpu().numpy().reshape(B, H, W, 3)

        def copy_route():
            return ops.disp_export(pred, (H, W), 1.0, 0.0, 1e9, out=depth).cpu()

        for stride in (1, 2):
            cloud = ops.new_point_cloud(ops.candidate_count([(H, W)] * B, stride), B, dev, True)
            for edge in (0.0, 0.1):
                def device():
                    ops.point_cloud(pred, (H, W), inv_K, pose, colour, None, 1.0, LO, HI, stride, edge, out=cloud.clear())

                def host():
                    return [evaluate.export_points(host_planes[b], (H, W), host_K, host_colour[b], host_pose[b], 1.0, LO, HI,
                                                   stride, edge, offset=b * H * W) for b in range(B)]

                runs = {"device": [], "host_depth_and_copy": [], "host_arithmetic": []}
                for _ in range(args.runs):
                    runs["device"].append(round(device_ms(device, args.calls, args.warmup), 4))
                    runs["host_depth_and_copy"].append(round(device_ms(copy_route, args.calls, args.warmup), 4))
                    runs["host_arithmetic"].append(round(host_ms(host, args.host_calls), 3))
                kept, dropped = cloud.cursor.tolist()
                kept_host = sum(len(x[2]) for x in host())          # pixels within rounding of a threshold may differ
                assert dropped == 0 and abs(kept - kept_host) <= 0.02 * cloud.xyz.shape[0], (kept, kept_host)
                cand = cloud.xyz.shape[0]
                nbytes = 2 * pred.numel() * 4 + 2 * (cand // 64) * 8 + kept * (12 + 3 + 8 + 3)
                cells[f"{tname}_stride{stride}_edge{edge}"] = {
                    "runs_ms": runs, "ms": {s: statistics.median(r) for s, r in runs.items()},
                    "spread_ms": {s: round(max(r) - min(r), 4) for s, r in runs.items()}, "candidates": cand, "kept": kept, "kept_host": kept_host,
                    "bytes_needed": nbytes, "hbm_floor_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 5)}
    res = {"metric": "ms per batch of 12 planes 192x640 -> points at the target size (median of timed calls per run)",
           "calls": args.calls, "host_calls": args.host_calls, "warmup": args.warmup, "runs": args.runs,
           "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "range": [LO, HI], "cells": cells,
           "command": "python tools/bench_points.py --calls %d --host_calls %d --warmup %d --runs %d"
                      % (args.calls, args.host_calls, args.warmup, args.runs)}
    stream = os.path.join(ROOT, "profiles", "stream_bench.json")
    if os.path.exists(stream):
        with open(stream) as f:
            res["captured_push_ms"] = {"B12_F1": json.load(f)["cells"]["B12_F1"]["ms"]["push"],
                                       "what": "profiles/stream_bench.json: another run, quoted for scale only"}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
