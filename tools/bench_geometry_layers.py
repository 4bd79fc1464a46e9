#!/usr/bin/env python3
"""`layers.BackprojectDepth` -> `layers.Project3D` on their HIP kernels against the torch composite they were before
(two batched GEMMs over HW columns + ~10 element-wise ops + cat), with the fused `ops.backproject_project` as the floor.

    python tools/bench_geometry_layers.py [--calls 50] [--warmup 10] [--runs 3] [--out profiles/geometry_layers.json]

B=12 at 192x640 and B=4 at 192x512, fp32, forward + backward per call (gradients into depth, K and T; the upstream gradient
of the grid is a fixed tensor).  Every figure is the median over `--calls` event-timed calls after `--warmup` untimed ones;
each path is measured `--runs` times, the three paths alternating, and the spread (max - min over the runs) is recorded.
`kernels_faster_by_more_than_spread` compares the slowest run on the kernels with the fastest composite run.
`point_cloud_MB` is what the split form moves that the fused kernel does not: [B,4,HW] fp32, written and read once forward
and once backward.  Prints ONE JSON line.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppea-depth_amd")]


def timed(fn, calls, warmup):
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


class CompositeBackproject(torch.nn.Module):
    """BackprojectDepth as a torch composite with resident pixel buffers (the class body before the kernels)."""

    def __init__(self, batch_size, height, width):
        super().__init__()
        self.batch_size = batch_size
        ys, xs = torch.meshgrid(torch.arange(height, dtype=torch.float32),
                                torch.arange(width, dtype=torch.float32), indexing="ij")
        pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(height * width)], 0)
        self.register_buffer("pix_coords", pix[None].repeat(batch_size, 1, 1), persistent=False)
        self.register_buffer("ones", torch.ones(batch_size, 1, height * width), persistent=False)

    def forward(self, depth, inv_K):
        cam_points = torch.matmul(inv_K[:, :3, :3], self.pix_coords)
        cam_points = depth.view(self.batch_size, 1, -1) * cam_points
        return torch.cat([cam_points, self.ones], 1)


class CompositeProject3D(torch.nn.Module):
    """Project3D as a torch composite (the class body before the kernels)."""

    def __init__(self, batch_size, height, width, eps=1e-7):
        super().__init__()
        self.batch_size, self.height, self.width, self.eps = batch_size, height, width, eps

    def forward(self, points, K, T):
        P = torch.matmul(K, T)[:, :3, :]
        cam_points = torch.matmul(P, points)
        pix = cam_points[:, :2, :] / (cam_points[:, 2, :].unsqueeze(1) + self.eps)
        pix = pix.view(self.batch_size, 2, self.height, self.width).permute(0, 2, 3, 1)
        scale = pix.new_tensor([self.width - 1, self.height - 1])
        return (pix / scale - 0.5) * 2


def make_inputs(B, H, W, dev):
    from ppeadepth import synthetic as synth
    g = torch.Generator().manual_seed(B + H + W)
    depth = (0.5 + 5 * torch.rand(B, 1, H, W, generator=g)).to(dev).requires_grad_(True)
    K, inv_K = synth.kitti_K(H, W, 0)
    K = K[None].repeat(B, 1, 1).to(dev).requires_grad_(True)
    inv_K = inv_K[None].repeat(B, 1, 1).to(dev)
    T = torch.eye(4)[None].repeat(B, 1, 1)
    T[:, :3, 3] = 0.1 * torch.randn(B, 3, generator=g)
    T = T.to(dev).requires_grad_(True)
    gg = torch.randn(B, H, W, 2, generator=g).to(dev)
    return depth, inv_K, K, T, gg


def cell(B, H, W, args, dev):
    from ppeadepth import layers, ops
    depth, inv_K, K, T, gg = make_inputs(B, H, W, dev)
    leaves = (depth, K, T)

    def step(forward):
        def fn():
            for t in leaves:
                t.grad = None
            forward().backward(gg)
        return fn

    bp, pr = layers.BackprojectDepth(B, H, W).to(dev), layers.Project3D(B, H, W).to(dev)
    cbp, cpr = CompositeBackproject(B, H, W).to(dev), CompositeProject3D(B, H, W).to(dev)
    paths = {"kernels": step(lambda: pr(bp(depth, inv_K), K, T)),
             "composite": step(lambda: cpr(cbp(depth, inv_K), K, T)),
             "fused": step(lambda: ops.backproject_project(depth, inv_K, K, T))}
    grads = {}
    for name, fn in paths.items():
        fn()
        grads[name] = [t.grad.clone() for t in leaves]
    same_bits = all(torch.equal(a, b) for a, b in zip(grads["kernels"], grads["fused"]))
    err = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["kernels"], grads["composite"]))
    runs = {name: [] for name in paths}
    for _ in range(args.runs):
        for name, fn in paths.items():
            runs[name].append(timed(fn, args.calls, args.warmup))
    spread = max(max(v) - min(v) for v in runs.values())
    med = {name: statistics.median(v) for name, v in runs.items()}
    return {"kernels_ms": [round(v, 4) for v in runs["kernels"]], "composite_ms": [round(v, 4) for v in runs["composite"]],
            "fused_ms": [round(v, 4) for v in runs["fused"]], "spread_ms": round(spread, 4),
            "composite_over_kernels": round(med["composite"] / med["kernels"], 3),
            "kernels_over_fused": round(med["kernels"] / med["fused"], 3),
            "kernels_faster_by_more_than_spread": bool(min(runs["composite"]) - max(runs["kernels"]) > spread),
            "kernels_gradients_equal_fused_bits": same_bits, "kernels_vs_composite_gradient_rel_err": err,
            "point_cloud_MB": round(4 * B * 4 * H * W * 4 / 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry_layers.py times device work and needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"metric": "BackprojectDepth -> Project3D forward + backward, ms per call, fp32 (median of timed calls, per run)",
           "calls": args.calls, "warmup": args.warmup, "runs": args.runs, "device": torch.cuda.get_device_name(0),
           "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
           "command": "python tools/bench_geometry_layers.py --calls %d --warmup %d --runs %d" % (
               args.calls, args.warmup, args.runs),
           "paths": {"kernels": "layers.BackprojectDepth / layers.Project3D (csrc/geometry.hip backproject_*, project3d_*)",
                     "composite": "the same classes as torch ops: batched GEMMs over HW columns, element-wise chain, cat",
                     "fused": "ops.backproject_project (no point cloud)"},
           "cells": {f"B{B}_{H}x{W}": cell(B, H, W, args, dev) for B, H, W in ((12, 192, 640), (4, 192, 512))}}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
