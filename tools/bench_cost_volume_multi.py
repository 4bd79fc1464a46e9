#!/usr/bin/env python3
"""The fused F-frame cost volume (`ops.cost_volume_multi`) against what the code could do before it existed: F launches with
one lookup frame each (`ops.cost_volume`) combined with torch ops (sum, count of `> 0`, divide).

    python tools/bench_cost_volume_multi.py [--calls 50] [--warmup 10] [--runs 3] [--predictor] [--out profiles/cost_volume_multi.json]

[B,128,48,160] features (RepLKNet-31B at 192 x 640), 96 bins, B in {1, 12}, F in {2, 3, 4}, fp32 and bf16 features.  Every
figure is the median over `--calls` event-timed calls after `--warmup` untimed ones; each cell is measured `--runs` times,
fused and composite alternating, and the spread (max - min over the runs) is recorded.  `faster_by_more_than_spread` compares
the slowest fused run with the fastest composite run.  The composite gets its per-frame lookup maps as separate contiguous
tensors (made outside the timed region), so it pays for no copy the fused path does not pay for.
--predictor adds `DepthPredictor` ms per call with two lookup frames against one (bf16, eager and graph replay, B in {1, 12}),
measured as tools/bench_infer.py does.  Prints ONE JSON line.
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

C, h, w, D = 128, 48, 160, 96


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


def make_inputs(B, F, dtype, dev):
    from ppeadepth import synthetic as synth
    g = torch.Generator().manual_seed(B * 10 + F)
    cur = torch.randn(B, C, h, w, generator=g).to(dtype).to(dev)
    look = torch.randn(B, F, C, h, w, generator=g).to(dtype).to(dev)
    K, inv_K = synth.kitti_K(4 * h, 4 * w, 2)
    K, inv_K = K[None].repeat(B, 1, 1).to(dev), inv_K[None].repeat(B, 1, 1).to(dev)
    T = torch.eye(4)[None, None].repeat(B, F, 1, 1)
    for f in range(F):                      # frames -1, -2, -3 one metre apart, the last of four the future frame
        step = f + 1 if f < 3 else -1
        T[:, f, 2, 3], T[:, f, 0, 3] = 1.0 * step, 0.05 * step
    bins = torch.exp(torch.linspace(torch.log(torch.tensor(0.1)), torch.log(torch.tensor(10.0)), D)).to(dev)
    return cur, look, T.to(dev), K, inv_K, bins


def composite(cur, frames, T, K, inv_K, bins):
    """F single-frame launches + torch ops: the masked differences summed, divided by the number of frames with one."""
    from ppeadepth import ops
    vols = [ops.cost_volume(cur, fr, T[:, f], K, inv_K, bins) for f, fr in enumerate(frames)]
    total, count = vols[0], (vols[0] > 0).float()
    for v in vols[1:]:
        total = total + v
        count = count + (v > 0).float()
    return total / (count + 1e-7)


def kernel_cells(args, dev):
    from ppeadepth import ops
    cells = {}
    for B in (1, 12):
        for F in (2, 3, 4):
            for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                cur, look, T, K, inv_K, bins = make_inputs(B, F, dtype, dev)
                frames = [look[:, f].contiguous() for f in range(F)]
                fused = lambda: ops.cost_volume_multi(cur, look, T, K, inv_K, bins)          # noqa: E731
                comp = lambda: composite(cur, frames, T, K, inv_K, bins)                     # noqa: E731
                a, b = fused(), comp()
                # a single-frame launch divides its frame's difference by 1 + 1e-7 first: a few ulps apart
                err = float((a - b).abs().max() / b.abs().max())
                runs = {"fused": [], "composite": []}
                for _ in range(args.runs):
                    runs["fused"].append(timed(fused, args.calls, args.warmup))
                    runs["composite"].append(timed(comp, args.calls, args.warmup))
                fu, co = runs["fused"], runs["composite"]
                spread = max(max(fu) - min(fu), max(co) - min(co))
                # algorithmic bytes: every feature map read once, the volume written once
                alg = (1 + F) * B * C * h * w * cur.element_size() + B * D * h * w * 4
                cells[f"B{B}_F{F}_{name}"] = {
                    "fused_ms": [round(v, 4) for v in fu], "composite_ms": [round(v, 4) for v in co],
                    "spread_ms": round(spread, 4), "speedup": round(statistics.median(co) / statistics.median(fu), 3),
                    "faster_by_more_than_spread": bool(min(co) - max(fu) > spread),
                    "fused_vs_composite_rel_err": err, "inside_edge_mask": round(float((a != 0).float().mean()), 3),
                    "algorithmic_MB": round(alg / 1e6, 2), "algorithmic_GB_per_s": round(alg / statistics.median(fu) / 1e6, 1)}
    return cells


def predictor_cells(args, dev):
    from ppeadepth import networks, options, synthetic
    from ppeadepth.inference import DepthPredictor
    H, W = 192, 640
    cells = {}
    for B in (1, 12):
        for nf in (1, 2):
            opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, num_matching_frames=nf)
            torch.manual_seed(0)
            model = networks.RepDepth(opt)
            synthetic.fill_state_dict(model, conditioned=True)
            model.to(dev).eval()
            data = {k: v.to(dev) for k, v in synthetic.make_rendered_inputs(B, H, W, frame_ids=(0, -1, -2)).items()}
            c0, K2, iK2 = data[("color", 0, 0)], data[("K", 2)], data[("inv_K", 2)]
            looks = data[("color", -1, 0)] if nf == 1 else torch.stack([data[("color", -1, 0)], data[("color", -2, 0)]], 1)
            eager = DepthPredictor(model, opt)
            graph = DepthPredictor(model, opt).capture(B, mono=False)
            ms = [timed(lambda p=p: p.predict(c0, looks, K2, iK2, 0.1, 10.0), args.calls, args.warmup) for p in (eager, graph)]
            cells[f"B{B}_F{nf}"] = {"predictor_eager_ms": round(ms[0], 4), "predictor_replay_ms": round(ms[1], 4)}
            del model, eager, graph
            torch.cuda.empty_cache()
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--predictor", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"metric": "cost volume ms per call, [B,128,48,160] features x 96 bins (median of timed calls, per run)",
           "calls": args.calls, "warmup": args.warmup, "runs": args.runs, "device": torch.cuda.get_device_name(0),
           "command": "python tools/bench_cost_volume_multi.py --calls %d --warmup %d --runs %d%s" % (
               args.calls, args.warmup, args.runs, " --predictor" if args.predictor else ""),
           "comparator": "F x ops.cost_volume + torch sum / count(> 0) / divide", "cells": kernel_cells(args, dev)}
    if args.predictor:
        res["predictor"] = {"metric": "DepthPredictor.predict ms per call at 640x192 RepLKNet-31B bf16, F lookup frames",
                            "cells": predictor_cells(args, dev)}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
