"""Streaming inference timing: a captured `DepthStream.push` against a captured `DepthPredictor.predict` at 192x640,
RepLKNet-31B, bf16, B = 1 and B = 12, F = 1 and F = 2 lookup frames.

    python tools/bench_stream.py [--calls 50] [--warmup 10] [--runs 3] [--out profiles/stream_bench.json]

Prints ONE JSON line.  Per cell the two paths alternate, `--runs` times each in this process on the same device; a run is the
median over `--calls` timed calls (HIP events around each call, after `--warmup` untimed ones; the input copies and the output
clones of a replayed call are inside the timed region on both sides).  Every run is kept; the cell's figure is the median run,
its spread max - min over the runs, and `push_faster_by_more_than_spread` compares the slowest push run with the fastest
predict run.  `predict` is the call of this build: the change that added the stream left its schedule and its kernels'
instantiations as they were.  The stream has its full history while it is timed (the state the camera is in after F frames).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.calls >= 50 and args.runs >= 3, "at least 50 timed calls and three runs"
    from ppeadepth import networks, options, synthetic
    from ppeadepth.inference import DepthPredictor
    dev = torch.device("cuda:0")
    H, W = 192, 640
    cells = {}
    for B in (1, 12):
        for Fr in (1, 2):
            opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, num_matching_frames=Fr)
            torch.manual_seed(0)
            model = networks.RepDepth(opt)
            synthetic.fill_state_dict(model, conditioned=True)
            model.to(dev).eval()
            data = {k: v.to(dev) for k, v in synthetic.make_rendered_inputs(B, H, W, frame_ids=(0, -1, -2)).items()}
            frames = [data[("color", f, 0)] for f in (-2, -1, 0)]
            K2, iK2 = data[("K", 2)], data[("inv_K", 2)]
            looks = torch.stack([frames[1 - j] for j in range(Fr)], 1)
            p = DepthPredictor(model, opt).capture(B, mono=False)
            s = DepthPredictor(model, opt).stream(B).capture()
            n = [0]

            def predict():
                return p.predict(frames[2], looks, K2, iK2, 0.1, 10.0)

            def push():
                n[0] += 1
                return s.push(frames[n[0] % 3], K2, iK2, 0.1, 10.0)

            runs = {"predict": [], "push": []}
            for _ in range(args.runs):
                runs["predict"].append(round(timed(predict, args.calls, args.warmup), 4))
                runs["push"].append(round(timed(push, args.calls, args.warmup), 4))
            assert bool(push()["present"].all())
            spread = {k: round(max(v) - min(v), 4) for k, v in runs.items()}
            cells[f"B{B}_F{Fr}"] = {
                "runs_ms": runs, "ms": {k: statistics.median(v) for k, v in runs.items()}, "spread_ms": spread,
                "predict_over_push": round(statistics.median(runs["predict"]) / statistics.median(runs["push"]), 3),
                "push_faster_by_more_than_spread": bool(min(runs["predict"]) - max(runs["push"]) > max(spread.values()))}
            del model, p, s
            torch.cuda.empty_cache()
    res = {"metric": "ms per call at 640x192 RepLKNet-31B bf16, graph replay (median of timed calls per run)", "calls": args.calls,
           "warmup": args.warmup, "runs": args.runs, "device": torch.cuda.get_device_name(0), "cells": cells,
           "command": "python tools/bench_stream.py --calls %d --warmup %d --runs %d" % (args.calls, args.warmup, args.runs)}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
