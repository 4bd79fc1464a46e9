"""Inference timing: the eval-mode module path (`model.eval()` + `Trainer.predict_disps`) against `DepthPredictor`, eager and
graph replay, at 192x640, RepLKNet-31B, bf16, B = 1 and B = 12, teacher only and multi-frame.

    python tools/bench_infer.py [--calls 50] [--warmup 10] [--out profiles/infer_bench.json] [--repeat-of FILE ...]

Prints ONE JSON line.  Every figure is the median over `--calls` timed calls (HIP events around each call, after `--warmup`
untimed ones, all three paths in this process on the same device); launch counts are device kernels of one call from the
profiler.  Run it three times and pass the earlier outputs with --repeat-of: the last run then also records the run-to-run
spread (max - min over the runs, per cell) next to its own numbers.
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


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA") and ev.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat-of", nargs="*", default=[])
    args = ap.parse_args()
    assert args.calls >= 50, "at least 50 timed calls"
    from ppeadepth import networks, options, synthetic
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.trainer import Trainer
    dev = torch.device("cuda:0")
    H, W = 192, 640
    cells = {}
    for B in (1, 12):
        opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False)
        torch.manual_seed(0)
        model = networks.RepDepth(opt)
        synthetic.fill_state_dict(model, conditioned=True)
        model.to(dev).eval()
        data = {k: v.to(dev) for k, v in synthetic.make_rendered_inputs(B, H, W).items()}
        c0, cm1, K2, iK2 = data[("color", 0, 0)], data[("color", -1, 0)], data[("K", 2)], data[("inv_K", 2)]
        tr = Trainer(opt, model, dev, amp_dtype=torch.bfloat16)

        @torch.no_grad()
        def parent_mono():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return model.mono_depth(model.mono_encoder(c0))[("disp", 0)].float()

        def parent_multi():
            return tr.predict_disps(dict(data), mono=False)

        eager = DepthPredictor(model, opt)
        graph = DepthPredictor(model, opt).capture(B)
        mn, mx = tr.depth_bin_tracker.compute()
        paths = {
            "teacher": (parent_mono, lambda: eager.predict_mono(c0), lambda: graph.predict_mono(c0)),
            "multi": (parent_multi, lambda: eager.predict(c0, cm1, K2, iK2, mn, mx), lambda: graph.predict(c0, cm1, K2, iK2, mn, mx)),
        }
        for name, (parent, pe, pg) in paths.items():
            ms = [timed(f, args.calls, args.warmup) for f in (parent, pe, pg)]
            cells[f"B{B}_{name}"] = {
                "ms": dict(zip(("module_path", "predictor_eager", "predictor_replay"), (round(m, 4) for m in ms))),
                "img_per_s": dict(zip(("module_path", "predictor_eager", "predictor_replay"), (round(B * 1e3 / m, 1) for m in ms))),
                "launches": {"module_path": launches(parent), "predictor_eager": launches(pe)},
            }
        del model, tr, eager, graph
        torch.cuda.empty_cache()
    res = {"metric": "inference ms per call at 640x192 RepLKNet-31B bf16 (median of timed calls)", "calls": args.calls,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "cells": cells,
           "command": "python tools/bench_infer.py --calls %d --warmup %d" % (args.calls, args.warmup)}
    if args.repeat_of:
        runs = [json.load(open(f))["cells"] for f in args.repeat_of] + [cells]
        res["runs"] = len(runs)
        res["spread_ms"] = {c: {k: round(max(r[c]["ms"][k] for r in runs) - min(r[c]["ms"][k] for r in runs), 4)
                                for k in cells[c]["ms"]} for c in cells}
        res["replay_faster_than_module_path_by_more_than_spread"] = {
            c: bool(min(r[c]["ms"]["module_path"] for r in runs) - max(r[c]["ms"]["predictor_replay"] for r in runs)
                    > max(res["spread_ms"][c].values())) for c in cells}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
