#!/usr/bin/env python3
"""Full fine-tuning (--fullft_reb) timings.

    python tools/bench_fullft.py [--part kernels step] [--calls 30] [--warmup 10] [--runs 3] [--steps 10] [--tag NAME]
                                 [--out profiles/fullft.json]

kernels  the depthwise filter gradients of one RepLKBlock (k x k + 5 x 5) at the four stage shapes of RepLKNet-31B,
         B = 12, 192 x 640: ONE launch of ppea_dwconv_lk_bwd_filter_bf16 (+ its fixed-order sum) against what the code did
         before that kernel existed for the same result -- four fp32 conversions of x / dy and two launches of
         ppea_dwconv_lk_bwd_filter_f32.  Median over --calls event-timed calls after --warmup untimed ones, --runs times
         each, new and old alternating; `spread_ms` is max - min over the runs.
step     one bf16 TrainEngine step of BASELINE config 2's model with every backbone weight trainable (B = 12, 192 x 640),
         eager and -- if the step captures -- replayed from the hipGraph: wall-clock ms per step over --steps steps ending in
         a device synchronise.  Runs on any commit that has the flag (the kernels part needs this commit's entry point), so
         the same script times the parent; --tag names the commit in the output.
Prints ONE JSON line.
"""
import argparse
import contextlib
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppea-depth_amd")]

SHAPES = [(12, 128, 48, 160, 31), (12, 256, 24, 80, 29), (12, 512, 12, 40, 27), (12, 1024, 6, 20, 13)]


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


def kernel_cells(args, dev):
    from ppeadepth import _abi, ops
    cells = {}
    for (N, C, H, W, K) in SHAPES:
        g = torch.Generator().manual_seed(K)
        x, dyb, dys = (torch.randn(N, C, H, W, generator=g).bfloat16().to(dev) for _ in range(3))

        def new():
            return ops.dwconv_lk_bwd_filter(x, dyb, dys, K)

        def old():
            dwb = torch.empty(C, K, K, device=dev)
            dws = torch.empty(C, 5, 5, device=dev)
            xa, da = x.float().contiguous(), dyb.float().contiguous()
            _abi.call("ppea_dwconv_lk_bwd_filter_f32", _abi.ptr(xa), _abi.ptr(da), _abi.ptr(dwb), N, C, H, W, K, _abi.stream_ptr())
            xb, db = x.float().contiguous(), dys.float().contiguous()
            _abi.call("ppea_dwconv_lk_bwd_filter_f32", _abi.ptr(xb), _abi.ptr(db), _abi.ptr(dws), N, C, H, W, 5, _abi.stream_ptr())
            return dwb, dws
        a, b = new(), old()
        err = max(float((a[i] - b[i]).abs().max() / b[i].abs().max()) for i in (0, 1))
        runs = {"new": [], "old": []}
        for _ in range(args.runs):
            runs["new"].append(timed(new, args.calls, args.warmup))
            runs["old"].append(timed(old, args.calls, args.warmup))
        nw, od = runs["new"], runs["old"]
        spread = max(max(nw) - min(nw), max(od) - min(od))
        # executed matrix work: two 32 x 32 x 16 tiles (k x k and 5 x 5) per 16 columns of every input row; operand bytes:
        # x, dy_big, dy_small read once (bf16)
        flop = 2 * 2 * 32 * 32 * 16 * N * C * H * ((W + 15) // 16)
        nbytes = 3 * N * C * H * W * 2
        med = statistics.median(nw)
        cells[f"{N}x{C}x{H}x{W}_k{K}"] = {
            "new_ms": [round(v, 4) for v in nw], "old_ms": [round(v, 4) for v in od], "spread_ms": round(spread, 4),
            "speedup": round(statistics.median(od) / med, 2), "faster_by_more_than_spread": bool(min(od) - max(nw) > spread),
            "new_vs_old_rel_err": err, "executed_mfma_GFLOP": round(flop / 1e9, 2), "operand_MB": round(nbytes / 1e6, 1),
            "executed_TFLOP_per_s": round(flop / med / 1e9, 1), "operand_GB_per_s": round(nbytes / med / 1e6, 1)}
    return cells


def step_cells(args, dev):
    from ppeadepth import dist as pdist, networks, options, rng, synthetic as synth
    from ppeadepth._abi import PpeaKernelError
    from ppeadepth.trainer import Trainer
    B, H, W = args.batch, 192, 640
    opt = options.default_options(height=H, width=W, batch_size=B, fullft_reb=True)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model, conditioned=True)
    model.to(dev).train()
    trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
    engine = pdist.TrainEngine(Trainer(opt, model, dev, amp_dtype=torch.bfloat16), bf16_params=True)
    rng.set_mode("device")
    inputs = {k: v.to(dev) for k, v in synth.make_rendered_inputs(B, H, W).items()}
    random.seed(1000)

    def run(steps, warmup):
        for _ in range(warmup):
            engine.step(inputs if engine.graph is not None else dict(inputs))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            _, losses = engine.step(inputs if engine.graph is not None else dict(inputs))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        loss = float(losses["loss"])
        assert loss == loss, "the loss is NaN"
        return {"ms_per_step": round(dt * 1e3, 2), "img_per_s": round(B / dt, 2), "loss": loss}
    res = {"B": B, "H": H, "W": W, "trainable_parameters": trainable, "eager": run(args.steps, args.warmup)}
    try:
        engine.capture(inputs, warmup=2)
    except (PpeaKernelError, RuntimeError) as e:
        res["replay"] = {"refused": str(e)[:200]}
    else:
        res["replay"] = run(args.steps, args.warmup)
    finally:
        rng.set_aug_buffer(None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernels", "step"], choices=["kernels", "step"])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fullft.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"tool": "bench_fullft", "tag": args.tag, "device": torch.cuda.get_device_name(0), "calls": args.calls,
           "warmup": args.warmup, "runs": args.runs, "steps": args.steps}
    if "kernels" in args.part:
        res["dwconv_filter_gradient"] = {
            "metric": "ms per call, both filter gradients of one block (median of timed calls, per run)",
            "comparator": "4 x .float() + 2 x ppea_dwconv_lk_bwd_filter_f32", "cells": kernel_cells(args, dev)}
    if "step" in args.part:
        res["fullft_step_bf16"] = step_cells(args, dev)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
