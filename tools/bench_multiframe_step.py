#!/usr/bin/env python3
"""The training step with several matching frames: eager `TrainEngine.step` against whole-step graph replay.

    python tools/bench_multiframe_step.py [--configs two_past future] [--modes eager replay] [--steps 20] [--warmup 5]
                                          [--grouped 0|1] [--tag NAME]

RepLKNet-31B, 192 x 640, B = 12, bf16 -- bench.py's flagship setting -- with `--num_matching_frames 2` (matching_ids
[0, -1, -2], "two_past"), `--use_future_frame` ([0, 1, -1], "future"), `--num_matching_frames 3` ("three_past": two new
no_grad pose passes, the case `--grouped` is about) or one lookup frame ("single").  Per configuration and mode: ms per
step and img/s over `--steps` steps after `--warmup` untimed ones (wall clock around a device synchronize), and the number
of device kernels one eager step launches (profiler).  A build whose `TrainEngine.capture` refuses the configuration reports
the eager step only, so the same file measures the code before the captured multi-frame step existed.  `--grouped` sets
`repdepth.NEW_PASSES_ONE_BATCH` where the build has it.  Prints ONE JSON line.
"""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppea-depth_amd")]

CONFIGS = {"single": dict(), "two_past": dict(num_matching_frames=2), "three_past": dict(num_matching_frames=3),
           "future": dict(num_matching_frames=1, use_future_frame=True)}
FRAMES = (0, -1, 1, -2, -3)


def build(cfg, args, dev):
    from ppeadepth import dist as pdist, networks, options, rng, synthetic as synth
    from ppeadepth.trainer import Trainer
    opt = options.default_options(height=args.height, width=args.width, batch_size=args.batch, **CONFIGS[cfg])
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model)
    model.to(dev).train()
    bf16 = args.dtype == "bf16"
    engine = pdist.TrainEngine(Trainer(opt, model, dev, amp_dtype=torch.bfloat16 if bf16 else None), bf16_params=bf16)
    rng.set_mode("device")
    inputs = {k: v.to(dev) for k, v in synth.make_inputs(args.batch, args.height, args.width, seed=1234, smooth=True,
                                                         frame_ids=FRAMES).items()}
    random.seed(1000)
    return model, engine, inputs


def time_steps(engine, inputs, steps, warmup):
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
    return dt, loss


def count_launches(engine, inputs):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        engine.step(dict(inputs))
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA") and ev.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["two_past", "future"], choices=list(CONFIGS))
    ap.add_argument("--modes", nargs="+", default=["eager", "replay"], choices=["eager", "replay"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--grouped", type=int, default=None, choices=[0, 1])
    ap.add_argument("--launches", type=int, default=1, choices=[0, 1])
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiframe_step.py needs a HIP device")
    dev = torch.device("cuda", 0)
    from ppeadepth import rng
    from ppeadepth._abi import PpeaKernelError
    from ppeadepth.networks import repdepth
    if args.grouped is not None and hasattr(repdepth, "NEW_PASSES_ONE_BATCH"):
        repdepth.NEW_PASSES_ONE_BATCH = bool(args.grouped)
    line = {"tool": "bench_multiframe_step", "tag": args.tag, "B": args.batch, "H": args.height, "W": args.width,
            "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup,
            "new_passes_one_batch": getattr(repdepth, "NEW_PASSES_ONE_BATCH", None), "results": {}}
    for cfg in args.configs:
        model, engine, inputs = build(cfg, args, dev)
        res = {"matching_ids": list(model.matching_ids)}
        if "eager" in args.modes:
            dt, loss = time_steps(engine, inputs, args.steps, args.warmup)
            res["eager"] = {"ms_per_step": round(dt * 1e3, 3), "img_per_s": round(args.batch / dt, 2), "loss": loss}
            if args.launches:
                res["eager"]["launches_per_step"] = count_launches(engine, inputs)
        if "replay" in args.modes:
            try:
                engine.capture(inputs, warmup=2)
            except PpeaKernelError as e:
                res["replay"] = {"refused": str(e)}
            else:
                dt, loss = time_steps(engine, inputs, args.steps, args.warmup)
                res["replay"] = {"ms_per_step": round(dt * 1e3, 3), "img_per_s": round(args.batch / dt, 2), "loss": loss}
            finally:
                rng.set_aug_buffer(None)
        line["results"][cfg] = res
        del model, engine, inputs
        torch.cuda.empty_cache()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
