#!/usr/bin/env python3
"""The DDAD training step (one source frame: `--frame_ids 0 -1 --selec_reproj`): eager `TrainEngine.step` against whole-step
graph replay.

    python tools/bench_ddad_step.py [--modes eager replay] [--steps 20] [--warmup 5] [--batch 12] [--tag NAME]

RepLKNet-31B, 384 x 640 (options.apply_ddad's training size), B = 12, bf16.  The batch is built the way a DDAD run builds
it: `synthetic.make_ddad_val` items (raw uint8 frames 0 and -1 at 1216 x 1936 with per-sample intrinsics) through
`DDADInputPipeline`.  Per mode: ms per step and img/s over `--steps` steps after `--warmup` untimed ones (wall clock around
a device synchronize; both modes run the same number of steps), and the number of device kernels one eager step launches
(profiler).  A build whose step or `TrainEngine.capture` refuses one source frame reports the refusal, so the same file
measures the code before the step existed.  Prints ONE JSON line.
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


def build(args, dev):
    from ppeadepth import dist as pdist, networks, options, rng, synthetic as synth
    from ppeadepth.input_pipeline import DDADInputPipeline
    from ppeadepth.trainer import Trainer
    opt = options.default_options(height=args.height, width=args.width, batch_size=args.batch, frame_ids=[0, -1],
                                  selec_reproj=False)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model)
    model.to(dev).train()
    bf16 = args.dtype == "bf16"
    engine = pdist.TrainEngine(Trainer(opt, model, dev, amp_dtype=torch.bfloat16 if bf16 else None), bf16_params=bf16)
    rng.set_mode("device")
    raw_hw = tuple(args.raw)
    raw, intr, _depth = synth.collate_ddad(synth.make_ddad_val(args.batch, raw_hw, seed=1234))
    inputs = DDADInputPipeline(dev, args.height, args.width, raw_hw)(raw, intr)
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
    ap.add_argument("--modes", nargs="+", default=["eager", "replay"], choices=["eager", "replay"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--raw", nargs=2, type=int, default=[1216, 1936], help="raw frame size (height width)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--launches", type=int, default=1, choices=[0, 1])
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ddad_step.py needs a HIP device")
    dev = torch.device("cuda", 0)
    from ppeadepth import rng
    from ppeadepth._abi import PpeaKernelError
    line = {"tool": "bench_ddad_step", "tag": args.tag, "B": args.batch, "H": args.height, "W": args.width,
            "raw": list(args.raw), "dtype": args.dtype, "steps": args.steps, "warmup": args.warmup, "frame_ids": [0, -1]}
    model, engine, inputs = build(args, dev)
    line["matching_ids"] = list(model.matching_ids)
    if "eager" in args.modes:
        try:
            dt, loss = time_steps(engine, inputs, args.steps, args.warmup)
        except (IndexError, ValueError) as e:               # a build without the one-source-frame loss path
            line["eager"] = {"refused": f"{type(e).__name__}: {e}"}
            args.modes = []
        else:
            line["eager"] = {"ms_per_step": round(dt * 1e3, 3), "img_per_s": round(args.batch / dt, 2), "loss": loss}
            if args.launches:
                line["eager"]["launches_per_step"] = count_launches(engine, inputs)
    if "replay" in args.modes:
        try:
            engine.capture(inputs, warmup=2)
        except PpeaKernelError as e:
            line["replay"] = {"refused": str(e)}
        else:
            dt, loss = time_steps(engine, inputs, args.steps, args.warmup)
            line["replay"] = {"ms_per_step": round(dt * 1e3, 3), "img_per_s": round(args.batch / dt, 2), "loss": loss}
        finally:
            rng.set_aug_buffer(None)
    if "ms_per_step" in line.get("eager", {}) and "ms_per_step" in line.get("replay", {}):
        line["replay_speedup"] = round(line["eager"]["ms_per_step"] / line["replay"]["ms_per_step"], 3)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
