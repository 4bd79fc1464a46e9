#!/usr/bin/env python3
"""What the training run adds to the bare step (profiles/train_loop.json).

    python tools/bench_train_loop.py [--out profiles/train_loop.json] [--calls 60] [--steps 100]

31B, B = 12, 192 x 640, bf16 with bf16 parameters, the whole step captured in one hipGraph (bench.py's configuration), one GPU.

  (a) monitor: the two launches of `ops.run_monitor` on the engine's real flat gradient buffer (after real steps) against the
      torch composite that computes the same three results on the same buffer -- linalg.vector_norm, abs().max() and the
      count of non-finite elements.  `--calls` back-to-back calls each after warm-up, alternating blocks, every call between
      its own pair of device events; the median, and the ratio to the streaming floor 4 n bytes / HBM bandwidth (8 TB/s
      peak).  Also one event pair around a whole block of back-to-back calls, divided by their number.
  (b) loop: the step time of `train.Run` on in-memory frames (KITTI's 375 x 1242, decoded once) between two log reads (each
      read ends in a stream synchronise), against the bare replay of the same engine on static inputs in the same session;
      and where the difference can go: the monitor (a), the input pipeline alone, and the host's share of a step (collate).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppea-depth_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12


class MemoryFrames:
    """The item contract of `datasets.KITTIRAWDataset` on frames held in memory: `distinct` random frames, served in turn."""

    def __init__(self, n, frame_idxs, distinct=24, hw=(375, 1242)):
        g = np.random.default_rng(0)
        self.n, self.frame_idxs = n, tuple(frame_idxs)
        self.frames = [g.integers(0, 256, hw + (3,), dtype=np.uint8) for _ in range(distinct)]

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {f: self.frames[(i + 7 * k) % len(self.frames)] for k, f in enumerate(self.frame_idxs)}


def events_ms(fn, calls):
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def block_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_loop.json"))
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num_workers", type=int, default=4)
    args = ap.parse_args()
    from ppeadepth import dist as pdist
    from ppeadepth import networks, options, rng, train
    from ppeadepth import synthetic as synth
    from ppeadepth.runlog import RunLog
    from ppeadepth.trainer import Trainer
    assert torch.cuda.is_available(), "bench_train_loop.py needs a HIP device"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, H, W = args.batch, args.height, args.width
    opt = options.default_options(height=H, width=W, batch_size=B, num_epochs=1)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model)
    model.to(device).train()
    trainer = Trainer(opt, model, device, amp_dtype=torch.bfloat16)
    engine = pdist.TrainEngine(trainer, bf16_params=True)
    rng.set_mode("device")
    steps = 60 + args.steps
    run_args = train._run_parser().parse_args(["--data_path", "-", "--num_workers", str(args.num_workers), "--log_every", "50",
                                               "--early_val_step", "0", "--validate_every", str(10 ** 9), "--saveoff",
                                               "--max_steps", str(steps)])
    ids = list(opt.frame_ids)
    run = train.Run(trainer, engine, run_args, seed=1, out=lambda *a: None,
                    train_data=MemoryFrames(B * steps, ids), val_data=MemoryFrames(B, [0, -1]))
    run.start()

    # ---- (b) the loop, timed between log reads ------------------------------------------------------------------------
    stamps = {}
    check = run.check_log

    def stamped():
        rows = check()
        if rows:
            stamps[rows[-1]["step"]] = time.perf_counter()
        return rows
    run.check_log = stamped
    run.train()
    last = max(s for s in stamps if s % 50 == 0)
    loop_ms = (stamps[last] - stamps[50]) * 1e3 / (last - 50)
    # the bare replay on static inputs, the same engine
    inputs = run.first_batch()
    for _ in range(5):
        engine.step(inputs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        engine.step(inputs)
    torch.cuda.synchronize()
    bare_ms = (time.perf_counter() - t0) * 1e3 / args.steps
    # the input pipeline alone, and the host's collate alone
    from ppeadepth.datasets import collate_raw
    items = [run.train_data[i] for i in range(B)]
    frames = collate_raw(items, pin=True)
    pipe_ms = statistics.median(events_ms(lambda: run.batch(frames, 0), 20))
    t0 = time.perf_counter()
    for _ in range(10):
        collate_raw(items)
    collate_ms = (time.perf_counter() - t0) * 1e2

    # ---- (a) the monitor on the real gradient buffer ----------------------------------------------------------------------
    flat, n = engine.flat.flat, engine.flat.numel
    log = RunLog(device, capacity=256, names=train.LOG_NAMES)
    scalars = {k: v for k, v in engine.static_out[1].items() if k in train.LOG_NAMES}

    def monitor():
        log.append(0, scalars, flat, n, 1.0)

    def composite():
        return torch.linalg.vector_norm(flat), flat.abs().max(), (~torch.isfinite(flat)).sum()
    for _ in range(10):
        monitor()
        composite()
    torch.cuda.synchronize()
    mon, comp, mon_block, comp_block = [], [], [], []
    half = max(args.calls // 2, 25)
    for _ in range(2):                                   # alternating blocks
        mon += events_ms(monitor, half)
        comp += events_ms(composite, half)
        mon_block.append(block_ms(monitor, half))
        comp_block.append(block_ms(composite, half))
    row = log.read()[-1]
    ref = composite()
    floor_ms = 4.0 * n / HBM_PEAK * 1e3
    result = {
        "config": f"31B B={B} {H}x{W} bf16 + bf16 params, captured step, 1 GPU",
        "device": torch.cuda.get_device_name(0),
        "monitor": {
            "elements": int(n), "bytes": int(4 * n), "calls": len(mon),
            "monitor_ms_median": round(statistics.median(mon), 4), "monitor_ms_min": round(min(mon), 4),
            "composite_ms_median": round(statistics.median(comp), 4), "composite_ms_min": round(min(comp), 4),
            "monitor_ms_back_to_back": [round(x, 4) for x in mon_block],
            "composite_ms_back_to_back": [round(x, 4) for x in comp_block],
            "monitor_not_slower_than_composite": bool(statistics.median(mon) <= statistics.median(comp)),
            "streaming_floor_ms_at_8TBps": round(floor_ms, 4),
            "monitor_over_floor": round(statistics.median(mon) / floor_ms, 3),
            "grad_l2": float(row["grad_l2"]), "torch_norm": float(ref[0]), "grad_max_abs": float(row["grad_max_abs"]),
            "torch_max": float(ref[1]), "grad_nonfinite": int(row["grad_nonfinite"]), "torch_nonfinite": int(ref[2]),
        },
        "loop": {
            "steps_timed": int(last - 50), "num_workers": args.num_workers,
            "run_step_ms": round(loop_ms, 3), "bare_replay_ms": round(bare_ms, 3), "difference_ms": round(loop_ms - bare_ms, 3),
            "input_pipeline_ms": round(pipe_ms, 3), "host_collate_ms": round(collate_ms, 3),
            "monitor_ms": round(statistics.median(mon), 4),
        },
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
