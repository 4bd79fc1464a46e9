"""Validation timing: `Trainer.val` with the host metric (numpy, as the reference) against `metrics="device"`
(csrc/eval_metrics.hip), predictions from a bf16 `DepthPredictor` replaying graphs at B = 12.

    python tools/bench_val.py [--reps 3] [--out profiles/val_bench.json] [--repeat-of FILE ...]

Two synthetic splits: 96 eigen-size images (192x640 frames, sparse 375x1242 / 370x1226 ground truth) and 24 Cityscapes-size
images (192x512 frames, dense 1024x2048 ground truth).  Per split and per metric path: the wall time of a whole `val` (both
networks; median of `--reps` calls after one warm-up call, the call returns host numbers so it ends synchronised), the
prediction loop alone, and the scoring alone on kept disparities.  The select kernel's time per image comes from the
profiler and stands beside its streaming floor (bytes it reads / 6.3 TB/s).  Prints ONE JSON line.  On a tree whose
`Trainer.val` has no `metrics` keyword only the host numbers are reported.  Run it three times and pass the earlier outputs
with --repeat-of: the last run then records the run-to-run spread and the acceptance (slowest device run < fastest host run).

    python tools/bench_val.py --case ddad [--reps 3] [--out profiles/val_bench_ddad.json]

The DDAD case: `Trainer.val_ddad` over 24 images at 384x640 (B = 12, frames 0 and -1) whose 1216x1936 ground truth with 1 %
valid pixels arrives inside each batch, host metric against `metrics="device"`, timed the same way.  A report, not a gate:
the only comparison is the host-scored `val_ddad` of the same commit.
"""
import argparse
import contextlib
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppea-depth_amd")]

B = 12
SPLITS = {"eigen": dict(n=96, hw=(192, 640), gt=[(375, 1242), (370, 1226)], keep=0.05),
          "cityscapes": dict(n=24, hw=(192, 512), gt=[(1024, 2048)], keep=0.6)}


def wall(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ms), 3)


def ground_truth(n, sizes, keep, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        y = torch.linspace(0, 1, h)[:, None]
        depth = (6 + 40 * (1 - y) ** 2) * (1 + 0.1 * torch.randn(h, w, generator=g)).clamp(0.5, 1.5)
        out.append((depth * (torch.rand(h, w, generator=g) < keep)).numpy().astype(np.float32))
    return out


def kernel_us(fn, pattern):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name]
    return sum(e.time_range.elapsed_us() for e in ev if pattern in e.name), len(ev)


DDAD = dict(n=24, hw=(384, 640), gt=(1216, 1936), keep=0.01)


def ddad_case(args):
    from ppeadepth import evaluate, networks, options, synthetic
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.trainer import Trainer
    dev = torch.device("cuda:0")
    (H, W), n, (gh, gw) = DDAD["hw"], DDAD["n"], DDAD["gt"]
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, frame_ids=[0, -1])
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synthetic.fill_state_dict(model, conditioned=True)
    model.to(dev).eval()
    tr = Trainer(opt, model, dev, amp_dtype=torch.bfloat16)
    pred = DepthPredictor(model, opt).capture(B)
    g = torch.Generator().manual_seed(11)
    y = torch.linspace(0, 1, gh)[:, None]
    batches, depths = [], []
    for j in range(n // B):
        data = {k: v.to(dev) for k, v in synthetic.make_rendered_inputs(B, H, W, seed=7 + j, frame_ids=(0, -1)).items()}
        depth = (6 + 230 * (1 - y) ** 2) * (1 + 0.1 * torch.randn(B, gh, gw, generator=g)).clamp(0.5, 1.5)
        depths.append((depth * (torch.rand(B, gh, gw, generator=g) < DDAD["keep"])).float())
        batches.append(data)
    on_host = lambda: [dict(b, depth=d) for b, d in zip(batches, depths)]                  # noqa: E731
    depths_dev = [d.to(dev) for d in depths]
    on_device = lambda: [dict(b, depth=d) for b, d in zip(batches, depths_dev)]            # noqa: E731

    def predict_only():
        for data in on_host():
            tr.predict_disps(data, True, pred, mono_max_depth=80)

    disps = [tr.predict_disps(data, True, pred, mono_max_depth=80) for data in on_host()]
    host_disps = [np.concatenate([d[k].float().cpu().numpy() for d in disps]) for k in (0, 1)]
    gts = np.concatenate([d.numpy() for d in depths])
    dgs = [evaluate.DeviceGroundTruth.from_batch(d, dev) for d in depths_dev]

    def host_scoring():
        evaluate.evaluate_disps_ddad(host_disps[0], gts, True, 1.0)
        evaluate.evaluate_disps_ddad(host_disps[1], gts, True)

    def device_scoring():
        from ppeadepth import ops
        errors = [[dg.score(d[k].float().contiguous(), 0, "val_ddad")[0] for dg, d in zip(dgs, disps)] for k in (0, 1)]
        return torch.stack([ops.depth_errors_mean(torch.cat(e)) for e in errors]).cpu()

    cell = {"images": n, "batch": B, "frames_hw": [H, W], "ground_truth_hw": [gh, gw], "valid_fraction": DDAD["keep"],
            "val_ms": {"host": wall(lambda: tr.val_ddad(on_host(), predictor=pred), args.reps),
                       "device": wall(lambda: tr.val_ddad(on_device(), predictor=pred, metrics="device"), args.reps),
                       "device_with_upload": wall(lambda: tr.val_ddad(on_host(), predictor=pred, metrics="device"), args.reps)},
            "predict_ms": wall(predict_only, args.reps),
            "scoring_ms": {"host": wall(host_scoring, args.reps), "device": wall(device_scoring, args.reps)}}
    one = disps[0][0].float().contiguous()
    us, events = kernel_us(lambda: dgs[0].score(one, 0, "val_ddad"), "eval_select_pass")
    gather, _ = kernel_us(lambda: dgs[0].score(one, 0, "val_ddad"), "eval_gather")
    total, _ = kernel_us(lambda: dgs[0].score(one, 0, "val_ddad"), "eval_")
    moved = 10 * 4 * gh * gw                  # gather: gt read, 2 workspaces written; 4 passes x 2 read; partial: 2 read
    cell["kernels"] = {"gather_us_per_image": round(gather / B, 3), "select_us_per_image": round(us / B, 3),
                       "all_scoring_kernels_us_per_image": round(total / B, 3), "bytes_moved_per_image": moved,
                       "floor_us_per_image_at_6.3TBps": round(moved / 6.3e12 * 1e6, 3), "device_events_per_batch": events}
    h = tr.val_ddad(on_host(), predictor=pred)
    d = tr.val_ddad(on_device(), predictor=pred, metrics="device")
    cell["max_rel_difference_of_the_7_errors"] = float(max(np.max(np.abs(a - b) / np.abs(b)) for a, b in zip(d, h)))
    cell["metric_share_of_host_val"] = round(1 - cell["predict_ms"] / cell["val_ms"]["host"], 4)
    res = {"metric": "Trainer.val_ddad wall ms (both networks), bf16 DepthPredictor graph replay at B=12, median of reps; "
                     "the only comparison is the host-scored val_ddad of the same commit",
           "reps": args.reps, "device": torch.cuda.get_device_name(0), "cells": {"val_ddad": cell},
           "command": "python tools/bench_val.py --case ddad --reps %d" % args.reps}
    line = json.dumps(res)
    with open(args.out or os.path.join(ROOT, "profiles", "val_bench_ddad.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat-of", nargs="*", default=[])
    ap.add_argument("--case", choices=["splits", "ddad"], default="splits")
    args = ap.parse_args()
    if args.case == "ddad":
        return ddad_case(args)
    from ppeadepth import evaluate, networks, options, synthetic
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.trainer import Trainer
    dev = torch.device("cuda:0")
    has_device = "metrics" in inspect.signature(Trainer.val).parameters
    cells = {}
    for split, cfg in SPLITS.items():
        (H, W), n = cfg["hw"], cfg["n"]
        opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False)
        torch.manual_seed(0)
        model = networks.RepDepth(opt)
        synthetic.fill_state_dict(model, conditioned=True)
        model.to(dev).eval()
        tr = Trainer(opt, model, dev, amp_dtype=torch.bfloat16)
        pred = DepthPredictor(model, opt).capture(B)
        batches = [{k: v.to(dev) for k, v in synthetic.make_rendered_inputs(B, H, W, seed=7 + j).items()}
                   for j in range(n // B)]
        gts = ground_truth(n, cfg["gt"], cfg["keep"], 11)
        fresh = lambda: [dict(b) for b in batches]                       # noqa: E731  (val adds the pose to the batch)

        def predict_only():
            for data in fresh():
                tr.predict_disps(data, True, pred)

        disps = [tr.predict_disps(data, True, pred) for data in fresh()]
        host_disps = [np.concatenate([d[k].cpu().numpy() for d in disps]) for k in (0, 1)]

        def host_scoring():
            evaluate.evaluate_disps(host_disps[0], gts, split, True, 1.0)
            evaluate.evaluate_disps(host_disps[1], gts, split, True)

        cell = {"images": n, "batch": B,
                "val_ms": {"host": wall(lambda: tr.val(fresh(), gts, split, predictor=pred), args.reps)},
                "predict_ms": wall(predict_only, args.reps),
                "scoring_ms": {"host": wall(host_scoring, args.reps)}}
        if has_device:
            dg = evaluate.DeviceGroundTruth(gts, dev)
            from ppeadepth import ops

            def device_scoring():
                errors = torch.empty(2, n, 7, device=dev, dtype=torch.float64)
                for j, d in enumerate(disps):
                    for k in (0, 1):
                        dg.score(d[k].float().contiguous(), j * B, split, True, 1.0, out=errors[k, j * B:(j + 1) * B])
                return torch.stack([ops.depth_errors_mean(e) for e in errors]).cpu()

            cell["val_ms"]["device"] = wall(lambda: tr.val(fresh(), dg, split, predictor=pred, metrics="device"), args.reps)
            cell["val_ms"]["device_with_upload"] = wall(lambda: tr.val(fresh(), gts, split, predictor=pred, metrics="device"),
                                                        args.reps)
            cell["scoring_ms"]["device"] = wall(device_scoring, args.reps)
            one = disps[0][0].float().contiguous()
            us, events = kernel_us(lambda: dg.score(one, 0, split), "eval_select_pass")
            total, _ = kernel_us(lambda: dg.score(one, 0, split), "eval_")
            region = dg.max_region(split, 0, B)
            read = 4 * 2 * 4 * region                                    # 4 passes x (pred, gt) x 4 bytes x region pixels
            cell["select"] = {"us_per_image": round(us / B, 3), "bytes_read_per_image": read,
                              "floor_us_per_image_at_6.3TBps": round(read / 6.3e12 * 1e6, 3),
                              "all_scoring_kernels_us_per_image": round(total / B, 3), "device_events_per_batch": events}
            h = tr.val(fresh(), gts, split, predictor=pred)
            d = tr.val(fresh(), dg, split, predictor=pred, metrics="device")
            cell["max_rel_difference_of_the_7_errors"] = float(max(np.max(np.abs(a - b) / np.abs(b)) for a, b in zip(d, h)))
        cell["metric_share_of_host_val"] = round(1 - cell["predict_ms"] / cell["val_ms"]["host"], 4)
        cells[split] = cell
        del model, tr, pred
        torch.cuda.empty_cache()
    res = {"metric": "Trainer.val wall ms per split (both networks), bf16 DepthPredictor graph replay at B=12, median of reps",
           "reps": args.reps, "device": torch.cuda.get_device_name(0), "cells": cells,
           "command": "python tools/bench_val.py --reps %d" % args.reps}
    if args.repeat_of:
        runs = [json.load(open(f))["cells"] for f in args.repeat_of] + [cells]
        res["runs"] = len(runs)
        res["val_ms_runs"] = {c: {k: [r[c]["val_ms"][k] for r in runs] for k in cells[c]["val_ms"]} for c in cells}
        if has_device:
            res["device_faster_than_host_by_more_than_spread"] = {
                c: bool(max(r[c]["val_ms"]["device"] for r in runs) < min(r[c]["val_ms"]["host"] for r in runs)) for c in cells}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
