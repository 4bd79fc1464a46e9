#!/usr/bin/env python3
"""What a Cityscapes run costs around the step (profiles/cityscapes_run.json).

    python tools/bench_cityscapes_run.py [--out profiles/cityscapes_run.json] [--items 96] [--steps 100] [--rounds 3]

31B, --train_cs --dc at 192 x 512, bf16 with bf16 parameters, the step captured in one hipGraph, one GPU.  Synthetic frames are
written to a temporary folder at the real sizes: triplet JPEGs of 384 x 3072, evaluation PNGs of 1024 x 2048 with their
sequence frames, ground truth of 1024 x 2048 as single .npy files; the evaluation split has `--items` items (the real one
1525; figures "scaled" below are multiplied by 1525 / items).

  (a) one validation through the loader path: decode on `--num_workers` CPU workers, upload, evaluation pipeline, predict, score;
  (b) one validation through the device-resident store (valstore.py): predict and score, nothing decoded or uploaded;
      (a) and (b) are timed in one session, `--rounds` times each in alternating order, wall clock around `Run.validate()`
      (which ends in the copy of the metrics to the host);
  (c) the loop's step against the bare replay of the same engine on static inputs, as tools/bench_train_loop.py does.
Recorded, not gated: no earlier build runs this path.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppea-depth_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

REAL_SPLIT = 1525


def _frame(g, h, w, phase):
    """A smooth image with noise: compresses neither like a flat field nor like white noise."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 90 * np.sin(x / 37.0 + phase + c) * np.cos(y / 23.0) for c in range(3)], -1)
    return np.clip(img + g.normal(0, 8, img.shape), 0, 255).astype(np.uint8)


def write_folder(root, items, distinct, train_lines):
    from PIL import Image
    g = np.random.default_rng(0)
    data, raw, splits = (os.path.join(root, d) for d in ("triplets", "cityscapes", "splits"))
    names = []
    os.makedirs(os.path.join(data, "ulm"))
    wide, full = _frame(g, 384, 3 * 1024, 0.0), _frame(g, 1024, 2048, 0.0)      # rolled per file: distinct bytes, one synthesis
    for i in range(distinct):
        name = f"ulm_{i:06d}_000019"
        Image.fromarray(np.roll(wide, 41 * i, 1)).save(os.path.join(data, "ulm", name + ".jpg"), quality=92)
        with open(os.path.join(data, "ulm", name + "_cam.txt"), "w") as f:
            f.write("1131.3125,0.0,523.4375,0.0,1130.03125,191.265625,0.0,0.0,1.0\n")
        names.append("ulm " + name)
    test = []
    for folder in ("leftImg8bit", "leftImg8bit_sequence"):
        os.makedirs(os.path.join(raw, folder, "test", "ulm"))
    os.makedirs(os.path.join(raw, "camera_trainvaltest", "camera", "test", "ulm"))
    os.makedirs(os.path.join(splits, "cityscapes", "gt_depths"))
    os.makedirs(os.path.join(splits, "cityscapes_preprocessed"))
    for i in range(items):
        name = f"ulm_{i:06d}_000019"
        for folder, frame, shift in (("leftImg8bit", name, 2 * i), ("leftImg8bit_sequence", f"ulm_{i:06d}_000017", 2 * i + 1)):
            Image.fromarray(np.roll(full, 29 * shift, 1)).save(
                os.path.join(raw, folder, "test", "ulm", frame + "_leftImg8bit.png"), compress_level=1)
        with open(os.path.join(raw, "camera_trainvaltest", "camera", "test", "ulm", name + "_camera.json"), "w") as f:
            json.dump({"intrinsic": {"fx": 2262.52, "fy": 2265.3017905988554, "u0": 1096.98, "v0": 513.137}}, f)
        np.save(os.path.join(splits, "cityscapes", "gt_depths", str(i).zfill(3) + "_depth.npy"),
                g.uniform(2.0, 60.0, (1024, 2048)).astype(np.float32))
        test.append("ulm " + name)
    for name, lines in (("train", [names[i % distinct] for i in range(train_lines)]), ("test", test)):
        with open(os.path.join(splits, "cityscapes_preprocessed", f"{name}_files.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return data, raw, splits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cityscapes_run.json"))
    ap.add_argument("--items", type=int, default=96)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--num_workers", type=int, default=12)
    args = ap.parse_args()
    from ppeadepth import dist as pdist
    from ppeadepth import networks, options, rng, train
    from ppeadepth import synthetic as synth
    from ppeadepth.trainer import Trainer
    assert torch.cuda.is_available(), "bench_cityscapes_run.py needs a HIP device"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B = args.batch
    steps = 60 + args.steps
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        data, raw, splits = write_folder(root, args.items, 24, B * steps)
        write_s = time.perf_counter() - t0
        print(f"folder written in {write_s:.1f} s", file=sys.stderr, flush=True)
        opt = options.apply_train_cs(options.default_options(batch_size=B, num_epochs=1, dc=True, train_cs=True))
        torch.manual_seed(0)
        model = networks.RepDepth(opt)
        model.dc_ft_init()
        synth.fill_state_dict(model)
        model.to(device).train()
        trainer = Trainer(opt, model, device, amp_dtype=torch.bfloat16)
        engine = pdist.TrainEngine(trainer, bf16_params=True)
        rng.set_mode("device")

        def flags():
            return train._run_parser().parse_args(
                ["--data_path", data, "--cs_eval_path", raw, "--splits_dir", splits, "--num_workers", str(args.num_workers),
                 "--log_every", "50", "--early_val_step", "0", "--validate_every", str(10 ** 9), "--saveoff",
                 "--max_steps", str(steps)])
        run = train.Run(trainer, engine, flags(), seed=1, out=lambda *a: None)
        loader_run = train.Run(trainer, engine, flags(), seed=1, out=lambda *a: None, val_store=False)
        run.start()

        # ---- the ground truth and the store: what stays on the device ---------------------------------------------------
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        loader_run._gt = run.ground_truth()
        torch.cuda.synchronize()
        gt_s, gt_bytes = time.perf_counter() - t0, torch.cuda.memory_allocated() - m0

        def timed(r):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = r.validate()
            return time.perf_counter() - t0, m
        fill_s, first = timed(run)                                  # the first validation: loader path + filling the store
        assert run.val_store.complete
        print(f"ground truth {gt_s:.1f} s, first validation {fill_s:.1f} s", file=sys.stderr, flush=True)
        loader_s, store_s, same = [], [], True
        for k in range(args.rounds):                               # alternating order
            for which in (("loader", "store") if k % 2 == 0 else ("store", "loader")):
                s, m = timed(loader_run if which == "loader" else run)
                (loader_s if which == "loader" else store_s).append(s)
                same = same and np.array_equal(np.stack(m), np.stack(first))

        # ---- (c) the loop against the bare replay -----------------------------------------------------------------------
        stamps = {}
        check = run.check_log

        def stamped():
            rows = check()
            if rows:
                stamps[rows[-1]["step"]] = time.perf_counter()
            return rows
        run.check_log = stamped
        print(f"loader {loader_s} store {store_s}", file=sys.stderr, flush=True)
        run.train()
        last = max(s for s in stamps if s % 50 == 0)
        loop_ms = (stamps[last] - stamps[50]) * 1e3 / (last - 50)
        inputs = run.first_batch()
        for _ in range(5):
            engine.step(inputs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            engine.step(inputs)
        torch.cuda.synchronize()
        bare_ms = (time.perf_counter() - t0) * 1e3 / args.steps

    scale = REAL_SPLIT / args.items
    a, b = statistics.median(loader_s), statistics.median(store_s)
    result = {
        "config": f"31B --train_cs --dc B={B} 192x512 bf16 + bf16 params, captured step, 1 GPU; {args.items}-item evaluation "
                  f"split of 1024x2048 PNGs, {args.num_workers} loader workers, {os.cpu_count()} CPUs visible",
        "device": torch.cuda.get_device_name(0),
        "folder_write_s": round(write_s, 1),
        "validation": {
            "items": args.items, "rounds": args.rounds,
            "loader_path_s": [round(x, 3) for x in loader_s], "store_path_s": [round(x, 3) for x in store_s],
            "loader_path_s_median": round(a, 3), "store_path_s_median": round(b, 3), "loader_over_store": round(a / b, 2),
            "first_validation_filling_the_store_s": round(fill_s, 3),
            "scaled_to_1525_items": {"loader_path_s": round(a * scale, 1), "store_path_s": round(b * scale, 1),
                                     "steps_between_validations_s_at_1000_steps": round(loop_ms, 1)},
            "metrics_equal_across_paths": bool(same),
        },
        "resident": {
            "store_bytes": int(run.val_store.nbytes()), "store_bytes_scaled": int(run.val_store.nbytes() * scale),
            "ground_truth_bytes": int(gt_bytes), "ground_truth_bytes_scaled": int(gt_bytes * scale),
            "ground_truth_upload_s": round(gt_s, 2),
        },
        "loop": {"steps_timed": int(last - 50), "run_step_ms": round(loop_ms, 3), "bare_replay_ms": round(bare_ms, 3),
                 "difference_ms": round(loop_ms - bare_ms, 3)},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
