#!/usr/bin/env python3
"""What a checkpoint costs the step loop, and how long the files take (profiles/checkpoint.json).

    python tools/bench_checkpoint.py [--out profiles/checkpoint.json] [--runs 3] [--folder DIR]

31B, B = 12, 192 x 640, bf16 with bf16 parameters, the whole step captured in one hipGraph (bench.py's configuration), one
GPU.  All variants run in ONE session, alternating, `--runs` times each:

  (a) step_loop_loss_ms: wall time from before the save call to the end of the NEXT replay (device idle again), minus a plain
      replay.  Variants:
        parent            what the tree offered before checkpoints: export_state_dict() plus optimizer.state_dict(), moved to
                          the host.  On the flat layout torch's optimizer object never steps, so this does NOT hold the Adam
                          moments (holds_moments false): it is not a resumable checkpoint, and the gap is why the feature exists.
        blocking_docs     checkpoint_state()                 -- the three documents in host memory
        nonblocking_docs  checkpoint_state(blocking=False)   -- wait() after the replay, outside the measured span
        blocking_files    Trainer.save_model_debug(folder, engine)                   -- the three files on disk
        nonblocking_files Trainer.save_model_debug(folder, engine, blocking=False)   -- written by the writer thread
  (b) files_on_disk_s: wall time from the save call until model.pth, track.pth and adam.pth are on disk (blocking; and
      non-blocking, where it overlaps the next replay), their sizes, and load_s: `Trainer.load_model(folder, engine)` into a
      fresh engine, followed by a bit-for-bit comparison of that engine's documents with the saved ones.
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppea-depth_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(device, B, H, W):
    from ppeadepth import dist as pdist
    from ppeadepth import networks, options
    from ppeadepth import synthetic as synth
    from ppeadepth.trainer import Trainer
    opt = options.default_options(height=H, width=W, batch_size=B)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model)
    model.to(device).train()
    trainer = Trainer(opt, model, device, amp_dtype=torch.bfloat16)
    return trainer, pdist.TrainEngine(trainer, bf16_params=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint.json"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--folder", default=None, help="where the checkpoint files go (default: a temporary folder, removed)")
    args = ap.parse_args()
    from ppeadepth import rng
    from ppeadepth import synthetic as synth
    assert torch.cuda.is_available(), "bench_checkpoint.py needs a HIP device"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, H, W = args.batch, args.height, args.width
    trainer, engine = build(device, B, H, W)
    rng.set_mode("device")
    inputs = {k: v.to(device) for k, v in synth.make_inputs(B, H, W, seed=1234, smooth=True).items()}
    random.seed(1000)
    engine.capture(inputs, warmup=1)
    for _ in range(3):
        engine.step(inputs)
    torch.cuda.synchronize()

    def replay():
        # the end of the replay as the step loop sees it: engine.step orders the caller's stream behind the step stream.  (A
        # device-wide synchronize would also wait for the copy stream of a pending non-blocking save.)
        engine.step(inputs)
        torch.cuda.current_stream().synchronize()

    def span(save):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        handle = save()
        t1 = time.perf_counter()
        replay()
        return time.perf_counter() - t0, t0, t1 - t0, handle

    plain = []
    for _ in range(7):
        t0 = time.perf_counter()
        replay()
        plain.append(time.perf_counter() - t0)
    plain_s = statistics.median(plain)

    folder = args.folder or tempfile.mkdtemp(prefix="ppea_ckpt_")
    parent_holds_moments = None

    def parent():
        nonlocal parent_holds_moments
        sd = {k: v.cpu() for k, v in engine.export_state_dict().items()}
        osd = engine.optimizer.state_dict()
        state = {i: {k: (x.cpu() if torch.is_tensor(x) else x) for k, x in st.items()} for i, st in osd["state"].items()}
        parent_holds_moments = len(state) > 0
        return sd, state

    variants = {
        "parent": parent,
        "blocking_docs": lambda: engine.checkpoint_state(),
        "nonblocking_docs": lambda: engine.checkpoint_state(blocking=False),
        "blocking_files": lambda: trainer.save_model_debug(folder, engine),
        "nonblocking_files": lambda: trainer.save_model_debug(folder, engine, blocking=False),
    }
    loss_ms = {k: [] for k in variants}
    done_s = {"blocking_files": [], "nonblocking_files": [], "nonblocking_docs": []}
    try:
        engine.checkpoint_state()                    # first use builds the pack table and the staging buffers: not timed
        for _ in range(args.runs):
            for name, save in variants.items():
                dt, t0, call_s, handle = span(save)
                loss_ms[name].append((dt - plain_s) * 1e3)
                if name.startswith("nonblocking"):
                    handle.wait()
                    done_s[name].append(time.perf_counter() - t0)
                elif name == "blocking_files":
                    done_s[name].append(call_s)              # the files exist when the call returns
                del handle
        sizes = {f: os.path.getsize(os.path.join(folder, f)) for f in ("model.pth", "track.pth", "adam.pth")}
        # (b) load into a fresh engine: one more save at this boundary, whose documents the loaded engine must reproduce
        saved = trainer.save_model_debug(folder, engine)
        trainer2, engine2 = build(device, B, H, W)
        load_s = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer2.load_model(folder, engine2)
            torch.cuda.synchronize()
            load_s.append(time.perf_counter() - t0)
        again = engine2.checkpoint_state()
        equal = all(torch.equal(again.model[k], v) for k, v in saved.model.items()) and \
            all(torch.equal(again.adam["state"][i][k], st[k]) for i, st in saved.adam["state"].items() for k in st)
    finally:
        if args.folder is None:
            shutil.rmtree(folder, ignore_errors=True)

    def stats(xs, digits=1):
        return {"runs": [round(x, digits) for x in xs], "median": round(statistics.median(xs), digits),
                "spread_max_minus_min": round(max(xs) - min(xs), digits)}
    result = {
        "config": f"31B B={B} {H}x{W} bf16 + bf16 params, captured step, 1 GPU, {args.runs} runs per variant, alternating",
        "device": torch.cuda.get_device_name(0),
        "plain_replay_ms": stats([x * 1e3 for x in plain]),
        "step_loop_loss_ms": {k: stats(v) for k, v in loss_ms.items()},
        "parent_holds_moments": parent_holds_moments,
        "files_on_disk_s": {"blocking": stats(done_s["blocking_files"], 3), "nonblocking": stats(done_s["nonblocking_files"], 3)},
        "nonblocking_docs_ready_s": stats(done_s["nonblocking_docs"], 3),
        "file_bytes": sizes,
        "load_s": stats(load_s, 3),
        "loaded_engine_equals_saved_bit_for_bit": bool(equal),
        "segments_in_one_pack_launch": len(engine._ckpt_layout.nbytes),
        "packed_bytes": int(engine._ckpt_layout.total),
    }
    for pair in ("docs", "files"):
        b, n = result["step_loop_loss_ms"]["blocking_" + pair], result["step_loop_loss_ms"]["nonblocking_" + pair]
        spread = max(b["spread_max_minus_min"], n["spread_max_minus_min"])
        result["nonblocking_wins_" + pair] = bool(b["median"] - n["median"] > spread)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
