"""The training run (ppeadepth/train.py) on the GPU, at B = 2, 64 x 96 with the 31B model of tests/test_checkpoint_gpu.py and a
KITTI-layout folder of small JPEGs of two frame sizes: 12 train lines (6 steps per epoch), 3 test lines and a gt_depths.npz.

  * `Run.train()` equals a hand-written loop over the same pipeline and `engine.step` calls BIT FOR BIT (rows and final
    engine state), eager and captured, over 2 epochs with the schedule stepping after each; the gradient columns of the last
    row equal the float64 norm / max of `engine.named_grads()`;
  * a run stopped after 3 steps, saved and resumed by a fresh trainer, engine and `Run` equals the uninterrupted 6 steps;
  * `train.main` end to end (log, two validations, a checkpoint) and `train.main --eval` on that checkpoint.
Everything but the gradient norm is compared with torch.equal / bytes: there is no tolerance on the loop."""
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

B, H, W, SEED = 2, 64, 96, 3
L2_RTOL = 2.0 ** -21               # tests/test_run_monitor_gpu.py


@pytest.fixture(scope="module")
def kitti(tmp_path_factory):
    """Two drives of two frame sizes, 8 frames each; train lines = frames 1..6 of both (every batch of two mixes the sizes),
    test lines = three frames; ground truth = positive random maps at the frames' sizes."""
    from PIL import Image
    root = tmp_path_factory.mktemp("run")
    g = np.random.default_rng(3)
    drives = {"2011_09_26/drive_a_sync": (100, 300), "2011_09_28/drive_b_sync": (110, 330)}
    for folder, (h, w) in drives.items():
        d = root / "kitti" / folder / "image_02" / "data"
        os.makedirs(d)
        for i in range(8):
            y, x = np.mgrid[0:h, 0:w]
            img = np.stack([127 + 100 * np.sin(x / 17.0 + i + c) * np.cos(y / 11.0) for c in range(3)], -1)
            img = np.clip(img + g.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(str(d / "{:010d}.jpg".format(i)), quality=95)
    a, b = drives
    train_lines = [f"{d} {i} l" for i in range(1, 7) for d in (a, b)]
    test_lines, sizes = [f"{a} 1 l", f"{b} 2 l", f"{a} 3 l"], [drives[a], drives[b], drives[a]]
    os.makedirs(root / "splits" / "eigen_zhou")
    os.makedirs(root / "splits" / "eigen")
    for name, lines in (("train", train_lines), ("test", test_lines)):
        with open(root / "splits" / "eigen_zhou" / f"{name}_files.txt", "w") as f:
            f.write("\n".join(lines) + "\n")
    gts = np.empty(len(sizes), dtype=object)
    for i, hw in enumerate(sizes):
        gts[i] = g.uniform(2.0, 60.0, hw).astype(np.float32)
    np.savez_compressed(str(root / "splits" / "eigen" / "gt_depths.npz"), data=gts)
    return {"root": str(root), "data": str(root / "kitti"), "splits": str(root / "splits"), "train": train_lines,
            "test": test_lines}


def _flags(kitti, *more):
    return ["--data_path", kitti["data"], "--splits_dir", kitti["splits"], "--num_workers", "0",
            "--ckpt_dir", os.path.join(kitti["root"], "ckpt")] + list(more)


def _args(kitti, *more):
    from ppeadepth import train
    return train._run_parser().parse_args(_flags(kitti, *more))


def _build(device, **overrides):
    """Model, trainer and engine as `train.main` builds them (bf16, bf16 parameters), with conditioned synthetic weights."""
    from ppeadepth import networks, options
    from ppeadepth.dist import TrainEngine
    from ppeadepth.trainer import Trainer
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=True, scheduler_step_size=1, num_epochs=2,
                                  **overrides)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model, conditioned=True)
    model.to(device).train()
    tr = Trainer(opt, model, device, amp_dtype=torch.bfloat16)
    return model, tr, TrainEngine(tr, bf16_params=True)


def _same(a, b, what):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what
    elif isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)) and any(torch.is_tensor(x) or isinstance(x, (dict, list, tuple)) for x in a):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert a == b, what


def _engine_state(eng):
    docs = eng.checkpoint_state()
    tracker = eng.trainer.depth_bin_tracker
    extra = {"W16": eng.W16.detach().cpu().clone(), "adam_state": eng.adam_state.detach().cpu().clone(),
             "tracker": torch.stack([tracker.min_depth, tracker.max_depth]).cpu(), "step": eng.trainer.step,
             "lr": eng.optimizer.param_groups[0]["lr"], "schedule": eng.scheduler.last_epoch}
    return {"model": docs.model, "track": docs.track, "adam": docs.adam, "engine": extra}


def _row_bytes(row, names):
    return {k: None if row[k] is None else row[k].tobytes() for k in names}


def _by_hand(device, kitti, steps, capture):
    """The loop written out: the same pipeline and `engine.step` calls with the same seeds; -> (rows, final state)."""
    from ppeadepth import datasets, train
    from ppeadepth.input_pipeline import DeviceInputPipeline
    model, tr, eng = _build(device)
    ids = (0, -1, 1)
    data = datasets.KITTIRAWDataset(kitti["data"], kitti["train"], ids)
    pipe = DeviceInputPipeline(None, H, W, device, frame_idxs=ids)
    gen = torch.Generator()

    def batch(g):
        gen.manual_seed(train.step_seed(SEED, g))
        return pipe(datasets.collate_raw([data[i] for i in train.item_indices(g, len(data), B)]), generator=gen)
    if capture:
        eng.capture(batch(0), restore_state=True)
    train.seed_all(SEED)
    rows = []
    for g in range(steps):
        _, losses = eng.step(batch(g))
        torch.cuda.synchronize()
        row = {k: losses[k].detach().cpu().numpy().reshape(()).copy() for k in train.LOG_NAMES if k in losses}
        row["min_depth_bin"] = tr.depth_bin_tracker.min_depth.cpu().numpy().copy()
        row["max_depth_bin"] = tr.depth_bin_tracker.max_depth.cpu().numpy().copy()
        row["lr"] = eng.adam_state[1].cpu().numpy().copy()
        rows.append(row)
        if (g + 1) % 6 == 0:
            eng.scheduler_step()
            tr.epoch = (g + 1) // 6                        # what a checkpoint records beside the step
    return rows, _engine_state(eng)


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
def test_the_loop_equals_a_hand_written_loop_bit_for_bit(device, kitti, capture):
    from ppeadepth import rng, train
    try:
        rng.set_mode("device")
        want_rows, want_state = _by_hand(device, kitti, 12, capture)
        model, tr, eng = _build(device)
        args = _args(kitti, "--early_val_step", "0", "--validate_every", "1000", "--log_every", "5",
                     *([] if capture else ["--no_capture"]))
        run = train.Run(tr, eng, args, seed=SEED, out=lambda *a: None)
        run.start()
        assert (eng.graph is not None) == capture and tr.step == 0
        rows = run.train()
        assert [r["step"] for r in rows] == list(range(12)) and tr.step == 12
        for r, w in zip(rows, want_rows):
            assert set(w) == set(train.LOG_NAMES)
            assert _row_bytes(r, train.LOG_NAMES) == {k: w[k].astype(np.float32).tobytes() for k in train.LOG_NAMES}, r["step"]
        # the schedule stepped after step 5 (and 11): the lr column changes exactly at row 6 and is the optimizer's lr as fp32
        assert all(r["lr"] == np.float32(1e-4) for r in rows[:6]) and all(r["lr"] == np.float32(1e-4 * 0.1) for r in rows[6:])
        assert eng.optimizer.param_groups[0]["lr"] == pytest.approx(1e-6) and eng.scheduler.last_epoch == 2
        # gradient columns of the last row against the float64 norm / max of the step's gradients
        grads = [g.detach().double().reshape(-1) for g in eng.named_grads().values()]
        l2 = float(torch.sqrt(sum((g * g).sum() for g in grads)))
        mx = np.float32(max(float(g.abs().max()) for g in grads))
        last = rows[-1]
        print(f"grad_l2 {last['grad_l2']!r} vs {l2!r} (rel {abs(float(last['grad_l2']) - l2) / l2:.3e}), max {last['grad_max_abs']!r} vs {mx!r}")
        assert l2 > 0 and abs(float(last["grad_l2"]) - l2) <= L2_RTOL * l2
        assert last["grad_max_abs"].tobytes() == mx.tobytes() and all(r["grad_nonfinite"] == 0 for r in rows)
        _same(want_state, _engine_state(eng), "state")
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")


def test_a_resumed_run_equals_the_uninterrupted_run_bit_for_bit(device, kitti):
    from ppeadepth import rng, train
    quiet = ["--early_val_step", "0", "--validate_every", "1000", "--log_every", "4"]
    folder = os.path.join(kitti["root"], "resume_ckpt")
    try:
        rng.set_mode("device")
        model, tr, eng = _build(device)
        run = train.Run(tr, eng, _args(kitti, *quiet, "--max_steps", "6"), seed=SEED, out=lambda *a: None)
        run.start()
        rows_a = run.train()
        state_a = _engine_state(eng)
        assert len(rows_a) == 6 and tr.step == 6
        del model, tr, eng, run
        model, tr, eng = _build(device)
        run = train.Run(tr, eng, _args(kitti, *quiet, "--max_steps", "3"), seed=SEED, out=lambda *a: None)
        run.start()
        assert len(run.train()) == 3 and tr.step == 3
        tr.save_model_debug(folder, eng)
        del model, tr, eng, run
        # a fresh trainer, engine and Run, other seeds: position, schedule and random streams come from the checkpoint
        model, tr, eng = _build(device, load_weights_folder=folder)
        train.seed_all(99)
        run = train.Run(tr, eng, _args(kitti, *quiet, "--max_steps", "3", "--resume"), seed=SEED, out=lambda *a: None)
        run.start()
        assert tr.step == 3 and eng.graph is not None
        rows_b = run.train()
        assert [r["step"] for r in rows_b] == [3, 4, 5] and tr.step == 6
        names = train.LOG_NAMES + ("grad_l2", "grad_max_abs")
        for a, b in zip(rows_a[3:], rows_b):
            assert _row_bytes(a, names) == _row_bytes(b, names), a["step"]
        _same(state_a, _engine_state(eng), "state")
    finally:
        shutil.rmtree(folder, ignore_errors=True)          # most of a gigabyte
        rng.set_aug_buffer(None)
        rng.set_mode("device")


@pytest.fixture(scope="module")
def main_run(device, kitti):
    """`train.main` once: 5 steps, validation after steps 2 (early) and 4 (regular, saved), a log line every 2 steps."""
    from ppeadepth import rng, train
    model_flags = ["--height", str(H), "--width", str(W), "--batch_size", str(B), "--adapter", "--use_checkpoint",
                   "--weights_init", "scratch", "--name", "t"]
    try:
        rng.set_mode("device")
        code = train.main(_flags(kitti, "--max_steps", "5", "--validate_every", "4", "--early_val_step", "2", "--log_every", "2",
                                 "--pytorch_random_seed", str(SEED)) + model_flags)
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")
    run = train.last_run
    folder = os.path.join(kitti["root"], "ckpt", "t_s4")
    yield {"code": code, "rows": run.rows, "validations": run.validations, "folder": folder, "model_flags": model_flags}
    shutil.rmtree(os.path.join(kitti["root"], "ckpt"), ignore_errors=True)


def test_main_logs_validates_and_saves(main_run):
    assert main_run["code"] == 0
    assert sorted(os.listdir(main_run["folder"])) == ["adam.pth", "model.pth", "track.pth"]
    assert [s for s, _ in main_run["validations"]] == [2, 4]
    for _, (student, teacher) in main_run["validations"]:
        assert student.shape == teacher.shape == (7,) and np.isfinite(student).all() and np.isfinite(teacher).all()
    rows = main_run["rows"]
    assert [r["step"] for r in rows] == [0, 1, 2, 3, 4]
    assert all(np.isfinite(r["loss"]) and r["grad_l2"] > 0 and r["grad_nonfinite"] == 0 for r in rows)


def test_main_eval_scores_the_checkpoint_like_a_direct_val(device, kitti, main_run):
    from ppeadepth import datasets, evaluate, networks, options, rng, train
    from ppeadepth.dist import TrainEngine
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.input_pipeline import DeviceInputPipeline
    from ppeadepth.trainer import Trainer
    try:
        rng.set_mode("device")
        assert train.main(_flags(kitti, "--eval") + main_run["model_flags"] + ["--load_weights_folder", main_run["folder"]]) == 0
        (_, (student, teacher)), = train.last_run.validations
        opt = options.MonodepthOptions().parse(main_run["model_flags"])
        model = networks.RepDepth(opt).to(device).train()
        tr = Trainer(opt, model, device, amp_dtype=torch.bfloat16)
        eng = TrainEngine(tr, bf16_params=True)
        tr.load_model(main_run["folder"], eng)
        p = DepthPredictor(model, opt, amp_dtype=torch.bfloat16)
        ids = [0] + p.lookup_ids
        data = datasets.KITTIRAWDataset(kitti["data"], kitti["test"], ids)
        pipe = DeviceInputPipeline(None, H, W, device, frame_idxs=tuple(ids), is_train=False)
        batches = [pipe(datasets.collate_raw([data[i] for i in range(s, min(s + B, len(data)))])) for s in range(0, len(data), B)]
        gt = evaluate.DeviceGroundTruth(train.load_gt_depths(kitti["splits"], "eigen"), device)
        want = tr.val(batches, gt, "eigen", hard_test_mono=True, predictor=p, metrics="device")
        assert student.tobytes() == want[0].tobytes() and teacher.tobytes() == want[1].tobytes()
        assert np.isfinite(student).all() and np.isfinite(teacher).all()
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")
