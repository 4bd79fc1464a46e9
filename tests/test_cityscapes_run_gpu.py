"""The Cityscapes run (ppeadepth/train.py under --train_cs --dc) on the GPU, at B = 2, 64 x 96 with the 31B model and the
conditioned synthetic weights of tests/test_train_loop_gpu.py, on a synthetic folder (tests/cityscapes_folder.py): triplets of
48 x 3*128, 12 train lines (6 steps per epoch), 3 evaluation items of 64 x 128 and ground truth of 400 x 320, the smallest
map for which the fixed [256:, 192:1856] crop of the top three quarters leaves a region (44 x 128).

  * `Run.train()` equals a hand-written loop over reader, `CityscapesInputPipeline` and `engine.step` BIT FOR BIT (rows and
    final engine state), eager and captured, over 2 epochs with the schedule stepping;
  * a run stopped after 3 of 6 steps, saved and resumed by a fresh model (`dc_ft_init` first), trainer, engine and `Run`
    equals the uninterrupted run; the decoder adapters' moments are in adam.pth where `model.parameters()` order puts them;
  * a Stage-1 checkpoint through `Run.start`: its weights, fresh adapters, an empty Adam, and a captured step that moves them;
  * validation from the device-resident store equals validation through the loader, in batches and in all 7 x 2 numbers, and
    reads no item again; device metrics on `DeviceGroundTruth.from_folder` against the host protocol;
  * `train.main` end to end at the size --train_cs sets (192 x 512), and `train.main --eval` on its checkpoint.
The sizes below 192 x 512 set `opt.dataset` themselves: `--train_cs` would rewrite height and width."""
import os
import shutil

import numpy as np
import pytest
import torch

import cityscapes_folder
from oracle import synth

pytestmark = pytest.mark.gpu

B, H, W, SEED = 2, 64, 96, 3
RTOL = 1e-5              # tests/test_eval_device_gpu.py:16, used for its Cityscapes case at :149 and for Trainer.val at :228


@pytest.fixture(scope="module")
def cs(tmp_path_factory):
    return cityscapes_folder.make(tmp_path_factory.mktemp("csrun"), (48, 128), (64, 128), 12, 3, gt_hw=(400, 320))


def _flags(cs, *more):
    return ["--data_path", cs["data"], "--cs_eval_path", cs["eval"], "--splits_dir", cs["splits"], "--num_workers", "0",
            "--ckpt_dir", os.path.join(cs["root"], "ckpt")] + list(more)


def _args(cs, *more):
    from ppeadepth import train
    return train._run_parser().parse_args(_flags(cs, *more))


def _build(device, dc=True, **overrides):
    """Model, trainer and engine in `train.main`'s order (dc_ft_init before the device, the trainer and the engine; bf16 with
    bf16 parameters), with conditioned synthetic weights, sized 64 x 96."""
    from ppeadepth import networks, options
    from ppeadepth.dist import TrainEngine
    from ppeadepth.trainer import Trainer
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=True, scheduler_step_size=1, num_epochs=2,
                                  dc=dc, **overrides)
    opt.dataset = "cityscapes_preprocessed"
    model = networks.RepDepth(opt)
    if dc:
        model.dc_ft_init()
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


def _is_adapter(name):
    return "adpt" in name or "adapter" in name


def _decoder_adapters(model):
    return {n: p for n, p in model.named_parameters() if n.startswith(("depth.", "mono_depth.")) and _is_adapter(n)}


def _quiet():
    from ppeadepth import rng
    rng.set_aug_buffer(None)
    rng.set_mode("device")


def _by_hand(device, cs, steps, capture):
    """The loop written out: reader, collate, pipeline and `engine.step` with the run's seeds -> (rows, final state)."""
    from ppeadepth import datasets, train
    from ppeadepth.input_pipeline import CityscapesInputPipeline
    model, tr, eng = _build(device)
    data = datasets.CityscapesPreprocessedDataset(cs["data"], cs["train"])
    assert data.raw_hw == (48, 128)
    pipe = CityscapesInputPipeline(device, H, W, data.raw_hw, frame_idxs=(0, -1, 1))
    gen = torch.Generator()

    def batch(g):
        gen.manual_seed(train.step_seed(SEED, g))
        triplets, cameras = datasets.collate_cityscapes([data[i] for i in train.item_indices(g, len(data), B)])
        return pipe(triplets, cameras, generator=gen)
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
            tr.epoch = (g + 1) // 6
    return rows, _engine_state(eng)


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
def test_the_cityscapes_loop_equals_a_hand_written_loop_bit_for_bit(device, cs, capture):
    from ppeadepth import rng, train
    try:
        rng.set_mode("device")
        want_rows, want_state = _by_hand(device, cs, 12, capture)
        model, tr, eng = _build(device)
        names = {id(p) for p in _decoder_adapters(model).values()}
        assert names and names <= {id(p) for p in model.parameters() if p.requires_grad}
        args = _args(cs, "--early_val_step", "0", "--validate_every", "1000", "--log_every", "5",
                     *([] if capture else ["--no_capture"]))
        run = train.Run(tr, eng, args, seed=SEED, out=lambda *a: None)
        assert (args.split, args.eval_split) == ("cityscapes_preprocessed", "cityscapes") and run.steps_in_epoch == 6
        run.start()
        assert (eng.graph is not None) == capture and tr.step == 0
        rows = run.train()
        assert [r["step"] for r in rows] == list(range(12)) and tr.step == 12
        for r, w in zip(rows, want_rows):
            assert set(w) == set(train.LOG_NAMES)
            assert _row_bytes(r, train.LOG_NAMES) == {k: w[k].astype(np.float32).tobytes() for k in train.LOG_NAMES}, r["step"]
        assert all(r["lr"] == np.float32(1e-4) for r in rows[:6]) and all(r["lr"] == np.float32(1e-4 * 0.1) for r in rows[6:])
        assert eng.scheduler.last_epoch == 2 and all(r["grad_nonfinite"] == 0 for r in rows)
        _same(want_state, _engine_state(eng), "state")
    finally:
        _quiet()


def test_a_resumed_stage2_run_equals_the_uninterrupted_run_bit_for_bit(device, cs):
    from ppeadepth import checkpoint, train
    quiet = ["--early_val_step", "0", "--validate_every", "1000", "--log_every", "4"]
    folder = os.path.join(cs["root"], "resume_ckpt")
    try:
        _quiet()
        model, tr, eng = _build(device)
        run = train.Run(tr, eng, _args(cs, *quiet, "--max_steps", "6"), seed=SEED, out=lambda *a: None)
        run.start()
        rows_a = run.train()
        state_a = _engine_state(eng)
        assert len(rows_a) == 6 and tr.step == 6
        del model, tr, eng, run
        model, tr, eng = _build(device)
        run = train.Run(tr, eng, _args(cs, *quiet, "--max_steps", "3"), seed=SEED, out=lambda *a: None)
        run.start()
        assert len(run.train()) == 3 and tr.step == 3
        tr.save_model_debug(folder, eng)
        # adam.pth: index i is the i-th tensor of `[p for p in model.parameters() if p.requires_grad]`, adapters included
        adam = checkpoint.read_folder(folder, False).adam
        trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        at = [i for i, (n, _) in enumerate(trainable) if n in _decoder_adapters(model)]
        assert at and len(adam["param_groups"][0]["params"]) == len(trainable)
        for i in at:
            m = adam["state"][i]["exp_avg"]
            assert tuple(m.shape) == tuple(trainable[i][1].shape) and float(m.abs().sum()) > 0, trainable[i][0]
        del model, tr, eng, run
        model, tr, eng = _build(device, load_weights_folder=folder)
        train.seed_all(99)
        run = train.Run(tr, eng, _args(cs, *quiet, "--max_steps", "3", "--resume"), seed=SEED, out=lambda *a: None)
        run.start()
        assert tr.step == 3 and eng.graph is not None
        rows_b = run.train()
        assert [r["step"] for r in rows_b] == [3, 4, 5] and tr.step == 6
        names = train.LOG_NAMES + ("grad_l2", "grad_max_abs")
        for a, b in zip(rows_a[3:], rows_b):
            assert _row_bytes(a, names) == _row_bytes(b, names), a["step"]
        _same(state_a, _engine_state(eng), "state")
    finally:
        shutil.rmtree(folder, ignore_errors=True)
        _quiet()


def test_a_stage1_checkpoint_hands_over_to_the_stage2_run(device, cs):
    from ppeadepth import checkpoint, train
    quiet = ["--early_val_step", "0", "--validate_every", "1000", "--log_every", "4"]
    folder = os.path.join(cs["root"], "stage1_ckpt")
    try:
        _quiet()
        model, tr, eng = _build(device, dc=False)                  # Stage 1: no decoder adapter, the decoders train
        assert not _decoder_adapters(model)
        run = train.Run(tr, eng, _args(cs, *quiet, "--max_steps", "2", "--no_capture"), seed=SEED, out=lambda *a: None)
        run.start()
        assert len(run.train()) == 2
        tr.save_model_debug(folder, eng)
        del model, tr, eng, run
        stage1 = checkpoint.read_folder(folder, False).model
        model, tr, eng = _build(device, load_weights_folder=folder)
        before = eng.checkpoint_state().model
        fresh = {n: before[n].float().clone() for n in _decoder_adapters(model)}
        moved = [k for k, v in stage1.items() if k.startswith("depth.") and v.dtype.is_floating_point
                 and not torch.equal(v, before[k])]
        assert moved                                               # Stage 1 trained what Stage 2 freezes: its decoder
        run = train.Run(tr, eng, _args(cs, *quiet, "--max_steps", "1"), seed=SEED, out=lambda *a: None)
        run.start()
        assert eng.graph is not None and tr.step == 0
        docs = eng.checkpoint_state()
        # student, teacher and pose weights and statistics are the file's: bit for bit what trains (fp32 masters) and every
        # buffer; a frozen dense weight is held in bf16 by a bf16-parameter engine (dist.TrainEngine._to_bf16_params, "frozen
        # ones once and for all"), so there the engine holds the file's value rounded to bf16 and nothing else
        frozen = {n for n, p in model.named_parameters() if not p.requires_grad}

        def held(k, v):
            return v.bfloat16().to(v.dtype) if k in frozen and v.dtype.is_floating_point else v
        assert set(moved) <= frozen
        for k, v in stage1.items():
            assert torch.equal(docs.model[k], v) or (k in frozen and torch.equal(docs.model[k], held(k, v))), k
        assert all(torch.equal(docs.model[k], v) for k, v in stage1.items() if k not in frozen)
        assert fresh and not set(fresh) & set(stage1)
        for n, v in fresh.items():                                 # the adapters: as drawn
            assert torch.equal(docs.model[n].float(), v), n
        assert docs.adam["state"] == {}                            # Adam: nothing of Stage 1
        rows = run.train()
        assert len(rows) == 1 and np.isfinite(rows[0]["loss"]) and rows[0]["grad_nonfinite"] == 0
        after = eng.checkpoint_state().model
        changed = [n for n, v in fresh.items() if not torch.equal(after[n].float(), v)]
        print(f"{len(changed)} of {len(fresh)} decoder-adapter tensors moved in one captured step")
        assert changed
        for k in moved:                                            # and the frozen decoder stays the checkpoint's
            assert torch.equal(after[k], docs.model[k]) and not torch.equal(after[k], before[k]), k
    finally:
        shutil.rmtree(folder, ignore_errors=True)
        _quiet()


class _Counting:
    """A dataset that counts the items it is asked for."""

    def __init__(self, data):
        self.data, self.reads, self.raw_hw = data, 0, data.raw_hw

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        self.reads += 1
        return self.data[i]


def test_validation_from_the_store_equals_validation_through_the_loader(device, cs):
    from ppeadepth import datasets, train
    try:
        _quiet()
        model, tr, eng = _build(device)
        counted = _Counting(datasets.CityscapesEvalDataset(cs["eval"], cs["test"]))
        quiet = lambda *a: None
        run = train.Run(tr, eng, _args(cs), seed=SEED, out=quiet, val_data=counted)
        assert run.val_store is not None and not run.val_store.complete and run.val_pipe.backend == "hip"
        first = run.validate()
        assert counted.reads == 3 and run.val_store.complete
        assert tuple(run.val_store.colors.shape) == (3, 2, 3, H, W) and run.val_store.colors.dtype == torch.uint8
        second = run.validate()
        assert counted.reads == 3                                  # no loader iterator, no item read
        off = train.Run(tr, eng, _args(cs), seed=SEED, out=quiet, val_data=counted, val_store=False)
        assert off.val_store is None
        loader = off.validate()
        assert counted.reads == 6
        for name, m in (("first", first), ("second", second), ("loader", loader)):
            print(name, m[0], m[1])
            assert len(m) == 2 and all(v.shape == (7,) and np.isfinite(v).all() for v in m)
        assert np.array_equal(np.stack(first), np.stack(second)) and np.array_equal(np.stack(first), np.stack(loader))
        # the batches themselves, in what the predictor reads
        got, want = list(run.val_store.batches(B)), list(off.loader_val_batches())
        assert [g[("color", 0, 0)].shape[0] for g in got] == [2, 1] == [w[("color", 0, 0)].shape[0] for w in want]
        for g, w in zip(got, want):
            assert set(g) == {("color", 0, 0), ("color", -1, 0), ("K", 2), ("inv_K", 2)}
            for k in g:
                assert g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), k
        # device metrics on the single-file ground truth against the host protocol on the same predictions
        gt = [np.load(os.path.join(cs["splits"], "cityscapes", "gt_depths", f"{i:03d}_depth.npy")) for i in range(3)]
        run.predictor.refresh()
        host = tr.val(off.loader_val_batches(), gt, "cityscapes", predictor=run.predictor, metrics="host")
        for d, h in zip(first, host):
            rel = np.abs(d - h) / np.abs(h)
            print(f"device {d}\n  host {h}\n   rel {rel.max():.3e}")
            assert rel.max() <= RTOL
        assert run.ground_truth().shapes == [(400, 320)] * 3
    finally:
        _quiet()


@pytest.fixture(scope="module")
def main_run(device, cs):
    """`train.main --train_cs --dc` once (192 x 512): 5 steps, validation after steps 2 (early) and 4 (regular, saved)."""
    from ppeadepth import train
    model_flags = ["--batch_size", str(B), "--train_cs", "--dc", "--adapter", "--use_checkpoint", "--weights_init", "scratch",
                   "--name", "cs"]
    try:
        _quiet()
        code = train.main(_flags(cs, "--max_steps", "5", "--validate_every", "4", "--early_val_step", "2", "--log_every", "2",
                                 "--pytorch_random_seed", str(SEED)) + model_flags)
    finally:
        _quiet()
    run = train.last_run
    folder = os.path.join(cs["root"], "ckpt", "cs_s4")
    yield {"code": code, "run": run, "rows": run.rows, "validations": run.validations, "folder": folder,
           "model_flags": model_flags}
    shutil.rmtree(os.path.join(cs["root"], "ckpt"), ignore_errors=True)


def test_main_trains_validates_and_saves_on_cityscapes(main_run):
    assert main_run["code"] == 0
    assert os.listdir(os.path.join(os.path.dirname(main_run["folder"]))) == ["cs_s4"]
    assert sorted(os.listdir(main_run["folder"])) == ["adam.pth", "model.pth", "track.pth"]
    assert [s for s, _ in main_run["validations"]] == [2, 4]
    for _, (student, teacher) in main_run["validations"]:
        assert student.shape == teacher.shape == (7,) and np.isfinite(student).all() and np.isfinite(teacher).all()
    rows, run = main_run["rows"], main_run["run"]
    assert [r["step"] for r in rows] == [0, 1, 2, 3, 4]
    assert all(np.isfinite(r["loss"]) and r["grad_l2"] > 0 and r["grad_nonfinite"] == 0 for r in rows)
    assert (run.opt.height, run.opt.width) == (192, 512) and run.cityscapes and run.val_store.complete
    assert tuple(run.val_store.colors.shape) == (3, 2, 3, 192, 512)


def test_main_eval_returns_the_numbers_of_the_last_validation(cs, main_run):
    from ppeadepth import train
    try:
        _quiet()
        assert train.main(_flags(cs, "--eval") + main_run["model_flags"] + ["--load_weights_folder", main_run["folder"]]) == 0
        (_, (student, teacher)), = train.last_run.validations
        step, (want_student, want_teacher) = main_run["validations"][-1]
        print(f"--eval {student} {teacher}\nstep {step} {want_student} {want_teacher}")
        assert step == 4 and np.array_equal(student, want_student) and np.array_equal(teacher, want_teacher)
    finally:
        _quiet()
