"""The training run (reference: train.py and trainer.py:296-418 `train` / `run_epoch`).

    python -m ppeadepth.train --data_path KITTI --adapter --use_checkpoint --validate_every 3000 --num_epochs 30
    python -m ppeadepth.train --data_path KITTI --adapter --use_checkpoint --eval --load_weights_folder CKPT
    python -m ppeadepth.train --data_path CS_TRIPLETS --cs_eval_path CS_RAW --train_cs --dc --adapter --use_checkpoint \\
        --validate_every 1000 --learning_rate 1e-5 --load_weights_folder STAGE1_CKPT
    python -m ppeadepth.train --data_path CS_TRIPLETS --cs_eval_path CS_RAW --train_cs --dc --adapter --use_checkpoint \\
        --eval --load_weights_folder CKPT

Run flags (this module's parser; every other flag is a model option of `options.MonodepthOptions`):
  reference names and defaults   --data_path --split (eigen_zhou) --eval_split (eigen) --png --num_workers (12)
                                 --validate_every (1000) --validate_from (0) --save_until (0) --saveoff --eval
                                 --pytorch_random_seed (None -> 1) --cs_eval_path (../cityscapes)
  new here                       --splits_dir (splits) --ckpt_dir (./ckpt) --log_every (50) --early_val_step (250, 0 = off)
                                 --fp32 (default bf16 with bf16 parameters) --no_capture (eager steps) --resume --max_steps

The loop on this build's parts: `KITTIRAWDataset` + `collate_raw` -> `DeviceInputPipeline(None, ...)` -> `TrainEngine.step`
(a captured hipGraph unless --no_capture) -> `RunLog.append` (two launches, csrc/run_monitor.hip).  A step that is neither a log,
a validation nor a save step reads no device value on the host.  Every --log_every steps ONE copy brings the rows of the
interval back; a row with a non-finite loss or gradient raises `NonFiniteRun` and nothing is saved after it.

Data order.  The reference does not shuffle (trainer.py:215-218; the split file is shuffled already): step g of the run trains
on the items `item_indices(g, ...)` of the split file, and its augmentation draws come from a `torch.Generator` seeded with
`step_seed(seed, g)`.  The batch is therefore a function of (seed, global step) alone and a resumed run needs no loader state:
the sampler starts at the right item.

Cityscapes (--train_cs; Stage 2 of the paper with --dc).  The same `Run` with other parts: `CityscapesPreprocessedDataset` +
`collate_cityscapes` -> `CityscapesInputPipeline` for the steps, `CityscapesEvalDataset(--cs_eval_path)` +
`collate_cityscapes_eval` -> `CityscapesEvalPipeline` for validation, the ground truth from `<splits_dir>/cityscapes/gt_depths`
(`DeviceGroundTruth.from_folder`); --split and --eval_split follow the flag, and both split files are read from
`<splits_dir>/cityscapes_preprocessed`.  With --dc `main` calls `model.dc_ft_init()` before the model moves to the device and
before trainer and engine exist, so the decoder adapters are in the trainable set and train (the reference builds its Adam
first and never steps them); a Stage-1 checkpoint leaves them as drawn and its adam.pth is skipped, a Stage-2 checkpoint of
this loop restores both (the reference drops the adapter keys on load).

Validation inputs never change during a run: the first validation reads them from disk and keeps what the predictor reads
on the device as uint8 (`valstore.ValidationStore`, both datasets); later validations start no loader worker.

Not served (refused with a message): --ddad (its pipeline exists, a folder reader does not), --train_cs with
--use_future_frame or --num_matching_frames > 1 (the evaluation loader holds frames 0 and -1), several ranks
(WORLD_SIZE > 1), --freeze_teacher_and_pose and --freeze_pose; --static_camera and --zero_cost_volume are not parsed.
"""
import argparse
import os
import random
import time

import numpy as np
import torch

LOG_NAMES = ("loss", "loss/0", "reproj_loss/0", "consistency_loss/0", "min_depth_bin", "max_depth_bin", "lr")


last_run = None          # the `Run` of this process's last `main()` call: its `rows` and `validations` outlive the call


class NonFiniteRun(RuntimeError):
    """The run monitor saw a non-finite loss, scalar or gradient element; `.step` is the first such step."""

    def __init__(self, step, columns):
        self.step, self.columns = int(step), tuple(columns)
        what = ", ".join(self.columns) if self.columns else "a row that has left the log"
        super().__init__(f"the run went non-finite at step {self.step} ({what}); no checkpoint is written after it")


# ---- the plan of a run: pure functions ------------------------------------------------------------------------------------
def step_events(s, validate_every, validate_from=0, save_until=0, early_val_step=250, saveoff=False):
    """What follows the 0-based step `s` (trainer.py:366-408) -> (validate, save).  Validation runs at s == early_val_step
    (0 = off; once, also where it coincides with a regular one) and whenever s != 0, s % validate_every == 0 and
    s > validate_from; the regular points also save, unless --saveoff or s < save_until."""
    regular = s != 0 and s % validate_every == 0 and s > validate_from
    early = early_val_step > 0 and s == early_val_step
    return regular or early, regular and not saveoff and s >= save_until


def event_plan(steps_per_epoch, num_epochs, validate_every, validate_from=0, save_until=0, early_val_step=250,
               saveoff=False, start_step=0, max_steps=None):
    """The steps `start_step <= s < end` of a run at which something follows the step: {"validate": [...], "save": [...],
    "schedule": [...]} -- `schedule` lists the last step of every epoch, after which the learning-rate schedule steps
    (trainer.py:418).  end = steps_per_epoch * num_epochs, or start_step + max_steps if that is sooner."""
    end = steps_per_epoch * num_epochs
    if max_steps is not None:
        end = min(end, start_step + max_steps)
    plan = {"validate": [], "save": [], "schedule": []}
    for s in range(start_step, end):
        validate, save = step_events(s, validate_every, validate_from, save_until, early_val_step, saveoff)
        if validate:
            plan["validate"].append(s)
        if save:
            plan["save"].append(s)
        if (s + 1) % steps_per_epoch == 0:
            plan["schedule"].append(s)
    return plan


def steps_per_epoch(num_items, batch_size):
    """drop_last=True (trainer.py:217)."""
    return num_items // batch_size


def resume_position(step, steps_in_epoch):
    """Global step count (what a checkpoint stores) -> (epoch, batches of that epoch already done)."""
    return step // steps_in_epoch, step % steps_in_epoch


def item_indices(global_step, num_items, batch_size):
    """The split-file lines step `global_step` trains on: no shuffling, the last partial batch of an epoch dropped."""
    _, k = resume_position(global_step, steps_per_epoch(num_items, batch_size))
    return list(range(k * batch_size, (k + 1) * batch_size))


def step_seed(seed, global_step):
    """Seed of the generator that draws step `global_step`'s flips and colour jitter: seed * 2^32 + step (mod 2^63)."""
    return (int(seed) * (1 << 32) + int(global_step)) % (1 << 63)


class _EpochSampler(torch.utils.data.Sampler):
    """Items `start .. stop` in order; `start` is moved to the resume position for the first epoch of a resumed run."""

    def __init__(self, stop):
        self.start, self.stop = 0, stop

    def __iter__(self):
        return iter(range(self.start, self.stop))

    def __len__(self):
        return self.stop - self.start


# ---- refusals -----------------------------------------------------------------------------------------------------------
def is_cityscapes(opt):
    """`--train_cs`, before or after `options.apply_train_cs` has rewritten the options (`--ddad` wins, trainer.py:90-103)."""
    if getattr(opt, "ddad", False):
        return False
    return bool(getattr(opt, "train_cs", False)) or getattr(opt, "dataset", None) == "cityscapes_preprocessed"


def check_served(opt, args=None):
    """SystemExit for what this loop does not serve, before anything is built.  args: the run flags; with them the files a
    `--train_cs` run opens first are looked for as well (both split files, the first training image)."""
    if getattr(opt, "ddad", False):
        raise SystemExit("--ddad: the input pipeline of that dataset exists (input_pipeline.py) but no folder reader does; "
                         "ppeadepth.train serves KITTI raw and Cityscapes folders only")
    if is_cityscapes(opt):
        # the wide training image holds frames -1, 0, +1 and the evaluation loader frames 0 and -1 (cityscapes_evaldataset.py)
        if getattr(opt, "use_future_frame", False) or getattr(opt, "num_matching_frames", 1) > 1:
            raise SystemExit("--train_cs with --use_future_frame or --num_matching_frames > 1: the Cityscapes evaluation "
                             "loader holds frames 0 and -1 only, no other lookup frame can be validated")
        if args is not None:
            from . import datasets
            folder = os.path.join(args.splits_dir, "cityscapes_preprocessed")
            for name in ("train", "test"):
                path = os.path.join(folder, f"{name}_files.txt")
                if not os.path.isfile(path):
                    raise SystemExit(f"--train_cs: {path} not found (the split files of the preprocessed triplets and of "
                                     "the evaluation frames are both read from that folder: --splits_dir)")
            lines = datasets.readlines(os.path.join(folder, "train_files.txt"))
            if not lines:
                raise SystemExit(f"--train_cs: {os.path.join(folder, 'train_files.txt')} is empty")
            data = datasets.CityscapesPreprocessedDataset(args.data_path, lines)
            path = data.get_image_path(*data.index_to_folder_and_frame_idx(0)[:2])
            if not os.path.isfile(path):
                raise SystemExit(f"--train_cs: {path} not found -- make sure --data_path is the folder of the preprocessed "
                                 "triplets (<city>/<frame_name>.jpg and _cam.txt)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"WORLD_SIZE={os.environ['WORLD_SIZE']}: ppeadepth.train runs on one rank; the step itself serves "
                         "several (dist.TrainEngine), the loop around it is not measured there")
    for flag in ("freeze_teacher_and_pose", "freeze_pose"):
        if getattr(opt, flag, False):
            raise SystemExit(f"--{flag}: freeze_tp_net() and the tracker reset of trainer.py:166-173 are not wired into "
                             "ppeadepth.train")


def follow_train_cs(args, opt):
    """The split run flags follow `--train_cs` (trainer.py:90-96): split "cityscapes_preprocessed", eval_split "cityscapes"."""
    if is_cityscapes(opt):
        args.split, args.eval_split = "cityscapes_preprocessed", "cityscapes"
    return args


def load_gt_depths(splits_dir, eval_split):
    path = os.path.join(splits_dir, eval_split, "gt_depths.npz")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found: write it with python -m ppeadepth.export_gt_depth "
                                f"(--split {eval_split}) before a run that validates")
    return np.load(path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]


def _run_parser():
    p = argparse.ArgumentParser(description="PPEA-Depth training run; other flags: options.MonodepthOptions")
    a = p.add_argument
    a("--data_path", required=True)
    a("--cs_eval_path", default="../cityscapes", help="--train_cs: the raw Cityscapes folder the validation frames are in")
    a("--split", default="eigen_zhou")
    a("--eval_split", default="eigen")
    a("--png", action="store_true", help="the frames are .png files (default .jpg)")
    a("--num_workers", type=int, default=12)
    a("--validate_every", "--validate-every", type=int, default=1000)
    a("--validate_from", type=int, default=0)
    a("--save_until", type=int, default=0)
    a("--saveoff", action="store_true")
    a("--eval", action="store_true")
    a("--pytorch_random_seed", type=int, default=None)
    a("--splits_dir", default="splits")
    a("--ckpt_dir", default="./ckpt")
    a("--log_every", type=int, default=50)
    a("--early_val_step", type=int, default=250)
    a("--fp32", action="store_true", help="train in fp32 (default bf16 autocast with bf16 parameters)")
    a("--no_capture", action="store_true", help="eager steps (default: the step is captured into a hipGraph)")
    a("--resume", action="store_true", help="with --load_weights_folder: go on at the checkpoint's step")
    a("--max_steps", type=int, default=None)
    a("--device", default=None)
    return p


def seed_all(seed):
    """train.py:14-24."""
    seed = seed if seed else 1
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    return seed


# ---- the run ------------------------------------------------------------------------------------------------------------
class Run:
    """Trainer, engine, loaders, pipelines, ground truth, predictor and `RunLog` of one run; `train()` and `run_epoch()`.
    trainer, engine: built by the caller (`main` builds them from the flags).  args: the run flags (`_run_parser`)."""

    def __init__(self, trainer, engine, args, seed=1, out=print, train_data=None, val_data=None, val_store=True):
        """train_data / val_data: datasets with the item contract of the run's readers (`KITTIRAWDataset`, or under
        `--train_cs` `CityscapesPreprocessedDataset` / `CityscapesEvalDataset`) to use instead of the split files' frames
        (train_data with `opt.frame_ids` and the matching frames, val_data with frame 0 and the lookup frames).
        val_store: keep the validation inputs on the device after the first validation (`valstore.ValidationStore`);
        False: every validation goes through the loader."""
        from . import datasets
        from . import input_pipeline as ip
        from .inference import DepthPredictor
        from .runlog import RunLog
        from .valstore import ValidationStore
        self.trainer, self.engine, self.args, self.seed, self.out = trainer, engine, args, int(seed), out
        opt = self.opt = trainer.opt
        follow_train_cs(args, opt)
        check_served(opt, args if train_data is None and val_data is None else None)
        self.device = dev = trainer.device
        self.cityscapes = cs = is_cityscapes(opt)
        model = trainer._module()
        ext = ".png" if args.png else ".jpg"
        fpath = os.path.join(args.splits_dir, args.split, "{}_files.txt")
        B = opt.batch_size
        train_ids = list(opt.frame_ids) + [int(f) for f in model.matching_ids if f not in opt.frame_ids]
        self.collate, self.val_collate = ((datasets.collate_cityscapes, datasets.collate_cityscapes_eval) if cs
                                          else (datasets.collate_raw, datasets.collate_raw))
        if train_data is None and cs:
            train_data = datasets.CityscapesPreprocessedDataset(args.data_path, datasets.readlines(fpath.format("train")))
        elif train_data is None:
            train_data = datasets.KITTIRAWDataset(args.data_path, datasets.readlines(fpath.format("train")), train_ids, ext)
        self.train_data = train_data
        self.steps_in_epoch = steps_per_epoch(len(train_data), B)
        if self.steps_in_epoch < 1:
            raise SystemExit(f"{len(train_data)} training items for batches of {B}")
        self.sampler = _EpochSampler(self.steps_in_epoch * B)
        # a DataLoader draws its workers' base seed when an epoch starts: from a generator of its own, so that the global
        # random streams stay the step's alone (a checkpoint stores them, and a resumed run starts no epoch it has finished)
        loader_gen = torch.Generator()
        loader_gen.manual_seed(self.seed)
        self.loader = torch.utils.data.DataLoader(self.train_data, B, shuffle=False, sampler=self.sampler, drop_last=True,
                                                  num_workers=args.num_workers, pin_memory=dev.type == "cuda",
                                                  collate_fn=self.collate, generator=loader_gen)
        if cs:
            self.pipe = ip.CityscapesInputPipeline(dev, opt.height, opt.width, train_data.raw_hw, frame_idxs=tuple(train_ids))
        else:
            self.pipe = ip.DeviceInputPipeline(None, opt.height, opt.width, dev, frame_idxs=tuple(train_ids))
        # validation (trainer.py:128-134, 204-212, 225-227): frame 0 and the lookup frames, no augmentation, the last batch
        # kept; under --train_cs the raw test frames of --cs_eval_path, listed by the same split folder
        self.predictor = DepthPredictor(model, opt, amp_dtype=trainer.amp_dtype)
        val_ids = [0] + self.predictor.lookup_ids
        if val_data is None and cs:
            val_data = datasets.CityscapesEvalDataset(args.cs_eval_path, datasets.readlines(fpath.format("test")), val_ids)
        elif val_data is None:
            val_data = datasets.KITTIRAWDataset(args.data_path, datasets.readlines(fpath.format("test")), val_ids, ext)
        self.val_data = val_data
        self.val_loader = torch.utils.data.DataLoader(self.val_data, B, shuffle=False, drop_last=False,
                                                      num_workers=args.num_workers, pin_memory=dev.type == "cuda",
                                                      collate_fn=self.val_collate, generator=loader_gen)
        if cs:
            self.val_pipe = ip.CityscapesEvalPipeline(dev, opt.height, opt.width, val_data.raw_hw, frame_idxs=tuple(val_ids))
        else:
            self.val_pipe = ip.DeviceInputPipeline(None, opt.height, opt.width, dev, frame_idxs=tuple(val_ids), is_train=False)
        self.val_store = ValidationStore(val_ids, len(val_data), dev, self.val_pipe.unit, self.val_pipe.backend) \
            if val_store else None
        self._gt = None
        self.log = RunLog(dev, capacity=max(256, 2 * args.log_every), names=LOG_NAMES)
        self.rows, self.validations = [], []          # everything logged / validated so far, for the caller
        self.pending_save = None
        self._gen = torch.Generator()
        self._stop, self._end = False, None

    def start(self):
        """Capture, load, seed -- in that order.  The step is captured on the inputs of step 0 with restore_state=True (the
        warm-up consumes no training step); --load_weights_folder is loaded in place afterwards, so the graph stays valid.
        With --resume the run goes on at the checkpoint's step with the checkpoint's random streams; without, a loaded run
        starts at step 0 of a fresh schedule with the optimizer it loaded (trainer.py:313-317), and the random streams
        start from the seed here, whatever the warm-up consumed."""
        a, opt, tr, eng = self.args, self.opt, self.trainer, self.engine
        if not a.no_capture and not a.eval:
            if eng.stream is None:
                raise SystemExit("the captured step needs a HIP device: pass --no_capture for eager steps on the host")
            if opt.load_weights_folder and getattr(opt, "dc", False):
                # Stage 2 freezes the decoder, whose weights are the checkpoint's and not this process's draws: the captured
                # step reads images of the frozen weights built before the capture, so they are in place before it.  The
                # load after the capture then finds them equal and puts everything the warm-up was restored to back again.
                tr.load_model(opt.load_weights_folder, eng, transfer=opt.ktf)
            eng.capture(self.first_batch(), restore_state=True)
        if opt.load_weights_folder:
            tr.load_model(opt.load_weights_folder, eng, transfer=opt.ktf)
            if not a.resume:
                tr.step, tr.epoch = 0, 0
                eng.scheduler.last_epoch = 0
        if not (a.resume and opt.load_weights_folder):
            seed_all(self.seed)

    # -- data ----------------------------------------------------------------------------------------------------------
    def batch(self, frames, global_step):
        """Packed frames of one step -> the step's inputs; the augmentation is a function of (seed, global_step)."""
        self._gen.manual_seed(step_seed(self.seed, global_step))
        if self.cityscapes:
            triplets, cameras = frames
            return self.pipe(triplets, cameras, generator=self._gen)
        return self.pipe(frames, generator=self._gen)

    def first_batch(self):
        """The inputs of step 0, for `TrainEngine.capture` (the warm-up consumes no training step: restore_state=True)."""
        idx = item_indices(0, len(self.train_data), self.opt.batch_size)
        return self.batch(self.collate([self.train_data[i] for i in idx]), 0)

    def loader_val_batches(self):
        """The validation batches from disk: loader workers, decode, upload, the evaluation pipeline."""
        for frames in self.val_loader:
            yield self.val_pipe(*frames) if self.cityscapes else self.val_pipe(frames)

    def val_batches(self):
        """The first validation of a run reads the loader's batches and keeps what the predictor reads of them on the
        device; every later one reads that store (valstore.py)."""
        store = self.val_store
        if store is None:
            yield from self.loader_val_batches()
        elif store.complete:
            yield from store.batches(self.opt.batch_size)
        else:
            store.begin()
            for data in self.loader_val_batches():
                store.add(data)
                yield data
            store.finish()

    def ground_truth(self):
        if self._gt is None:
            from .evaluate import DeviceGroundTruth
            a = self.args
            if a.eval_split == "cityscapes":               # single files, for their combined size (trainer.py:760-780)
                self._gt = DeviceGroundTruth.from_folder(os.path.join(a.splits_dir, a.eval_split, "gt_depths"),
                                                         len(self.val_data), self.device)
            else:
                self._gt = DeviceGroundTruth(load_gt_depths(a.splits_dir, a.eval_split), self.device)
        return self._gt

    # -- what follows a step ---------------------------------------------------------------------------------------------
    def validate(self, hard_test_mono=False):
        """-> the student's 7 metrics, and the teacher's unless it is frozen.  The loop never calls model.eval(): the
        predictor reads the weights and running statistics through its own tables (`refresh`)."""
        self.predictor.refresh()
        return self.trainer.val(self.val_batches(), self.ground_truth(), self.args.eval_split, hard_test_mono=hard_test_mono,
                                predictor=self.predictor, metrics="device")

    def check_log(self):
        """ONE read of the log: print the interval's line, keep the rows, raise `NonFiniteRun` if the run has gone bad."""
        rows = self.log.read()
        self.rows.extend(rows)
        if rows.first_bad_step >= 0:
            bad = [r for r in rows if r["step"] == rows.first_bad_step]
            cols = []
            if bad:
                cols = [k for k in self.log.names if bad[0][k] is not None and not np.isfinite(bad[0][k])]
                cols += ["grad_nonfinite"] if bad[0]["grad_nonfinite"] else []
            raise NonFiniteRun(rows.first_bad_step, cols)
        if rows:
            r = rows[-1]
            self.out("step {:7d}  loss {:.5f}  lr {:.3g}  bins {:.3f} .. {:.3f}  |grad| {:.4g} (max {:.3g})".format(
                r["step"], r["loss"], r["lr"], r["min_depth_bin"], r["max_depth_bin"], r["grad_l2"], r["grad_max_abs"]))
        return rows

    def save(self, s):
        if self.pending_save is not None:
            self.pending_save.wait()
        folder = os.path.join(self.args.ckpt_dir, f"{self.opt.name}_s{s}")
        self.pending_save = self.trainer.save_model_debug(folder, self.engine, blocking=False)
        return folder

    def after_step(self, s, losses):
        tr, eng, a = self.trainer, self.engine, self.args
        scalars = {k: losses[k] for k in self.log.names if k in losses}
        scalars.update(min_depth_bin=tr.depth_bin_tracker.min_depth, max_depth_bin=tr.depth_bin_tracker.max_depth)
        flat = eng.flat.flat if eng.flat is not None else None
        if getattr(eng, "flat_adam", False):
            scalars["lr"] = eng.adam_state[1]
        self.log.append(s, scalars, flat, eng.flat.numel if flat is not None else None, eng.grad_scale)
        validate, save = step_events(s, a.validate_every, a.validate_from, a.save_until, a.early_val_step, a.saveoff)
        if s % a.log_every == 0 or validate or save:
            self.check_log()
        if validate:
            metrics = self.validate()
            self.validations.append((s, metrics))
            if tr.freeze_tp:
                self.out(f"step {s} validate {metrics}")
            else:
                self.out(f"step {s} validate {metrics[0]}\nvalidate teacher {metrics[1]}")
        if save:
            self.out(f"step {s}: saving {self.save(s)}")

    # -- the loop (trainer.py:296-418) -----------------------------------------------------------------------------------
    def run_epoch(self, first=0):
        """One epoch from its batch `first` on, then the schedule's step (trainer.py:418)."""
        tr, eng = self.trainer, self.engine
        self.sampler.start = first * self.opt.batch_size
        try:
            for frames in self.loader:
                g = tr.step
                if self._end is not None and g >= self._end:
                    self._stop = True
                    return
                _, losses = eng.step(self.batch(frames, g))
                self.after_step(tr.step - 1, losses)
        finally:
            self.sampler.start = 0
        eng.scheduler_step()
        tr.epoch = getattr(tr, "epoch", 0) + 1

    def train(self):
        """From `trainer.step` (0, or a resumed run's position) to the end of --num_epochs or --max_steps."""
        tr, a = self.trainer, self.args
        self._end = None if a.max_steps is None else tr.step + a.max_steps
        self._stop = False
        epoch, first = resume_position(tr.step, self.steps_in_epoch)
        tr.epoch = epoch
        t0, s0 = time.time(), tr.step
        try:
            while epoch < self.opt.num_epochs and not self._stop and (self._end is None or tr.step < self._end):
                self.out(f"epoch {epoch + 1}/{self.opt.num_epochs}")
                self.run_epoch(first)
                epoch, first = epoch + 1, 0
            self.check_log()
        finally:
            if self.pending_save is not None:
                self.pending_save.wait()
                self.pending_save = None
        self.out(f"{tr.step - s0} steps in {time.time() - t0:.1f} s")
        return self.rows


def main(argv=None):
    from . import networks, options
    from .dist import TrainEngine
    from .trainer import Trainer
    args, rest = _run_parser().parse_known_args(argv)
    opt = options.MonodepthOptions().parse(rest)
    follow_train_cs(args, opt)
    check_served(opt, args)
    options.apply_train_cs(opt)                # before the model is built (options.apply_train_cs)
    if args.resume and not opt.load_weights_folder:
        raise SystemExit("--resume goes on from a checkpoint: give --load_weights_folder")
    if args.eval and not opt.load_weights_folder:
        raise SystemExit("--eval scores a checkpoint: give --load_weights_folder")
    seed = seed_all(args.pytorch_random_seed)
    print("[ Using Seed : ", seed, " ]")
    device = torch.device(args.device if args.device else ("cuda" if torch.cuda.is_available() else "cpu"))
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    model = networks.RepDepth(opt)
    if opt.dc:
        # Stage 2: the decoder adapters are built and the rest of the decoders frozen BEFORE the engine exists, so the
        # engine's trainable set and its fresh Adam are the Stage-2 ones; their initialisation draws follow the model's own
        # (trainer.py:154).  `Run.start` loads --load_weights_folder afterwards: a Stage-1 checkpoint has no adapter keys
        # and leaves them as drawn, a Stage-2 checkpoint of this loop restores them and their Adam moments.
        model.dc_ft_init()
    model.to(device).train()
    trainer = Trainer(opt, model, device, amp_dtype=None if args.fp32 else torch.bfloat16)
    engine = TrainEngine(trainer, bf16_params=not args.fp32)
    global last_run
    run = last_run = Run(trainer, engine, args, seed=seed)
    print("Training model named:\n  ", opt.name, "\nTraining is using:\n  ", device)
    print(f"Using split:\n   {args.split}\nThere are {len(run.train_data)} training items and {len(run.val_data)} "
          "validation items\n")
    run.start()
    print(engine.describe_schedule())
    if args.eval:
        metrics, metrics_mono = run.validate(hard_test_mono=True)
        print("validate after load ", metrics, metrics_mono)
        run.validations.append((trainer.step, (metrics, metrics_mono)))
        return 0
    run.train()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
