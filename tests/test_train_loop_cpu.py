"""The plan of a training run (ppeadepth/train.py) as pure functions: which steps validate, save and step the schedule
(reference trainer.py:366-418, hand-written tables), which items a step trains on and where a resumed run starts, and what
the entry point refuses."""
import pytest
import torch


def test_event_plan_matches_the_reference_loop():
    from ppeadepth import train
    # 6 steps per epoch, 2 epochs: `step == early` validates only; `step != 0 and step % 4 == 0` validates and saves; the
    # schedule steps after the last step of each epoch
    plan = train.event_plan(6, 2, validate_every=4, validate_from=0, save_until=0, early_val_step=2)
    assert plan == {"validate": [2, 4, 8], "save": [4, 8], "schedule": [5, 11]}
    # validate_from is exclusive (step > validate_from), save_until inclusive (step >= save_until), early validation off
    plan = train.event_plan(5, 3, validate_every=3, validate_from=3, save_until=9, early_val_step=0)
    assert plan == {"validate": [6, 9, 12], "save": [9, 12], "schedule": [4, 9, 14]}
    # --saveoff, a resumed run cut short by --max_steps, and an early step that is a regular one too (validated once)
    plan = train.event_plan(5, 3, validate_every=3, early_val_step=6, saveoff=True, start_step=4, max_steps=6)
    assert plan == {"validate": [6, 9], "save": [], "schedule": [4, 9]}
    assert train.step_events(0, 1) == (False, False)                   # never at step 0
    assert train.step_events(250, 1000) == (True, False) and train.step_events(1000, 1000) == (True, True)


def test_data_position_is_a_function_of_seed_and_global_step():
    from ppeadepth import train
    assert train.steps_per_epoch(13, 2) == 6                            # drop_last
    assert train.item_indices(0, 13, 2) == [0, 1] and train.item_indices(5, 13, 2) == [10, 11]
    assert train.item_indices(7, 13, 2) == [2, 3]                       # no shuffling: epoch 1 reads the same lines
    assert train.resume_position(9, 6) == (1, 3) and train.resume_position(12, 6) == (2, 0)
    seeds = {train.step_seed(s, g) for s in (1, 2, 3) for g in range(100)}
    assert len(seeds) == 300 and train.step_seed(1, 5) == (1 << 32) + 5
    a, b = torch.Generator().manual_seed(train.step_seed(1, 5)), torch.Generator().manual_seed(train.step_seed(1, 5))
    assert torch.equal(torch.rand(4, generator=a), torch.rand(4, generator=b))
    sampler = train._EpochSampler(12)
    assert list(sampler) == list(range(12))
    sampler.start = 3 * 2                                              # resumed after 3 batches of 2
    assert list(sampler) == list(range(6, 12)) and len(sampler) == 6
    loader = torch.utils.data.DataLoader(list(range(13)), 2, sampler=sampler, drop_last=True)
    assert [b.tolist() for b in loader] == [train.item_indices(g, 13, 2) for g in (3, 4, 5)]


@pytest.mark.parametrize("flag", ["--train_cs", "--ddad", "--freeze_teacher_and_pose", "--freeze_pose"])
def test_unserved_flags_are_refused_by_name(flag, tmp_path):
    from ppeadepth import train
    with pytest.raises(SystemExit) as e:
        train.main(["--data_path", str(tmp_path), flag])
    assert flag in str(e.value)


def test_several_ranks_are_refused(monkeypatch, tmp_path):
    from ppeadepth import train
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        train.main(["--data_path", str(tmp_path)])
    assert "WORLD_SIZE=2" in str(e.value) and "one rank" in str(e.value)


def test_missing_ground_truth_names_the_export_command(tmp_path):
    from ppeadepth import train
    with pytest.raises(FileNotFoundError) as e:
        train.load_gt_depths(str(tmp_path), "eigen")
    assert "python -m ppeadepth.export_gt_depth" in str(e.value) and "gt_depths.npz" in str(e.value)


def test_run_flags_keep_the_reference_defaults():
    from ppeadepth import train
    a = train._run_parser().parse_args(["--data_path", "x"])
    assert (a.split, a.eval_split, a.num_workers, a.validate_every, a.validate_from, a.save_until) == \
        ("eigen_zhou", "eigen", 12, 1000, 0, 0)
    assert not (a.png or a.saveoff or a.eval or a.fp32 or a.no_capture or a.resume) and a.pytorch_random_seed is None
    assert (a.splits_dir, a.ckpt_dir, a.log_every, a.early_val_step, a.max_steps) == ("splits", "./ckpt", 50, 250, None)
    assert train.seed_all(None) == 1 and train.seed_all(7) == 7
