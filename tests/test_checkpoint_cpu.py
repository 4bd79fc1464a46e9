"""Checkpoints on the host (no GPU, no forward pass; gradients are synthetic): the file layer (ppeadepth/checkpoint.py:
the reference's model.pth / track.pth / adam.pth, trainer.py:1290-1381), the engine's translation between its own layout
and the reference's parameter order (TrainEngine.checkpoint_state / load_checkpoint_state, on the CPU engine: torch's
optimizer holds the state, the index remapping is the one the flat layout uses), and the reference-named glue
(Trainer.save_model_debug / load_model).  The full-size files are ~1.6 GB: no test writes them -- disk round trips use a
stand-in module with a handful of parameters, engine tests work on the in-memory documents.

tests/golden/checkpoint_spec.npz (tools/gen_checkpoint_golden.py) holds names, shapes and dtypes of the files the
REFERENCE's own `save_model_debug` wrote; state_spec.npz / fullft_spec.npz are the reference's state_dict orders."""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN


def _spec():
    return np.load(os.path.join(GOLDEN, "checkpoint_spec.npz"))


# ---- parameter order: what index i of adam.pth means ----------------------------------------------------------
@pytest.mark.parametrize("size,fullft", [("b", False), ("l", False), ("b", True)])
def test_parameter_order_and_trainable_flags_are_the_references(size, fullft):
    from ppeadepth import networks, options
    model = networks.RepDepth(options.default_options(rep_size=size, fullft_reb=fullft))
    mine = [n for n, _ in model.named_parameters()]
    z = np.load(os.path.join(GOLDEN, "fullft_spec.npz" if fullft else "state_spec.npz"))
    names = [str(n) for n in z[f"{size}:names"]]
    flags = dict(zip(names, (bool(t) for t in z[f"{size}:trainable"])))
    assert [n for n in names if n in set(mine)] == mine           # the reference's key order, restricted to parameters
    assert {n: p.requires_grad for n, p in model.named_parameters()} == {n: flags[n] for n in mine}
    if size == "b" and not fullft:
        # the names and shapes behind every index of the adam.pth that the reference's save_model_debug wrote
        spec = _spec()
        trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        assert [n for n, _ in trainable] == [str(n) for n in spec["adam_names"]]
        assert [";".join(str(d) for d in p.shape) for _, p in trainable] == [str(s) for s in spec["adam_shapes"]]


# ---- the full model on the CPU engine ------------------------------------------------------------------------------
def _engine(seed=0, **flags):
    from ppeadepth import networks, options
    from ppeadepth.dist import TrainEngine
    from ppeadepth.trainer import Trainer
    opt = options.default_options(height=64, width=96, batch_size=2, **flags)
    torch.manual_seed(seed)
    model = networks.RepDepth(opt)
    if flags.get("dc"):
        model.dc_ft_init()
    tr = Trainer(opt, model, "cpu")
    return model, tr, TrainEngine(tr)


@pytest.fixture(scope="module")
def stepped():
    """(model, trainer, engine, stock Adam over the reference's list on a twin model): two steps on the same synthetic
    gradients, given by parameter NAME.  Python's hash of a str is salted per process, so the seeds come from a table."""
    model, tr, eng = _engine()
    twin = type(model)(tr.opt)
    twin.load_state_dict(model.state_dict())
    stock = torch.optim.Adam([p for p in twin.parameters() if p.requires_grad], tr.opt.learning_rate)
    seeds = {n: i for i, (n, _) in enumerate(model.named_parameters())}
    for step in range(2):
        for m in (model, twin):
            for n, p in m.named_parameters():
                if p.requires_grad:
                    g = torch.Generator().manual_seed(seeds[n] * 7 + step)
                    p.grad = torch.randn(p.shape, generator=g) * 1e-2
        eng.optimizer.step()
        stock.step()
    return model, tr, eng, twin, stock


def test_stock_adam_document_loads_into_the_engine_bit_equal(stepped):
    """adam.pth written by stock torch.optim.Adam over `[p for p in model.parameters() if p.requires_grad]` -- what a
    reference checkpoint is -- loaded through load_checkpoint_state: every moment and the step counter by NAME."""
    model, tr, eng, twin, stock = stepped
    _, tr2, eng2 = _engine(seed=1)
    before = eng2.checkpoint_state()
    assert before.adam["state"] == {}                                      # no step taken: torch's own empty state
    track = {"height": 64, "width": 96, "min_depth_bin": torch.tensor(0.25), "max_depth_bin": torch.tensor(42.0)}
    keys = eng2.load_checkpoint_state((twin.state_dict(), track, stock.state_dict()))
    assert not keys.missing_keys and not keys.unexpected_keys
    names = {id(p): n for n, p in eng2.trainer._module().named_parameters()}
    mine = {names[id(p)]: eng2.optimizer.state[p] for p in eng2.opt_params}
    ref = {n: stock.state[p] for n, p in twin.named_parameters() if p.requires_grad}
    assert set(mine) == set(ref) and len(ref) == 1306
    for n, st in ref.items():
        assert torch.equal(mine[n]["exp_avg"], st["exp_avg"]) and torch.equal(mine[n]["exp_avg_sq"], st["exp_avg_sq"]), n
        assert float(mine[n]["step"]) == float(st["step"]) == 2.0
    for (n, a), (_, b) in zip(eng2.trainer._module().state_dict().items(), twin.state_dict().items()):
        assert torch.equal(a, b), n
    # a track.pth without the "ppea" key (a reference file): the tracker is loaded, nothing else is touched
    assert float(tr2.depth_bin_tracker.min_depth) == 0.25 and float(tr2.depth_bin_tracker.max_depth) == 42.0
    assert tr2.depth_bin_tracker.updated and tr2.step == 0


def test_engine_document_loads_into_stock_adam_bit_equal(stepped):
    model, tr, eng, twin, stock = stepped
    docs = eng.checkpoint_state()
    spec = _spec()
    group, entry = docs.adam["param_groups"][0], docs.adam["state"][0]
    assert sorted(group) == sorted(set(str(k) for k in spec["group_keys"]) | {"initial_lr"})      # StepLR adds initial_lr
    assert sorted(entry) == [str(k) for k in spec["state_keys"]]
    assert str(entry["step"].dtype) == str(spec["step_dtype"]) and list(entry["step"].shape) == list(spec["step_shape"])
    assert group["params"] == list(range(1306)) and sorted(docs.adam["state"]) == group["params"]
    fresh = type(model)(tr.opt)
    fresh.load_state_dict(docs.model)
    other = torch.optim.Adam([p for p in fresh.parameters() if p.requires_grad], 1e-4)
    other.load_state_dict(docs.adam)
    ref = {n: stock.state[p] for n, p in twin.named_parameters() if p.requires_grad}
    for n, p in fresh.named_parameters():
        if p.requires_grad:
            st = other.state[p]
            assert torch.equal(st["exp_avg"], ref[n]["exp_avg"]) and torch.equal(st["exp_avg_sq"], ref[n]["exp_avg_sq"]), n
            assert float(st["step"]) == 2.0
    # the two Adams were given the same gradients by name: the models agree bit for bit as well
    for (n, a), (_, b) in zip(docs.model.items(), twin.state_dict().items()):
        assert torch.equal(a, b), n


def test_unequal_step_counters_and_wrong_shapes_raise_before_anything_is_written(stepped):
    import copy
    model, tr, eng, twin, stock = stepped
    docs = eng.checkpoint_state()
    _, tr2, eng2 = _engine(seed=1)
    before = eng2.checkpoint_state()
    adam = copy.deepcopy(docs.adam)
    adam["state"][5]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="step"):
        eng2.load_checkpoint_state(docs._replace(adam=adam))
    adam = copy.deepcopy(docs.adam)
    adam["state"][7]["exp_avg"] = torch.zeros(3)
    with pytest.raises(ValueError, match="shape"):
        eng2.load_checkpoint_state(docs._replace(adam=adam))
    adam = copy.deepcopy(docs.adam)
    adam["param_groups"][0]["params"] = list(range(10))
    with pytest.raises(ValueError, match="parameters"):
        eng2.load_checkpoint_state(docs._replace(adam=adam))
    after = eng2.checkpoint_state()
    assert after.adam["state"] == {} and all(torch.equal(a, b) for a, b in zip(after.model.values(), before.model.values()))


def test_ppea_key_restores_step_schedule_and_random_streams(stepped):
    from ppeadepth import checkpoint, rng
    model, tr, eng, twin, stock = stepped
    tr.step, tr.epoch = 17, 3
    for _ in range(tr.opt.scheduler_step_size):
        eng.scheduler_step(lr_quirk=False)                   # the rate drops
    rng.set_mode("reference")
    random.seed(5)
    torch.manual_seed(5)
    try:
        docs = eng.checkpoint_state()
    finally:
        rng.set_mode("device")
    want = (random.random(), torch.rand(3))
    ppea = docs.track["ppea"]
    assert set(ppea) == set(checkpoint.PPEA_FIELDS) and ppea["version"] == checkpoint.FORMAT_VERSION
    assert ppea["world_size"] == 1 and ppea["bf16_params"] is False and ppea["device_rng"] is None
    assert ppea["lr"] == pytest.approx(1e-5) and ppea["step"] == 17 and ppea["epoch"] == 3
    _, tr2, eng2 = _engine(seed=1)
    try:
        eng2.load_checkpoint_state(docs)
        assert rng.get_mode() == "reference"
    finally:
        rng.set_mode("device")
    assert (random.random(), ) == want[:1] and torch.equal(torch.rand(3), want[1])
    assert tr2.step == 17 and tr2.epoch == 3
    assert eng2.optimizer.param_groups[0]["lr"] == pytest.approx(1e-5)
    assert eng2.scheduler.last_epoch == eng.scheduler.last_epoch == tr.opt.scheduler_step_size
    assert eng2.scheduler.state_dict() == eng.scheduler.state_dict()


def test_stage1_document_hands_over_to_a_stage2_engine(stepped):
    """Stage 1 -> Stage 2 (--dc): the Stage-1 model document into a fresh model, dc_ft_init(), then the engine: it trains
    the Stage-2 set with a fresh Adam; the Stage-1 adam.pth does not fit that set and Trainer.load_model's rule applies."""
    from ppeadepth import networks, options
    from ppeadepth.dist import TrainEngine
    from ppeadepth.trainer import Trainer
    model, tr, eng, twin, stock = stepped
    docs = eng.checkpoint_state()
    opt = options.default_options(height=64, width=96, batch_size=2, dc=True)
    fresh = networks.RepDepth(opt)
    keys = fresh.load_state_dict(docs.model, strict=False)
    assert not keys.unexpected_keys and all(k.startswith(("depth.", "mono_depth.")) for k in keys.missing_keys) and keys.missing_keys
    fresh.dc_ft_init()
    tr2 = Trainer(opt, fresh, "cpu")
    eng2 = TrainEngine(tr2)
    stage2 = [n for n, p in fresh.named_parameters() if p.requires_grad]
    names = {id(p): n for n, p in fresh.named_parameters()}
    assert sorted(names[id(p)] for p in eng2.params) == sorted(stage2)
    assert any(".adapter." in n or "deconv_adpt" in n for n in stage2 if n.startswith("depth."))
    assert set(stage2) != {n for n, p in model.named_parameters() if p.requires_grad}
    d2 = eng2.checkpoint_state()
    assert d2.adam["state"] == {} and len(d2.adam["param_groups"][0]["params"]) == len(stage2)
    with pytest.raises(ValueError):
        eng2.load_checkpoint_state(docs)
    eng2.load_checkpoint_state(docs._replace(adam=None))                 # what Trainer.load_model falls back to
    assert eng2.checkpoint_state().adam["state"] == {}
    for k, v in docs.model.items():
        assert torch.equal(d2.model[k], v), k


# ---- the file layer and the glue, on a stand-in module --------------------------------------------------------------
class _StandIn(nn.Module):
    def __init__(self):
        super().__init__()
        self.frozen = nn.Conv2d(3, 4, 3)
        self.bn = nn.BatchNorm2d(4)
        self.head = nn.Linear(4, 2)
        self.late = nn.Linear(2, 2, bias=False)
        for p in self.frozen.parameters():
            p.requires_grad = False


def _standin(seed=0, **flags):
    from ppeadepth import options
    from ppeadepth.dist import TrainEngine
    from ppeadepth.trainer import Trainer
    opt = options.default_options(height=64, width=96, batch_size=2, **flags)
    torch.manual_seed(seed)
    model = _StandIn()
    tr = Trainer(opt, model, "cpu")
    eng = TrainEngine(tr)
    return model, tr, eng


def _step(eng, k=1):
    for i in range(k):
        for j, p in enumerate(eng.params):
            p.grad = torch.full_like(p, 0.01 * (i + j + 1))
        eng.optimizer.step()


def test_folder_round_trip_files_keys_and_resume(tmp_path):
    from ppeadepth import checkpoint
    model, tr, eng = _standin()
    _step(eng, 2)
    model.bn.running_mean.add_(0.5)
    model.bn.num_batches_tracked.add_(2)
    tr.depth_bin_tracker.load(0.3, 55.0)
    tr.step = 2
    folder = str(tmp_path / "weights_0")
    docs = tr.save_model_debug(folder, eng)
    spec = _spec()
    assert sorted(os.listdir(folder)) == [str(f) for f in spec["files"]] == ["adam.pth", "model.pth", "track.pth"]
    got = checkpoint.read_folder(folder)
    assert list(got.model) == list(model.state_dict()) and all(v.dtype == model.state_dict()[k].dtype for k, v in got.model.items())
    assert set(got.track) == set(str(k) for k in spec["track_keys"]) | {"ppea"}
    assert set(got.track["ppea"]) == set(checkpoint.PPEA_FIELDS)
    assert float(got.track["min_depth_bin"]) == pytest.approx(0.3) and got.track["height"] == 64 and got.track["width"] == 96
    # index i of adam.pth is the i-th trainable parameter in registration order, whatever order the engine keeps
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert [id(p) for p in eng.params] != [id(p) for p in trainable]
    for i, p in enumerate(trainable):
        assert torch.equal(got.adam["state"][i]["exp_avg"], eng.optimizer.state[p]["exp_avg"])
    # resume in a fresh engine: every document equal to the saved one
    model2, tr2, eng2 = _standin(seed=1)
    keys = tr2.load_model(folder, eng2)
    assert not keys.missing_keys and not keys.unexpected_keys and tr2.step == 2
    again = eng2.checkpoint_state()
    for k in docs.model:
        assert torch.equal(again.model[k], docs.model[k]), k
    for i in docs.adam["state"]:
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(again.adam["state"][i][k], docs.adam["state"][i][k])
    assert float(tr2.depth_bin_tracker.max_depth) == 55.0
    # and the next step is the same step
    _step(eng, 1)
    _step(eng2, 1)
    assert all(torch.equal(a, b) for a, b in zip(eng.checkpoint_state().model.values(), eng2.checkpoint_state().model.values()))
    # Trainer.load_model without an engine: model and tracker only
    model3, tr3, _ = _standin(seed=2)
    tr3.load_model(folder)
    assert torch.equal(model3.bn.running_mean, docs.model["bn.running_mean"]) and float(tr3.depth_bin_tracker.min_depth) == pytest.approx(0.3)
    assert tr3.step == 0


def test_strict_false_missing_adam_shape_mismatch_and_transfer(tmp_path, capsys):
    from ppeadepth import checkpoint
    model, tr, eng = _standin()
    _step(eng, 1)
    tr.depth_bin_tracker.load(0.3, 55.0)
    docs = eng.checkpoint_state()
    # strict=False: a missing and an extra key
    sd = dict(docs.model)
    del sd["late.weight"]
    sd["gone.weight"] = torch.zeros(2)
    folder = str(tmp_path / "a")
    checkpoint.write_folder(folder, sd, docs.track, docs.adam)
    model2, tr2, eng2 = _standin(seed=1)
    late = model2.late.weight.detach().clone()
    keys = tr2.load_model(folder, eng2)
    assert keys.missing_keys == ["late.weight"] and keys.unexpected_keys == ["gone.weight"]
    assert torch.equal(model2.late.weight, late) and torch.equal(model2.head.weight, docs.model["head.weight"])
    # no adam.pth: a fresh optimizer, with the reference's message
    os.remove(os.path.join(folder, "adam.pth"))
    model3, tr3, eng3 = _standin(seed=1)
    tr3.load_model(folder, eng3)
    assert "Cannot find Adam weights so Adam is randomly initialized" in capsys.readouterr().out
    assert eng3.checkpoint_state().adam["state"] == {} and float(tr3.depth_bin_tracker.max_depth) == 55.0
    # a shape mismatch in adam.pth raises ValueError in the engine; Trainer.load_model goes on with a fresh optimizer
    bad = {"state": {i: dict(st) for i, st in docs.adam["state"].items()}, "param_groups": docs.adam["param_groups"]}
    bad["state"][0]["exp_avg_sq"] = torch.zeros(5, 5)
    folder_b = str(tmp_path / "b")
    checkpoint.write_folder(folder_b, docs.model, docs.track, bad)
    model4, tr4, eng4 = _standin(seed=1)
    with pytest.raises(ValueError):
        eng4.load_checkpoint_state(checkpoint.read_folder(folder_b))
    tr4.load_model(folder_b, eng4)
    assert "Can't load Adam - using random" in capsys.readouterr().out
    assert eng4.checkpoint_state().adam["state"] == {} and torch.equal(model4.head.weight, docs.model["head.weight"])
    # transfer (--ktf): model.pth only -- neither tracker nor optimizer nor step
    model5, tr5, eng5 = _standin(seed=1)
    _step(eng5, 1)
    mom = eng5.checkpoint_state().adam["state"][0]["exp_avg"]
    got = checkpoint.read_folder(folder_b, transfer=True)
    assert got.track is None and got.adam is None
    tr5.load_model(folder_b, eng5, transfer=True)
    assert torch.equal(model5.head.weight, docs.model["head.weight"])
    assert float(tr5.depth_bin_tracker.max_depth) == 10.0 and not tr5.depth_bin_tracker.updated
    assert torch.equal(eng5.checkpoint_state().adam["state"][0]["exp_avg"], mom)


def test_reference_track_file_without_ppea_key_loads(tmp_path):
    from ppeadepth import checkpoint
    model, tr, eng = _standin()
    _step(eng, 1)
    docs = eng.checkpoint_state()
    track = {k: v for k, v in docs.track.items() if k != "ppea"}
    track["min_depth_bin"], track["max_depth_bin"] = torch.tensor(0.7), torch.tensor(33.0)
    folder = str(tmp_path / "ref")
    checkpoint.write_folder(folder, docs.model, track, docs.adam)
    model2, tr2, eng2 = _standin(seed=1)
    tr2.step = 9
    tr2.load_model(folder, eng2)
    assert float(tr2.depth_bin_tracker.min_depth) == pytest.approx(0.7) and tr2.depth_bin_tracker.updated and tr2.step == 9
    assert torch.equal(eng2.checkpoint_state().adam["state"][1]["exp_avg"], docs.adam["state"][1]["exp_avg"])


@pytest.mark.parametrize("flag", ["notadabins", "freeze_teacher_and_pose"])
def test_depth_bins_are_absent_when_they_are_not_tracked(flag):
    model, tr, eng = _standin(**{flag: True})
    track = eng.checkpoint_state().track
    assert "min_depth_bin" not in track and "max_depth_bin" not in track and {"height", "width", "ppea"} <= set(track)
    # and a document without them leaves the tracker alone
    tr.depth_bin_tracker.load(0.4, 44.0)
    tr.depth_bin_tracker.updated = False
    eng.load_checkpoint_state(eng.checkpoint_state()._replace(track={"height": 64, "width": 96}))
    assert float(tr.depth_bin_tracker.max_depth) == 44.0 and not tr.depth_bin_tracker.updated


def test_options_have_the_references_checkpoint_flags():
    from ppeadepth import options
    opt = options.MonodepthOptions().parse([])
    assert opt.load_weights_folder is None and opt.ktf is False and opt.name == "test"
    opt = options.MonodepthOptions().parse(["--load_weights_folder", "~/w", "--ktf", "--name", "run"])
    assert (opt.load_weights_folder, opt.ktf, opt.name) == ("~/w", True, "run")
