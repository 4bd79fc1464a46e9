"""Several lookup frames end to end on the GPU (64 x 96, B = 2, RepLKNet-31B, conditioned synthetic weights as `_build` of
tests/test_inference_gpu.py): `--num_matching_frames 2` and `--use_future_frame` through the predictor, the eval-mode module
path, graph replay, one training step and `Trainer.val`."""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_err

from oracle import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3           # tests/test_inference_gpu.py
FOLD_TOL = 1e-4      # predictor vs the eval-mode module path, both fp32 (tests/test_inference_gpu.py)
TIE_CAP = 5e-3       # share of quarter-resolution pixels whose winning bin may differ (tests/test_inference_gpu.py)
RTOL = 1e-5          # device metrics vs host metrics (tests/test_eval_device_gpu.py)
H, W, B = 64, 96, 2
CONFIGS = {"two_past": dict(num_matching_frames=2), "future": dict(num_matching_frames=1, use_future_frame=True)}
EXPECTED_IDS = {"two_past": [-1, -2], "future": [1, -1]}
_cache = {}


def _setup(device, cfg):
    """(model in train mode, opt, rendered inputs on the device): built once per configuration, never modified."""
    if cfg not in _cache:
        from ppeadepth import networks, options
        opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, **CONFIGS[cfg])
        torch.manual_seed(0)
        model = networks.RepDepth(opt)
        synth.fill_state_dict(model, conditioned=True)
        model.to(device).train()
        assert model.matching_ids[1:] == EXPECTED_IDS[cfg]
        data = {k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W, frame_ids=(0, -1, 1, -2)).items()}
        _cache[cfg] = (model, opt, data)
    return _cache[cfg]


def _run(p, model, data):
    looks = torch.stack([data[("color", f, 0)] for f in model.matching_ids[1:]], 1)
    return p.predict(data[("color", 0, 0)], looks, data[("K", 2)], data[("inv_K", 2)], 0.1, 10.0)


def _module_path(model, opt, data, device, amp):
    """model.eval() + Trainer.predict_disps -> (scaled disparity, lowest_cost of the matching encoder, relative poses)."""
    from ppeadepth.trainer import Trainer
    tr = Trainer(opt, model, device, amp_dtype=amp)
    seen = []
    hook = model.encoder.register_forward_hook(lambda m, i, out: seen.append(out[1]))
    model.eval()
    try:
        d = dict(data)
        disp, _ = tr.predict_disps(d, mono=False)
    finally:
        model.train()
        hook.remove()
    return disp.float(), seen[0], torch.stack([d[("relative_pose", f)] for f in model.matching_ids[1:]], 1)


def _scaled(disp):
    from ppeadepth.layers import disp_to_depth
    return disp_to_depth(disp, 1e-3, 80)[0][:, 0]


def _differ(low, ref):
    return float(((low - ref).abs() > 1e-5 * ref.abs().clamp_min(1e-6)).float().mean())


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_fp32_predictor_matches_the_eval_mode_module_path(device, cfg):
    """Measured: two_past disp 7.0e-07 pose 8.1e-10, future disp 6.4e-07 pose 1.2e-07; lowest_cost equal at every pixel."""
    from ppeadepth.inference import DepthPredictor
    model, opt, data = _setup(device, cfg)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    modes = [m.training for m in model.modules()]
    r = _run(DepthPredictor(model, opt, amp_dtype=None), model, data)
    assert r["pose"].shape == (B, 2, 4, 4) and r["disp"].shape == (B, 1, H, W)
    d_mod, low_mod, pose_mod = _module_path(model, opt, data, device, None)
    e, e_pose, differ = rel_err(_scaled(r["disp"]), d_mod), rel_err(r["pose"], pose_mod), _differ(r["lowest_cost"], low_mod)
    print(f"[{cfg}] fp32 predictor vs module path: disp {e:.3e} pose {e_pose:.3e} lowest_cost differs at {differ:.4%}")
    assert e <= FOLD_TOL and e_pose <= FOLD_TOL
    assert differ <= TIE_CAP
    assert float((r["lowest_cost"] < 9.9).float().mean()) > 0.2               # the plane sweep found minima past bin 0 (1 / 0.1)
    assert model.training and [m.training for m in model.modules()] == modes
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_fp32_predictor_matches_the_cpu_predictor(device):
    from ppeadepth.inference import DepthPredictor
    model, opt, data = _setup(device, "two_past")
    r = _run(DepthPredictor(model, opt, amp_dtype=None), model, data)
    cpu_model = copy.deepcopy(model).cpu()
    rc = _run(DepthPredictor(cpu_model, opt, device="cpu"), cpu_model, {k: v.cpu() for k, v in data.items()})
    errs = {"disp": rel_err(r["disp"].cpu(), rc["disp"]), "pose": rel_err(r["pose"].cpu(), rc["pose"])}
    differ = _differ(r["lowest_cost"].cpu(), rc["lowest_cost"])
    print(f"fp32 GPU predictor vs CPU predictor: {errs} lowest_cost differs at {differ:.4%}")
    assert all(e <= TOL for e in errs.values()), errs
    assert differ <= TIE_CAP


def test_bf16_predictor_is_no_worse_than_the_bf16_module_path(device):
    """Error against the fp32 predictor <= 1.5 x the error of the bf16 eval-mode module path on the same inputs.
    Measured: predictor 6.4e-03, module path 6.2e-03."""
    from ppeadepth.inference import DepthPredictor
    model, opt, data = _setup(device, "two_past")
    ref = _scaled(_run(DepthPredictor(model, opt, amp_dtype=None), model, data)["disp"])
    e_p = rel_err(_scaled(_run(DepthPredictor(model, opt), model, data)["disp"]), ref)
    e_m = rel_err(_module_path(model, opt, data, device, torch.bfloat16)[0], ref)
    print(f"bf16 vs fp32 predictor: predictor {e_p:.3e} module path {e_m:.3e}")
    assert e_p <= 1.5 * e_m


def test_graph_replay_is_bitwise_the_eager_predictor(device):
    from ppeadepth.inference import DepthPredictor
    model, opt, _ = _setup(device, "two_past")
    batches = [{k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W, seed=s, frame_ids=(0, -1, -2)).items()}
               for s in (7, 8)]
    p = DepthPredictor(model, opt)
    eager = [_run(p, model, b) for b in batches]
    p.capture(B, mono=False)
    assert set(p._graphs) == {("multi", (B, 3, H, W))}
    replays = []
    g = p._graphs[("multi", (B, 3, H, W))]
    assert g["in"][1].shape == (B, 2, 3, H, W)
    inner = g["graph"]
    g["graph"] = type("Counted", (), {"replay": (lambda self: (replays.append(1), inner.replay())[1])})()
    replay = [_run(p, model, b) for b in batches] + [_run(p, model, batches[0])]
    for r, re_ in zip(replay, eager + eager[:1]):
        for k in ("disp", "lowest_cost", "pose"):
            assert torch.equal(r[k], re_[k]), k
    assert not torch.equal(eager[0]["disp"], eager[1]["disp"])
    assert len(replays) == 3


def test_one_eager_training_step_with_two_matching_frames(device, monkeypatch):
    from ppeadepth import ops, rng
    from ppeadepth.trainer import Trainer
    model, opt, data = _setup(device, "two_past")
    model = copy.deepcopy(model)                              # the step updates running statistics
    calls = []
    kernel = ops.cost_volume_multi

    def spy(cur, lookups, poses, *rest):
        out = kernel(cur, lookups, poses, *rest)
        calls.append(((cur.clone(), lookups.clone(), poses.clone()) + tuple(rest), out.clone()))
        return out

    monkeypatch.setattr(ops, "cost_volume_multi", spy)
    rng.set_mode("device")
    tr = Trainer(opt, model, device)
    _outputs, losses = tr.process_batch(dict(data), True)
    losses["loss"].backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses["loss"]))
    grad = model.encoder.replk.stages[0].blocks[0].adapter.D_fc1.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().sum()) > 0
    assert len(calls) == 1
    args, raw = calls[0]
    assert args[1].shape[:2] == (B, 2) and args[2].shape == (B, 2, 4, 4)
    assert torch.equal(kernel(*args), raw)
    assert float((raw != 0).float().mean()) > 0.05 or float(args[2].abs().sum()) == 0      # (both items may draw "no pose")


def test_val_on_a_split_with_frames_0_m1_m2(device, tmp_path):
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.trainer import Trainer
    model, opt, _ = _setup(device, "two_past")
    n = 4
    synth.make_eval_split(str(tmp_path), n=n, height=H, width=W, seed=7, split="eigen", frame_ids=(0, -1, -2))
    ds = synth.SynthEigenDataset(str(tmp_path), split="eigen", height=H, width=W, frame_idxs=(0, -1, -2))
    items, gt = [ds[i] for i in range(n)], ds.gt_depths()
    assert all(float(it[("color", -2, 0)].abs().sum()) > 0 for it in items)
    batches = [synth.collate(items[:2]), synth.collate(items[2:])]
    tr = Trainer(opt, model, device)
    p = DepthPredictor(model, opt, amp_dtype=None)
    host = tr.val([dict(b) for b in batches], gt, "eigen", predictor=p, metrics="host")
    dev = tr.val([dict(b) for b in batches], gt, "eigen", predictor=p, metrics="device")
    assert model.training
    for name, d, h in (("multi", dev[0], host[0]), ("mono", dev[1], host[1])):
        d, h = np.asarray(d, np.float64), np.asarray(h, np.float64)
        diff = np.abs(d - h)
        rel = float(np.max(np.where(diff == 0, 0.0, diff / np.abs(h))))
        print(f"{name}: device {d}\n    host {h}  rel {rel:.3e}")
        assert d.shape == (7,) and np.isfinite(d).all() and np.isfinite(h).all()
        assert rel <= RTOL
