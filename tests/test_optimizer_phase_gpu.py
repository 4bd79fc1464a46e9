"""The optimizer phase of `TrainEngine.step` against an independent Adam, step by step (B = 2, 64 x 96, a fixed batch, four
steps, `scheduler_step()` -- StepLR with step size 1 -- between steps 2 and 3).

Shadow reference.  Before every step P, M, V (the whole flat buffers) are cloned; after it the step's gradients are read from
`eng.flat.flat` and oracle/ref_ops.py::adam_step (float64, evaluated on the device with torch's float64 operators to keep the
test quick) is applied to the clones with the HOST's step count and `eng.optimizer.param_groups[0]["lr"]` -- never with
`eng.adam_state`.  P, M, V after the step are held, element by element, to the bounds derived in tests/test_adam_cpu.py (the
ones tests/test_adam_gpu.py holds the bare kernel to).  After the learning-rate drop this fails unless `sync_lr` reached the
device scalar, eager and replayed; a captured step that kept t or lr as constants fails at its second replay.

On the flat path the reference takes b1, b2, eps at the fp32 values the kernel is handed.  On the non-flat arm
(`fused_adam=False`: torch's own foreach Adam) it takes the doubles of `param_groups`: torch rounds b2 and 1 - b2 to fp32
separately (each within u, which the v bound's 5u + second-order margin of 6u still covers), parameters and exp_avg /
exp_avg_sq are compared, gradients come from `named_grads()`.

Asserted along the way: the layout (`.data` of every trainable parameter a view into P at its offset -- into W16 for a bf16
working copy, its master into P), zero padding between the tensors in P, M, V, W16 == bfloat16(P[:n_lo]) bit for bit,
`eng.params` == the model's requires_grad parameters (each once), `export_state_dict()`, the state after
`capture(restore_state=True)`, and the set of trainable tensors that received NO gradient: `FlatGrads` zero-fills them where
the reference's torch.optim.Adam (trainer.py:142, zero_grad() at :349) skips them, which is the same thing only while such a
tensor's moments stay zero -- so the set must be the same at every step, on the hook path and on the gather path, and those
tensors' P, M, V must never change a bit.
"""
import random

import pytest
import torch

from oracle import synth
from test_adam_cpu import HYPER, check_step
from test_e2e_gpu import _build

pytestmark = pytest.mark.gpu

B, H, W = 2, 64, 96
LR = 1e-4

CASES = {
    "fp32_eager": dict(bf16=False),
    "bf16_eager": dict(bf16=True),
    "bf16_graph_restored": dict(bf16=True, graph="restore"),
    "bf16_graph_after_warmup": dict(bf16=True, graph="warm"),
    "fp32_torch_adam": dict(bf16=False, fused_adam=False),
    "bf16_fullft": dict(bf16=True, flags=dict(fullft_reb=True)),
    "fp32_dc": dict(bf16=False, build=dict(dc=True), intrinsics="cityscapes"),
    "fp32_two_past_frames": dict(bf16=False, build=dict(conditioned=True), flags=dict(num_matching_frames=2),
                                 frame_ids=(0, -1, 1, -2)),
}


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _engine(device, bf16, fused_adam=None, build=None, flags=None, intrinsics="kitti", frame_ids=None, **_):
    from ppeadepth import rng
    from ppeadepth.dist import TrainEngine
    opt, model, tr = _build(device, B, H, W, use_checkpoint=True, amp=torch.bfloat16 if bf16 else None,
                            scheduler_step_size=1, **(build or {}), **(flags or {}))
    rng.set_mode("device")
    eng = TrainEngine(tr, lr=LR, bf16_params=bf16, fused_adam=fused_adam)
    if frame_ids is not None:
        inputs = synth.make_rendered_inputs(B, H, W, frame_ids=frame_ids)
    else:
        inputs = synth.make_inputs(B, H, W, smooth=True, intrinsics=intrinsics)
    return model, eng, {k: v.to(device) for k, v in inputs.items()}


def _assert_layout(eng, model):
    """Views, offsets, padding and the bf16 working copy of the flat layout."""
    fl = eng.flat
    trainable = {id(p): n for n, p in model.named_parameters() if p.requires_grad}
    assert len(eng.params) == len(trainable) == len({id(p) for p in eng.params})
    assert {id(p) for p in eng.params} == set(trainable)
    assert len(eng.opt_params) == len(eng.params) == len(fl.offsets) == len(fl.views)
    pad = torch.ones(fl.numel, dtype=torch.bool, device=eng.P.device)
    n_lo_t = len(eng._lo)
    for i, (p, t, off, gv) in enumerate(zip(eng.params, eng.opt_params, fl.offsets, fl.views)):
        n = t.numel()
        assert off % 128 == 0 and off + n <= fl.numel
        assert t.dtype == torch.float32 and t.data_ptr() == eng.P.data_ptr() + 4 * off and t.is_contiguous(), trainable[id(p)]
        assert gv.data_ptr() == fl.flat.data_ptr() + 4 * off and gv.shape == t.shape
        if i < n_lo_t:
            assert p is eng._lo[i] and eng.masters[id(p)] is t and t is eng._hi[i]
            assert p.dtype == torch.bfloat16 and p.data_ptr() == eng.W16.data_ptr() + 2 * off and p.shape == t.shape
            assert off + n <= eng.n_lo
        else:
            assert p is t and off >= eng.n_lo
        pad[off:off + n] = False
    for name, buf in (("P", eng.P), ("M", eng.M), ("V", eng.V), ("G", fl.flat)):
        assert not bool(buf[pad].any()), f"padding of {name} is not zero"
    if eng.n_lo:
        assert eng.W16.numel() == eng.n_lo
        assert torch.equal(_bits(eng.W16), _bits(eng.P[:eng.n_lo].bfloat16()))
    else:
        assert n_lo_t == 0
    return pad


def _no_grad_set_from_hooks(eng):
    """Indices (into eng.params) of the tensors whose post-accumulate hook did not fire in the last backward; a range that
    holds one cannot have been launched from a hook."""
    fl = eng.flat
    none = [i for i in range(len(eng.params)) if i not in fl._fired]
    for (a, cnt, _, from_hook), k in zip(fl.last_plan, range(len(fl._ranges))):
        assert fl._ranges[k] == (a, a + cnt)
        if any(a <= i < a + cnt for i in none):
            assert not from_hook
    return none


def _element_mask(eng, indices):
    mask = torch.zeros(eng.flat.numel, dtype=torch.bool, device=eng.P.device)
    for i in indices:
        mask[eng.flat.offsets[i]:eng.flat.offsets[i] + eng.opt_params[i].numel()] = True
    return mask


def _flat_step(eng, inputs, t, what):
    """One step with the shadow reference over the whole flat buffer -> largest error / bound of p, m, v."""
    p0, m0, v0 = eng.P.clone(), eng.M.clone(), eng.V.clone()
    lr = eng.optimizer.param_groups[0]["lr"]
    random.seed(0)
    _, losses = eng.step(inputs if eng.graph is not None else dict(inputs))
    torch.cuda.synchronize()
    assert float(losses["loss"]) == float(losses["loss"])
    assert bool((eng.flat.flat != 0).any()), "the step produced no gradient"
    return check_step((eng.P, eng.M, eng.V), p0, eng.flat.flat, m0, v0, t, lr, gscale=eng.grad_scale, what=f"{what} t={t}")


@pytest.mark.parametrize("case", [c for c in CASES if c != "fp32_torch_adam"])
def test_flat_optimizer_phase_against_float64_adam(device, case):
    from ppeadepth import rng
    cfg = CASES[case]
    model, eng, inputs = _engine(device, **cfg)
    graph = cfg.get("graph")
    try:
        assert eng.flat_adam and eng.flat.hooked and eng.grad_scale == 1.0
        group = eng.optimizer.param_groups[0]
        assert (HYPER["b1"], HYPER["b2"], HYPER["eps"]) == tuple(float(torch.tensor(x, dtype=torch.float32))
                                                                 for x in (*group["betas"], group["eps"]))
        n_keys = list(model.state_dict().keys())
        pad = _assert_layout(eng, model)
        p_start = eng.P.clone()
        t = 0
        if graph:
            random.seed(0)
            eng.capture(inputs, warmup=1 if graph == "restore" else 2, restore_state=graph == "restore")
            if graph == "restore":          # the first replay is step 1 from the weights of before the warm-up
                assert torch.equal(_bits(eng.P), _bits(p_start)) and not bool(eng.M.any()) and not bool(eng.V.any())
                assert float(eng.adam_state[0]) == 0.0
            else:
                t = 2                       # the warm-up's steps count: the first replay is step 3
                assert not torch.equal(_bits(eng.P), _bits(p_start)) and bool(eng.M.any())
            assert float(eng.adam_state[1]) == float(torch.tensor(LR, dtype=torch.float32))
            none_sets = [_no_grad_set_from_hooks(eng)]          # a replay runs no hook: the captured backward's set
        else:
            none_sets = []
        worst = [0.0, 0.0, 0.0]
        for k in range(4):
            if k == 2:
                eng.scheduler_step(lr_quirk=False)
                assert abs(group["lr"] - 0.1 * LR) < 1e-12
            t += 1
            worst = [max(a, b) for a, b in zip(worst, _flat_step(eng, inputs, t, case))]
            if not graph:
                none_sets.append(_no_grad_set_from_hooks(eng))
            _assert_layout(eng, model)
        if not graph:
            # the gather path (hooks off): `p.grad is None` as FlatGrads.gather finds it
            seen, real = [], eng.flat.gather
            eng.flat.gather = lambda sources: (seen.append([i for i, p in enumerate(sources) if p.grad is None]), real(sources))[1]
            eng.flat.hooked = False
            try:
                t += 1
                worst = [max(a, b) for a, b in zip(worst, _flat_step(eng, inputs, t, case + " gather"))]
            finally:
                eng.flat.hooked, eng.flat.gather = True, real
            assert len(seen) == 1
            none_sets.append(seen[0])
            _assert_layout(eng, model)
        # tensors without a gradient: the same set at every step, and never touched
        names = {id(p): n for n, p in model.named_parameters()}
        assert all(s == none_sets[0] for s in none_sets), [[names[id(eng.params[i])] for i in s] for s in none_sets]
        mask = _element_mask(eng, none_sets[0])
        assert torch.equal(_bits(eng.P)[mask], _bits(p_start)[mask])
        assert not bool(eng.M[mask].any()) and not bool(eng.V[mask].any()) and not bool(eng.flat.flat[mask].any())
        moved = (_bits(eng.P) != _bits(p_start)) & ~pad
        print(f"{case}: {len(eng.params)} trainable tensors, {eng.flat.numel} flat elements (n_lo {eng.n_lo}), "
              f"{len(none_sets[0])} tensors / {int(mask.sum())} elements without a gradient at every one of {len(none_sets)} "
              f"steps, {int(moved.sum())} elements moved; largest error / bound  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
        # checkpoint format: the masters' values under the model's full key set
        sd = eng.export_state_dict()
        assert list(sd.keys()) == n_keys and all(v.dtype != torch.bfloat16 for v in sd.values())
        for p, tt, off in zip(eng.params, eng.opt_params, eng.flat.offsets):
            v = sd[names[id(p)]]
            assert v.dtype == torch.float32 and v.shape == p.shape
            assert torch.equal(_bits(v.reshape(-1)), _bits(eng.P[off:off + tt.numel()])), names[id(p)]
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")


def test_torch_adam_arm_against_float64_adam(device):
    """`fused_adam=False`: no flat buffers, torch's foreach Adam steps the parameters.  Same reference, same bounds; a
    parameter without gradient is skipped (no optimizer state, value untouched), and it is the same set at every step."""
    from ppeadepth import rng
    model, eng, inputs = _engine(device, **CASES["fp32_torch_adam"])
    try:
        assert not eng.flat_adam and eng.flat is None and eng.masters is None
        names = {id(p): n for n, p in model.named_parameters()}
        assert {id(p) for p in eng.params} == {id(p) for p in model.parameters() if p.requires_grad}
        assert len(eng.params) == len({id(p) for p in eng.params})
        group = eng.optimizer.param_groups[0]
        hyper = dict(b1=group["betas"][0], b2=group["betas"][1], eps=group["eps"])
        cat = lambda ts: torch.cat([x.detach().reshape(-1) for x in ts])
        state = eng.optimizer.state
        start = [p.detach().clone() for p in eng.params]
        worst, none_sets = [0.0, 0.0, 0.0], []
        for k in range(4):
            if k == 2:
                eng.scheduler_step(lr_quirk=False)
                assert abs(group["lr"] - 0.1 * LR) < 1e-12
            t, lr = k + 1, group["lr"]
            before = [(p.detach().clone(), state[p]["exp_avg"].clone() if p in state else torch.zeros_like(p),
                       state[p]["exp_avg_sq"].clone() if p in state else torch.zeros_like(p)) for p in eng.params]
            random.seed(0)
            eng.step(dict(inputs))
            torch.cuda.synchronize()
            grads = eng.named_grads()
            has = [i for i, p in enumerate(eng.params) if grads[names[id(p)]] is not None]
            none_sets.append([i for i in range(len(eng.params)) if i not in set(has)])
            assert 2 * len(has) > len(eng.params)
            ps = [eng.params[i] for i in has]
            assert all(int(state[p]["step"]) == t for p in ps)
            got = (cat(ps), cat([state[p]["exp_avg"] for p in ps]), cat([state[p]["exp_avg_sq"] for p in ps]))
            p0, m0, v0 = (cat([before[i][j] for i in has]) for j in range(3))
            g = cat([grads[names[id(p)]].float() for p in ps])
            r = check_step(got, p0, g, m0, v0, t, lr, what=f"torch adam t={t}", hyper=hyper)
            worst = [max(a, b) for a, b in zip(worst, r)]
        assert all(s == none_sets[0] for s in none_sets), [[names[id(eng.params[i])] for i in s] for s in none_sets]
        for i in none_sets[0]:
            assert eng.params[i] not in state and torch.equal(eng.params[i].detach(), start[i]), names[id(eng.params[i])]
        print(f"fp32_torch_adam: {len(eng.params)} trainable tensors, {len(none_sets[0])} without a gradient at every step; "
              f"largest error / bound  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")
