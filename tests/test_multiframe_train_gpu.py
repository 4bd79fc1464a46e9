"""The training step with several matching frames on the GPU (B = 2, 64 x 96, RepLKNet-31B, conditioned synthetic weights,
rendered frames): the pose-chain kernel, the batched pose path against the sequential one, the fp32 engine step against
goldens written by the REFERENCE's unmodified process_batch + backward (tools/gen_golden_multiframe.py), whole-step graph
capture against the eager step bit for bit, and the library-GEMM census of the step."""
import copy
import random
import re

import pytest
import torch

from conftest import rel_err
from oracle import synth

pytestmark = pytest.mark.gpu

H, W, B = 64, 96, 2
FRAMES = (0, -1, 1, -2, -3)       # (the goldens were written with (0, -1, 1, -2): a frame does not depend on the others)
CONFIGS = {"single": dict(), "two_past": dict(num_matching_frames=2), "three_past": dict(num_matching_frames=3),
           "future": dict(num_matching_frames=1, use_future_frame=True)}
MATCHING = {"single": [0, -1], "two_past": [0, -1, -2], "three_past": [0, -1, -2, -3], "future": [0, 1, -1]}
GOLDEN = {"two_past": "e2e_mf_two_past", "future": "e2e_mf_future"}
CHAINS = [[0, -1], [0, 1, -1], [0, -1, -2], [0, -1, -2, -3], [0, 1, -1, -2, -3]]
FWD_TOL = 2e-5            # fp32 forward kernels against the float64 composite
_cache = {}


def _template(device, cfg, ckpt=False):
    """(model on the device in train mode, opt): built once per configuration and never stepped -- users deep-copy it.
    ckpt: `--use_checkpoint` (a checkpointed block updates its running statistics twice: not what the goldens hold)."""
    key = (cfg, ckpt)
    if key not in _cache:
        from ppeadepth import networks, options
        opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=ckpt, **CONFIGS[cfg])
        model = networks.RepDepth(opt)
        synth.fill_state_dict(model, conditioned=True)
        model.to(device).train()
        assert model.matching_ids == MATCHING[cfg]
        _cache[key] = (model, opt)
    return _cache[key]


def _batch(device, seed=7):
    key = ("batch", seed)
    if key not in _cache:
        _cache[key] = {k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W, seed=seed, frame_ids=FRAMES).items()}
    return _cache[key]


def _engine(device, cfg, bf16, ckpt=False):
    from ppeadepth.dist import TrainEngine
    from ppeadepth.trainer import Trainer
    model, opt = _template(device, cfg, ckpt)
    model = copy.deepcopy(model)
    tr = Trainer(opt, model, device, amp_dtype=torch.bfloat16 if bf16 else None)
    return model, tr, TrainEngine(tr, lr=1e-4, bf16_params=bf16)


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------
def _composite_f64(pairs, chain, keep):
    """transformation_from_parameters + matmul + mask in float64 on the host, frame by frame as repdepth.py:465-507."""
    from ppeadepth.layers import transformation_from_parameters
    rel = []
    for j, (p, invert, pred) in enumerate(chain):
        T = transformation_from_parameters(pairs[p][0].double().cpu(), pairs[p][1].double().cpu(), invert=invert)
        if pred >= 0:
            T = torch.matmul(T, rel[pred])
        rel.append(T * keep[:, j].double().cpu()[:, None, None])
    return torch.stack(rel, 1)


@pytest.mark.parametrize("ids", CHAINS, ids=lambda c: "_".join(str(i) for i in c))
def test_pose_chain_kernel_against_the_float64_composite(device, ids):
    """B = 3; axis-angles up to ~1 rad with one exactly 0, translations ~1; one (item, frame) absent in the middle of the
    chain: it and every frame chained behind it are exact zeros.  The pair tensors are views with the pose decoder's
    batch stride (12 floats) and are read in place; contiguous copies give the same bits, and so do two calls.  A frame
    without predecessor is `ops.pose_matrix` bit for bit (one shared device function).  Measured: 5.2e-8 .. 8.2e-8."""
    from ppeadepth import ops
    from ppeadepth.networks.repdepth import pose_pair_plan
    plan = pose_pair_plan([0, -1, 1], ids)
    used = sorted({f.pair for f in plan.frames})
    chain = [(used.index(f.pair), f.invert, f.pred) for f in plan.frames]
    n, F_ = 3, len(chain)
    g = torch.Generator().manual_seed(11 + F_)
    raw = [torch.randn(n, 12, generator=g) for _ in used]                        # the decoder's [B, 2 * 6] layout
    for r in raw:
        r[:, :3] *= 0.6                                                          # |axis-angle| up to ~1 rad
    raw[0][2, :3] = 0.0                                                          # angle exactly 0: the 1e-7 guard
    raw = [r.to(device) for r in raw]
    pairs = [(r.view(n, 2, 1, 6)[:, 0, :, :3], r.view(n, 2, 1, 6)[:, 0, :, 3:]) for r in raw]
    assert pairs[0][0].shape == (n, 1, 3) and not pairs[0][0].is_contiguous()
    has_succ = [j for j in range(F_) if any(c[2] == j for c in chain)]
    middle = [j for j in has_succ if chain[j][2] >= 0] or has_succ or [0]
    off = middle[0]
    keep = torch.ones(n, F_, device=device)
    keep[1, off] = 0.0
    T = ops.pose_chain(pairs, chain, keep)
    assert T.shape == (n, F_, 4, 4) and T.dtype == torch.float32
    ref = _composite_f64(pairs, chain, keep)
    err = rel_err(T.cpu(), ref)
    print(f"{ids}: pose_chain vs float64 composite {err:.3e}; absent (1, {off})")
    assert err <= FWD_TOL
    behind = {off}
    for j, c in enumerate(chain):
        if c[2] in behind:
            behind.add(j)
    for j in range(F_):
        assert (float(T[1, j].abs().max()) == 0.0) == (j in behind), j
    assert bool((T[0].abs().sum((1, 2)) > 0).all()) and bool((T[2].abs().sum((1, 2)) > 0).all())
    assert torch.equal(ops.pose_chain(pairs, chain, keep), T)
    assert torch.equal(ops.pose_chain([(a.contiguous(), t.contiguous()) for a, t in pairs], chain, keep), T)
    assert torch.equal(ops.pose_chain(pairs, chain)[0], T[0])                    # keep = None keeps all
    for j, (p, invert, pred) in enumerate(chain):
        if pred < 0:
            assert torch.equal(T[0, j], ops.pose_matrix(pairs[p][0], pairs[p][1], invert)[0]), j


# ---- 2. batched against sequential pose path ----------------------------------------------------------------------------
def _count_pose_passes(model):
    """Number of B-sized batches that go through the pose encoder (a groups = n call is n passes)."""
    n, fwd = [0], model.pose_encoder.forward

    def counted(x, groups=1, record=False):
        n[0] += groups
        return fwd(x, groups=groups, record=record)
    model.pose_encoder.forward = counted
    return n


@pytest.mark.parametrize("cfg,passes,grouped", [("future", 2, False), ("two_past", 3, False), ("three_past", 4, False),
                                                ("three_past", 4, True)])
def test_batched_pose_path_equals_the_sequential_one(device, cfg, passes, grouped):
    """From one state, in train mode: every pose output and relative pose to 1e-6 (the same passes run; only the chain's
    summation order may differ), every BatchNorm running statistic of the pose encoder to the bound of
    test_pose_pass_replay_equals_three_sequential_passes (2e-5) with the same number of tracked batches, and the number of
    pose-network passes that really ran: 2 for [0, 1, -1], 3 for [0, -1, -2] (the sequential path runs 4), 4 for [0, -1, -2, -3]
    (5), whose two new passes run one after another or as one groups = 2 batch (`NEW_PASSES_ONE_BATCH`).
    Measured: [0, 1, -1] 0 (equal), the others 1.2e-7."""
    from ppeadepth.networks import repdepth
    template, _ = _template(device, cfg)
    seq, bat = copy.deepcopy(template), copy.deepcopy(template)
    a_in, b_in = dict(_batch(device)), dict(_batch(device))
    n_seq, n_bat = _count_pose_passes(seq), _count_pose_passes(bat)
    out_seq = seq._predict_poses_sequential(a_in)
    old = repdepth.NEW_PASSES_ONE_BATCH
    repdepth.NEW_PASSES_ONE_BATCH = grouped
    try:
        out_bat = bat.predict_poses(b_in)
    finally:
        repdepth.NEW_PASSES_ONE_BATCH = old
    torch.cuda.synchronize()
    n_all = 2 + len(MATCHING[cfg]) - 1                         # what the reference runs: 2 gradient passes + one per lookup frame
    assert n_seq[0] == n_all and n_bat[0] == passes
    assert set(out_bat) == set(out_seq) and len(out_seq) == 6
    errs = {k: rel_err(out_bat[k].detach().cpu(), v.detach().cpu()) for k, v in out_seq.items()}
    for f in MATCHING[cfg][1:]:
        errs[("relative_pose", f)] = rel_err(b_in[("relative_pose", f)].cpu(), a_in[("relative_pose", f)].cpu())
        assert float(a_in[("relative_pose", f)].abs().sum()) > 0
    print(f"[{cfg}] batched vs sequential: {max(errs.values()):.3e}")
    assert all(e <= 1e-6 for e in errs.values()), errs
    sd_seq, sd_bat = seq.pose_encoder.state_dict(), bat.pose_encoder.state_dict()
    template_sd = template.pose_encoder.state_dict()
    for k, v in sd_seq.items():
        if "running" in k:
            assert rel_err(sd_bat[k].float().cpu(), v.float().cpu()) < 2e-5, k
        elif "num_batches_tracked" in k:
            assert int(sd_bat[k]) == int(v) == int(template_sd[k]) + n_all, k


# ---- 3. the fp32 engine step against the reference's goldens ------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["two_past", "future"])
@pytest.mark.parametrize("graph", [False, True])
def test_engine_step_fp32_vs_multiframe_reference_golden(device, golden, cfg, graph):
    """TrainEngine.step in fp32, eager and replayed, with the reference's random draws: the keys and bounds of
    test_engine_step_fp32_vs_reference_golden (losses, disp / depth / warps / cam_T_cam 1e-3; lowest_cost deviating at
    <= 0.5 % of the pixels; gradient checksums; running statistics, the pose encoder's included; depth-bin tracker) plus
    every lookup frame's relative pose.  Measured, eager = replayed: loss 3.0e-6 / 1.8e-6, out 7.7e-6, buf 1.4e-6, grad_abs
    6.5e-5, grad_head 2.3e-3, lowest_cost equal at every pixel."""
    from test_e2e_gpu import TOL_F32, _assert_within, _errors
    from ppeadepth import rng
    g = golden(GOLDEN[cfg])
    assert [int(v) for v in g["meta"]] == [B, H, W, 1, 1] and [int(v) for v in g["matching_ids"]] == MATCHING[cfg]
    rng.set_mode("reference")
    model, tr, eng = _engine(device, cfg, False)
    inputs = dict(_batch(device))
    try:
        if graph:
            eng.capture(inputs, warmup=1, restore_state=True)
        torch.manual_seed(1)
        random.seed(1)
        outputs, losses = eng.step(inputs)
        torch.cuda.synchronize()
        grads = {k: v.detach().float().clone() for k, v in eng.named_grads().items()}
        seen = eng.static_step_inputs if graph else inputs
        errs = _errors(g, model, tr, seen, outputs, losses, 1, grads)
        for f in MATCHING[cfg][1:]:
            errs[f"out:relative_pose|{f}"] = rel_err(seen[("relative_pose", f)].float().cpu(), g[f"in:relative_pose|{f}"])
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")
    worst = {p: max(v for k, v in errs.items() if k.split(":")[0] == p) for p in sorted({k.split(":")[0] for k in errs})}
    print(f"[{cfg}, graph={graph}] loss {float(losses['loss'].detach()):.6f} (golden {float(g['loss:loss']):.6f}); worst per group "
          + ", ".join(f"{p} {v:.2e}" for p, v in worst.items()))
    assert sum(k.startswith("out:relative_pose|") for k in errs) == 2
    assert "buf:pose_encoder.encoder.bn1.running_mean" in errs
    _assert_within(errs, TOL_F32)


# ---- 4. capture works and is exact ---------------------------------------------------------------------------------------
def _capture_equals_eager(device, cfg, bf16):
    """Protocol of test_step_is_a_pure_function_of_state_inputs_and_seeds: two different batches, each stepped eagerly from a
    restored snapshot and then replayed from the same snapshot, agree in every bit of every loss, output, gradient and
    post-step state tensor."""
    from ppeadepth import rng
    rng.set_mode("reference")
    model, tr, eng = _engine(device, cfg, bf16, ckpt=True)
    batches = [dict(_batch(device, 7)), dict(_batch(device, 8))]
    snap = eng.snapshot()

    def run(batch):
        eng.restore(snap)
        torch.manual_seed(3)
        random.seed(3)
        inputs = dict(batch)
        outputs, losses = eng.step(inputs)
        torch.cuda.synchronize()
        seen = inputs if eng.graph is None else eng.static_step_inputs
        res = {"loss:" + k: v.detach().clone() for k, v in losses.items()}
        res.update({"out:" + str(k): v.detach().clone() for k, v in outputs.items() if torch.is_tensor(v)})
        res.update({"in:" + str(k): v.detach().clone() for k, v in seen.items() if k[0] == "relative_pose"})
        res.update({"grad:" + k: v.detach().clone() for k, v in eng.named_grads().items()})
        res.update({"state:" + k: v.detach().clone() for k, v in model.state_dict().items()})
        return res

    try:
        eager = [run(b) for b in batches]
        eng.restore(snap)
        torch.manual_seed(3)
        random.seed(3)
        eng.capture(batches[0], warmup=1, restore_state=True)
        assert eng.graph is not None
        for f in MATCHING[cfg][1:]:
            assert ("relative_pose", f) in eng.static_step_inputs and ("color_aug", f, 0) in eng.static_inputs
        replay = [run(b) for b in batches] + [run(batches[0])]
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")
    assert len([k for k in eager[0] if k.startswith("in:")]) == len(MATCHING[cfg]) - 1
    assert len([k for k in eager[0] if k.startswith("grad:")]) > 1000
    for what, a, e in (("replay 1", replay[0], eager[0]), ("replay 2", replay[1], eager[1]), ("replay 3", replay[2], eager[0])):
        diff = [k for k in e if not torch.equal(e[k], a[k])]
        assert not diff, (what, len(diff), diff[:6])
    # the graph reads its inputs: the two batches give different losses
    assert float(eager[0]["loss:loss"]) != float(eager[1]["loss:loss"])
    assert all(bool(torch.isfinite(e["loss:loss"])) for e in eager)


@pytest.mark.parametrize("cfg", ["two_past", "future"])
@pytest.mark.parametrize("bf16", [False, True])
def test_captured_multiframe_step_is_bitwise_the_eager_step(device, cfg, bf16):
    _capture_equals_eager(device, cfg, bf16)


def test_captured_single_frame_step_is_still_bitwise_the_eager_step(device):
    _capture_equals_eager(device, "single", True)


# ---- 5. library GEMM census -----------------------------------------------------------------------------------------------
LIBRARY = re.compile(r"Cijk_|igemm|ck::|ck_tile|miopen|MIOpen|naive_conv|SubTensorOp|gemm_|Gemm|wmma|batched_transpose")


def _library_census(device, cfg):
    """One eager fp32 engine step under the profiler, as test_fp32_step_launches_no_library_convolution_or_gemm does it
    -> (library GEMM launches, other library kernel names, number of distinct device kernels, pose_chain launches)."""
    from torch.profiler import ProfilerActivity, profile
    from ppeadepth import rng
    rng.set_mode("device")
    _model, _tr, eng = _engine(device, cfg, False, ckpt=True)
    eng.step(dict(_batch(device)))                            # warm-up (lazy initialisations)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        _, losses = eng.step(dict(_batch(device)))
        torch.cuda.synchronize()
    assert bool(torch.isfinite(losses["loss"]))
    names = {}
    for ev in prof.events():
        if str(ev.device_type).endswith("CUDA") and ev.name:
            names[ev.name] = names.get(ev.name, 0) + 1
    hits = {n: c for n, c in names.items() if LIBRARY.search(n)}
    return (sum(c for n, c in hits.items() if "Cijk_" in n), {n: c for n, c in hits.items() if "Cijk_" not in n}, len(names),
            sum(c for n, c in names.items() if "pose_chain" in n))


def test_two_frame_step_launches_no_more_library_gemms_than_the_single_frame_step(device):
    """The pose chain is one HIP launch: the F = 2 step keeps the F = 1 step's census of tiny pose-algebra products
    (K @ T, 4x4), and neither step launches a library convolution."""
    gemms2, others2, kernels2, chain2 = _library_census(device, "two_past")
    gemms1, others1, kernels1, chain1 = _library_census(device, "single")
    print(f"library GEMMs: [0,-1,-2] {gemms2}, [0,-1] {gemms1}; distinct device kernels {kernels2} / {kernels1}")
    assert kernels1 > 20 and kernels2 > 20, "the profiler recorded no device kernels"
    assert not others1 and not others2, (others1, others2)
    assert gemms2 <= gemms1
    assert chain1 == 1 and chain2 == 1
