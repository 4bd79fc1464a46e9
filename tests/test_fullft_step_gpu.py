"""Full fine-tuning (--fullft_reb) as a served configuration of the training step: the reference's unmodified process_batch
+ backward (tests/golden/e2e_small_fullft.npz, tools/gen_fullft_golden.py), the kernel census of the fp32 and bf16 steps,
bitwise purity of the captured step, and the adapter-only step left alone."""
import random
import re

import pytest
import torch

from oracle import synth
from test_e2e_gpu import TOL_F32, _assert_within, _build, _check, _engine_step, _errors, _run

pytestmark = pytest.mark.gpu

# library convolution / GEMM kernels (tests/test_e2e_gpu.py::test_bf16_step_launches_no_library_convolution_or_gemm)
LIB = re.compile(r"Cijk_|igemm|ck::|ck_tile|miopen|MIOpen|naive_conv|SubTensorOp|gemm_|Gemm|wmma|batched_transpose")


def test_fullft_e2e_small_vs_reference_golden(device, golden):
    """The direct fp32 step with every backbone weight trainable: losses, outputs, BN statistics and the gradients of 57
    parameters -- large-kernel / 5x5 / 3x3 depthwise filters, 1x1 weights of every stage, the stem and two transitions in
    both encoders -- against the reference, at the tolerance of the adapter-only goldens."""
    g, model, tr, inputs, outputs, losses, stride = _run("e2e_small_fullft", golden, device, fullft_reb=True)
    _check(g, model, tr, inputs, outputs, losses, stride)
    params = dict(model.named_parameters())
    keys = [k[9:] for k in g if k.startswith("grad_sum:")]
    assert len(keys) == 57 and sum("conv.weight" in k for k in keys) >= 50
    for k in keys:
        assert params[k].requires_grad and params[k].grad is not None, k


@pytest.mark.parametrize("graph", [False, True])
def test_fullft_engine_step_fp32_vs_reference_golden(device, golden, graph):
    """TrainEngine.step in fp32, eager and replayed from a hipGraph, at the tolerance of
    test_engine_step_fp32_vs_reference_golden."""
    res = _engine_step("e2e_small_fullft", golden, device, bf16=False, graph=graph, fullft_reb=True)
    _assert_within(_errors(*res), TOL_F32)


def _census(device, bf16):
    """One TrainEngine step (after a warm-up step) at B = 1, 64 x 96 with fullft_reb under the profiler, with every
    ops.call / ops.try_call and every PointwiseConv fallback logged.  -> (kernel name -> launches, entry-point log,
    fallbacks [(module, x shape, x dtype)], served trainable 1x1 forward calls, shapes of the 1x1 conv weights whose
    gradient ops.pwgrad_into wrote)."""
    from torch.profiler import ProfilerActivity, profile
    from ppeadepth import ops, rng
    from ppeadepth.dist import TrainEngine
    from ppeadepth.networks import replknet_adapter as rka
    B, H, W = 1, 64, 96
    opt, model, tr = _build(device, B, H, W, use_checkpoint=True, amp=torch.bfloat16 if bf16 else None, conditioned=True,
                            fullft_reb=True)
    rng.set_mode("device")
    eng = TrainEngine(tr, lr=1e-4, bf16_params=bf16)
    inputs = {k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W).items()}
    eng.step(dict(inputs))                                   # warm-up (lazy initialisations)
    torch.cuda.synchronize()
    calls, fallbacks, served, wgrads = [], [], [], []
    real = (ops.call, ops.try_call, ops.Conv2d.forward, ops.pwconv_trainable, ops.pwgrad_into)

    def call(name, *a):
        calls.append(name)
        return real[0](name, *a)

    def try_call(name, *a):
        calls.append(name)
        return real[1](name, *a)

    def conv_forward(self, x):
        if isinstance(self, rka.PointwiseConv):
            fallbacks.append((self, tuple(x.shape), x.dtype))
        return real[2](self, x)

    def pw_trainable(x, w, want_sums=False):
        r = real[3](x, w, want_sums=want_sums)
        if r is not None:
            served.append(tuple(w.shape))
        return r

    def pwgrad_into(p, q, w_shape, *a, **k):
        if len(w_shape) == 4 and tuple(w_shape[2:]) == (1, 1):          # a 1x1 CONV weight (the adapters' are Linear / 3x3)
            wgrads.append(tuple(w_shape))
        return real[4](p, q, w_shape, *a, **k)
    try:
        ops.call, ops.try_call, ops.Conv2d.forward, ops.pwconv_trainable, ops.pwgrad_into = (
            call, try_call, conv_forward, pw_trainable, pwgrad_into)
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            _, losses = eng.step(dict(inputs))
            torch.cuda.synchronize()
    finally:
        ops.call, ops.try_call, ops.Conv2d.forward, ops.pwconv_trainable, ops.pwgrad_into = real
    assert float(losses["loss"]) == float(losses["loss"])
    names = {}
    for ev in prof.events():
        if str(ev.device_type).endswith("CUDA") and ev.name:
            names[ev.name] = names.get(ev.name, 0) + 1
    assert len(names) > 20, "the profiler recorded no device kernels"
    hits = {n: c for n, c in names.items() if LIB.search(n)}
    others = {n: c for n, c in hits.items() if "Cijk_" not in n}
    assert not others, others
    assert sum(c for n, c in hits.items() if "Cijk_" in n) <= 16, hits          # pose algebra only
    return names, calls, fallbacks, served, wgrads


def _count(names, part):
    return sum(c for n, c in names.items() if part in n)


def test_fullft_bf16_step_census(device):
    """Every convolution and every weight gradient of the bf16 full-fine-tuning step is a gfx950 kernel of this build: no
    library convolution / GEMM (the pose algebra's tiny products excepted), the depthwise filter gradients come from
    dwconv_lk_bwd_filter_* and dwconv3x3_bwd_filter*, and no 1x1 conv whose shape ops.pwconv_trainable serves falls back to
    csrc/conv_f32.hip -- shown by the model walk itself: every PointwiseConv call that reached ops.Conv2d.forward is logged
    with its shape, and the conv_f32 launches are bounded by the logged generic-conv entry points (each launches at most two
    kernels: the weight gradient and its slab sum)."""
    names, calls, fallbacks, served, wgrads = _census(device, bf16=True)
    assert _count(names, "dwconv_lk_bwd_filter") >= 2 * 24 * 2, names     # 24 blocks per encoder pass, MFMA launch + sum
    assert _count(names, "dwconv3x3_bwd_filter") >= 2 * 5 * 2             # stem[1], stem[3], three transitions
    assert _count(names, "dwconv_wgrad_kernel") == 0                     # the fp32 filter-gradient kernel is not needed
    # The model walk.  What carries the claim is the per-call log: EVERY PointwiseConv call that left the GEMM path reaches
    # ops.Conv2d.forward and is logged with its shape, and none of them has a shape ops.pwconv_trainable serves.  2 encoders x
    # (24 blocks x 4 + stem[2] + 3 transitions) = 200 1x1 convs; at 64 x 96 stage 3 works on 2 x 3 maps (HW = 6, no
    # multiple of 8), so its 2 x 8 convs may fall back, nothing else.
    for mod, shape, dtype in fallbacks:
        Cout, Cin = mod.weight.shape[:2]
        assert dtype != torch.bfloat16 or Cin % 32 or Cout % 32 or (shape[2] * shape[3]) % 8, (shape, tuple(mod.weight.shape))
    assert len(fallbacks) <= 2 * 8, len(fallbacks)
    # ... and the other 184 got their WEIGHT gradient from the split-K reduce kernel: ops.pwgrad_into calls whose target is a
    # [Cout, Cin, 1, 1] conv weight (the adapters' own calls write Linear / 3x3 weights and are not counted; forward calls
    # under no_grad or recomputation would inflate `served`, which is therefore only a lower-bound sanity check)
    assert len(wgrads) == 2 * (24 * 4 + 4) - len(fallbacks), (len(wgrads), len(fallbacks))
    assert len(served) >= len(wgrads)
    # consistency of the two logs (not a bound on its own): every conv_f32 kernel was launched by a logged generic-conv entry
    # point, each of which launches at most two (the weight gradient and its slab sum)
    generic = sum(1 for n in calls if n.startswith("ppea_conv2d_"))
    assert _count(names, "conv_f32") <= 2 * generic, (_count(names, "conv_f32"), generic)


def test_fullft_fp32_step_census(device):
    """The fp32 full-fine-tuning step, as test_fp32_step_launches_no_library_convolution_or_gemm: library-free, dense
    convolutions on csrc/conv_f32.hip, the depthwise filter gradients on the fp32 kernels."""
    names, calls, fallbacks, served, wgrads = _census(device, bf16=False)
    assert _count(names, "conv_f32") > 300
    assert _count(names, "dwconv_wgrad_kernel") >= 2 * 24 * 2             # big + 5x5 filter per block
    assert _count(names, "dwconv3x3_bwd_filter") >= 2 * 5 * 2
    assert not served and not wgrads                                     # the bf16 GEMM is not part of the fp32 step


def test_fullft_bf16_step_is_a_pure_function_of_state_inputs_and_seeds(device):
    """B = 2, 64 x 96, bf16, every backbone weight trainable: eager step == captured replay == second replay from the
    restored state, bit for bit -- losses, disp and every gradient (pattern and state handling of
    test_step_is_a_pure_function_of_state_inputs_and_seeds).  The new reductions add their parts in a fixed order."""
    from ppeadepth import rng
    from ppeadepth.dist import TrainEngine
    B, H, W = 2, 64, 96
    opt, model, tr = _build(device, B, H, W, use_checkpoint=True, amp=torch.bfloat16, fullft_reb=True)
    eng = TrainEngine(tr, lr=1e-4, bf16_params=True)
    inputs = {k: v.to(device) for k, v in synth.make_inputs(B, H, W, smooth=True).items()}
    snap = eng.snapshot()

    def run():
        eng.restore(snap)
        torch.manual_seed(3)
        random.seed(3)
        outputs, losses = eng.step(dict(inputs) if eng.graph is None else inputs)
        torch.cuda.synchronize()
        res = {"loss:" + k: v.detach().clone() for k, v in losses.items()}
        res.update({"out:" + str(k): v.detach().clone() for k, v in outputs.items() if torch.is_tensor(v)})
        res.update({"grad:" + k: v.detach().clone() for k, v in eng.named_grads().items()})
        return res

    try:
        e1 = run()
        eng.restore(snap)
        torch.manual_seed(3)
        random.seed(3)
        eng.capture(inputs, warmup=1, restore_state=True)
        g1, g2 = run(), run()
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")
    grads = [k for k in e1 if k.startswith("grad:")]
    assert "out:('disp', 0)" in e1 and len(grads) > 1306            # the adapter-only step has 1 306 trainable tensors
    for k in ("grad:encoder.replk.stages.0.blocks.0.large_kernel.lkb_origin.conv.weight",
              "grad:mono_encoder.stem.1.conv.weight", "grad:encoder.replk.stages.2.blocks.7.pw1.conv.weight"):
        assert k in e1 and float(e1[k].float().abs().sum()) > 0.0, k
    for what, a in (("replay 1", g1), ("replay 2", g2)):
        diff = [k for k in e1 if not torch.equal(e1[k], a[k])]
        assert not diff, (what, len(diff), diff[:6])


def test_adapter_only_step_enters_no_full_fine_tuning_path(device):
    """fullft_reb=False: one bf16 engine step calls none of the new entry points and never ops.pwconv_trainable -- the
    frozen backbone's launch sequence is the parent's (asserted in-process by counting, not against a recorded fixture)."""
    from ppeadepth import ops, rng
    from ppeadepth.dist import TrainEngine
    B, H, W = 1, 64, 96
    opt, model, tr = _build(device, B, H, W, use_checkpoint=True, amp=torch.bfloat16, conditioned=True)
    rng.set_mode("device")
    eng = TrainEngine(tr, lr=1e-4, bf16_params=True)
    inputs = {k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W).items()}
    calls, entered = [], []
    real = (ops.call, ops.try_call, ops.pwconv_trainable, ops.dwconv_lk_bwd_filter)
    try:
        ops.call = lambda name, *a: (calls.append(name), real[0](name, *a))[1]
        ops.try_call = lambda name, *a: (calls.append(name), real[1](name, *a))[1]
        ops.pwconv_trainable = lambda *a, **k: (entered.append("pwconv_trainable"), real[2](*a, **k))[1]
        ops.dwconv_lk_bwd_filter = lambda *a, **k: (entered.append("dwconv_lk_bwd_filter"), real[3](*a, **k))[1]
        _, losses = eng.step(dict(inputs))
        torch.cuda.synchronize()
    finally:
        ops.call, ops.try_call, ops.pwconv_trainable, ops.dwconv_lk_bwd_filter = real
    assert float(losses["loss"]) == float(losses["loss"]) and len(calls) > 500
    assert not entered, entered[:4]
    assert not [n for n in calls if "bwd_filter" in n]
