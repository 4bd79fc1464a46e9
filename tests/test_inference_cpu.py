"""DepthPredictor(device="cpu"): the folding algebra of the inference path, checked without a GPU.

The eval-mode MODULE path of this package cannot run on the CPU (its depthwise and cost-volume operators are HIP only), so
the unfused comparator here is the CPU oracle's eval path (`oracle.ref_model.RefRepDepth.predict_val`, BatchNorm as
F.batch_norm on the running statistics, two depthwise convs + two BatchNorms per large-kernel pair) next to the
reference's own outputs in tests/golden/infer.npz.  The predictor against the module path itself is a GPU test.
"""
import copy
import types

import pytest
import torch

from conftest import rel_err

from oracle import ref_model, synth

TOL = 1e-3          # the project's fp32 tolerance
FOLD_TOL = 1e-4     # fp32 torch on the same machine; only the affine maps and the merged k x k + 5 x 5 sum re-associate
B, H, W = 2, 64, 96


def _build(rep_size="b", dc=False, train=True):
    from ppeadepth import networks, options
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, rep_size=rep_size, dc=dc)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    if dc:
        model.dc_ft_init()
    synth.fill_state_dict(model, conditioned=True)
    model.train(train)
    return model, opt


def _predict(p, data):
    r = p.predict(data[("color", 0, 0)], data[("color", -1, 0)], data[("K", 2)], data[("inv_K", 2)], 0.1, 10.0)
    return r, p.predict_mono(data[("color", 0, 0)])


def _oracle(model, opt, data, rep_size, dc):
    from ppeadepth.layers import disp_to_depth
    ropt = types.SimpleNamespace(rep_size=rep_size, g_blk=1.0, g_ffn=1.0, use_checkpoint=False, height=H, width=W,
                                 batch_size=B, num_depth_bins=96, min_depth=0.1, max_depth=100.0, dc=dc)
    ref = ref_model.RefRepDepth({k: v.clone() for k, v in model.state_dict().items()}, ropt)
    ref.training = False
    d, m = ref.predict_val({k: v.clone() for k, v in data.items()}, 0.1, 10.0, opt.max_depth)
    return d, m, disp_to_depth


@pytest.mark.parametrize("rep_size,dc", [("b", False), ("l", False), ("b", True)])
def test_cpu_predictor_matches_unfused_eval_oracle(rep_size, dc):
    """Measured (rel_err of the scaled disparities, predictor vs oracle): b 3.5e-07 / 3.3e-07, l 3.2e-07 / 3.1e-07,
    dc 3.0e-07 / 2.1e-07 (multi-frame / teacher)."""
    from ppeadepth.inference import DepthPredictor
    model, opt = _build(rep_size, dc)
    data = synth.make_rendered_inputs(B, H, W)
    r, dm = _predict(DepthPredictor(model, opt, device="cpu"), data)
    d_ref, m_ref, disp_to_depth = _oracle(model, opt, data, rep_size, dc)
    e_multi = rel_err(disp_to_depth(r["disp"], 1e-3, 80)[0][:, 0], d_ref)
    e_mono = rel_err(disp_to_depth(dm, 1e-3, opt.max_depth)[0][:, 0], m_ref)
    print(f"predictor vs unfused oracle [{rep_size}, dc={dc}]: multi {e_multi:.3e} mono {e_mono:.3e}")
    assert e_multi <= FOLD_TOL and e_mono <= FOLD_TOL, (e_multi, e_mono)


def test_cpu_predictor_matches_reference_golden(golden):
    """Measured: disp 3.4e-07, disp_mono 3.2e-07, pose 7.0e-10, lowest_cost equal everywhere."""
    from ppeadepth.inference import DepthPredictor
    g = golden("infer")
    model, opt = _build()
    data = synth.make_rendered_inputs(B, H, W)
    r, dm = _predict(DepthPredictor(model, opt, device="cpu"), data)
    errs = {"disp": rel_err(r["disp"], g["64x96:disp"]), "disp_mono": rel_err(dm, g["64x96:disp_mono"]),
            "pose": rel_err(r["pose"], g["64x96:pose"])}
    print("predictor vs reference golden:", errs)
    assert all(e <= TOL for e in errs.values()), errs
    assert torch.equal(r["lowest_cost"], g["64x96:lowest_cost"])


def test_cpu_predictor_builds_and_runs_with_trans_and_input_adapters():
    """--trans / --input / --mono_trans / --mono_input: the CPU oracle has no such branches, so the numerical comparison with
    the module path is the GPU test; here the schedule runs, uses the adapters (the output moves when one changes) and
    raises nothing."""
    from ppeadepth import networks, options
    from ppeadepth.inference import DepthPredictor
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, trans=True, input=True,
                                  mono_trans=True, mono_input=True)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model, conditioned=True)
    model.train()
    data = synth.make_rendered_inputs(B, H, W)
    p = DepthPredictor(model, opt, device="cpu")
    r0, m0 = _predict(p, data)
    assert bool(torch.isfinite(r0["disp"]).all()) and bool(torch.isfinite(m0).all())
    with torch.no_grad():
        model.mono_encoder.input_adapter.D_fc2.bias.add_(0.05)
        model.encoder.replk.trans_adpt[1].D_fc2.bias.add_(0.05)
    r1, m1 = _predict(p, data)
    assert not torch.equal(m0, m1) and not torch.equal(r0["disp"], r1["disp"])


def test_predictor_is_non_destructive():
    from ppeadepth.inference import DepthPredictor
    model, opt = _build()
    before = copy.deepcopy(model.state_dict())
    names = [n for n, _ in model.named_modules()]
    modes = [m.training for m in model.modules()]
    data = synth.make_rendered_inputs(B, H, W)
    p = DepthPredictor(model, opt, device="cpu")
    p.refresh()
    _predict(p, data)
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    assert all(torch.equal(after[k], before[k]) for k in before)
    assert [n for n, _ in model.named_modules()] == names
    assert [m.training for m in model.modules()] == modes and model.training
    assert [p_.requires_grad for p_ in model.parameters()] == [p_.requires_grad for p_ in _build()[0].parameters()]


def test_refresh_follows_running_statistics_and_adapter_weights():
    from ppeadepth.inference import DepthPredictor
    model, opt = _build()
    data = synth.make_rendered_inputs(B, H, W)
    p = DepthPredictor(model, opt, device="cpu")
    r0, m0 = _predict(p, data)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for enc in (model.encoder.replk, model.mono_encoder):
            blk = enc.stages[1].blocks[0]
            blk.pw2.bn.running_mean.add_(0.05 * torch.randn(blk.pw2.bn.running_mean.shape, generator=g))
            blk.large_kernel.small_conv.bn.running_var.mul_(1.3)
            blk.adapter.D_fc2.weight.add_(0.02 * torch.randn(blk.adapter.D_fc2.weight.shape, generator=g))
        bn = model.pose_encoder.encoder.layer2[0].bn1
        bn.running_mean.add_(0.05 * torch.randn(bn.running_mean.shape, generator=g))
    r_stale, m_stale = _predict(p, data)
    fresh = DepthPredictor(model, opt, device="cpu")
    r_new, m_new = _predict(fresh, data)
    # the adapters are read from the live model, the tables are not: a stale predictor is neither the old nor the new one
    assert not torch.equal(m_stale, m_new) and not torch.equal(r_stale["disp"], r_new["disp"])
    assert not torch.equal(m0, m_new) and not torch.equal(r0["pose"], r_new["pose"])
    p.refresh()
    r_ref, m_ref = _predict(p, data)
    assert torch.equal(m_ref, m_new)
    for k in ("disp", "lowest_cost", "pose"):
        assert torch.equal(r_ref[k], r_new[k]), k


def test_unsupported_configuration_raises_at_construction():
    from ppeadepth import _abi
    from ppeadepth.inference import DepthPredictor
    model, opt = _build()
    with pytest.raises(_abi.PpeaKernelError):
        DepthPredictor(model, types.SimpleNamespace(num_matching_frames=2), device="cpu")
    model.mono_encoder.structural_reparam()
    with pytest.raises(_abi.PpeaKernelError):
        DepthPredictor(model, opt, device="cpu")


def test_inference_entry_point_is_declared_and_bound():
    import os
    import re
    from conftest import ROOT
    from ppeadepth import _abi
    header = open(os.path.join(ROOT, "include", "ppea_depth.h")).read()
    assert re.search(r"\bint ppea_pwconv_infer_bf16\(", header)
    assert "ppea_pwconv_infer_bf16" in _abi.SIGNATURES
    assert len(_abi.SIGNATURES["ppea_pwconv_infer_bf16"]) == 17
    assert hasattr(_abi.lib, "ppea_pwconv_infer_bf16")
