"""GPU parity of the pose network's kernels at their edge shapes, and of the trunk in isolation, against plain PyTorch on
the CPU in fp64 evaluated on the operands the kernels see (oracle/pose_inputs.py; tests/test_pose_trunk_cpu.py proves
those inputs and references fit).  A: conv_image.hip through ops.conv2d_nhwc with the 6- / 3-channel weights the
product passes.  B: nhwc_bn.hip through ops.nhwc_bn_act.  C: nhwc_pool.hip through ops.maxpool3x3s2.  D: ResnetEncoder +
PoseDecoder against RefRepDepth.pose_net, fp32 (every tensor to 1e-3) and the bf16 step's arithmetic."""
import contextlib
import functools

import pytest
import torch

from conftest import rel_err
from oracle import pose_inputs as PI

pytestmark = pytest.mark.gpu

BWD_TOL = 2e-4                   # tests/test_kernels_gpu.py: fp32 gradients
CL = torch.channels_last


def _ops():
    from ppeadepth import ops
    return ops


# ---- A. image-fed convolution, forward and weight gradient ---------------------------------------------------------------
@pytest.mark.parametrize("case", PI.IMAGE_CONV_CASES, ids=[PI.case_id(c) for c in PI.IMAGE_CONV_CASES])
def test_image_conv_forward_and_weight_gradient(device, case):
    """conv_image_kernel / image_pack_kernel / conv_image_wgrad_kernel / image_wgrad_reduce_kernel with Cin = 6 and 3 (the
    pack gate `ci < Cin`, the reduce into [Cout][Cin][K][K]), ragged tiles, Cout = 72, plans with one and with two trips
    of the patch loop.  y: one bf16 rounding after fp32 accumulation, element-wise; dw into an fp32 parameter: fp32
    accumulation of exact products (BWD_TOL); into a bf16 parameter: one more rounding (2^-7 of the tensor's max)."""
    from ppeadepth import _abi
    ops = _ops()
    K, Cout, nhw, nchw, wdt = case
    img, w, go = PI.image_conv_case(K, Cout, nhw)
    plan = (nhw[0], Cout, K, go.shape[2], go.shape[3])
    assert _abi.lib.ppea_conv_image_wgrad_workspace_bytes(*plan) == PI.img_ws_bytes(*plan)   # img_plan restated for the CPU test
    if wdt == "bf16":
        w = w.bfloat16()
    yr, dwr = PI.image_conv_reference(img, w.float(), go)
    x = ops.image_to_nhwc(img.to(device), 8, 0.45, 0.225)
    Cin = img.shape[1]
    assert torch.equal(x[:, :Cin].float().cpu(), ((img - 0.45) / 0.225).bfloat16().float())
    assert float(x[:, Cin:].abs().max()) == 0.0
    wd = w.to(device).requires_grad_(True)
    y = ops.conv2d_nhwc(x, wd, None, 2, K // 2, False, "none", nchw)
    assert y.shape == yr.shape and y.dtype == torch.bfloat16
    assert y.is_contiguous() if nchw else y.is_contiguous(memory_format=CL)
    y.backward(go.to(device).bfloat16())
    err = (y.double().cpu() - yr).abs()
    bound = 2.0 ** -7 * yr.abs() + 1e-3 * yr.abs().max()
    print("y: max err / bound %.3g" % float((err / bound).max()), " dw rel_err %.3g" % rel_err(wd.grad.float().cpu(), dwr))
    assert bool((err <= bound).all())
    assert wd.grad.shape == w.shape and wd.grad.dtype == w.dtype
    assert rel_err(wd.grad.float().cpu(), dwr) < (BWD_TOL if wdt == "f32" else 2.0 ** -7)


# ---- B. nhwc_bn_act ------------------------------------------------------------------------------------------------------
def _run_bn(device, c, groups, act, dtype):
    ops = _ops()
    dev = lambda t: None if t is None else t.to(dtype).to(device).contiguous(memory_format=CL).requires_grad_(True)
    x, res = dev(c["x"]), dev(c["res"])
    w, b = c["weight"].to(device).requires_grad_(True), c["bias"].to(device).requires_grad_(True)
    rm, rv = c["running_mean"].clone().to(device), c["running_var"].clone().to(device)
    assert ops.nhwc_bn_supported(x, groups)
    y, stats = ops.nhwc_bn_act(x, w, b, rm, rv, res, act, groups, 1e-5, 0.1)
    assert y.is_contiguous(memory_format=CL) and y.dtype == dtype
    (y.float() * c["go"].to(device)).sum().backward()
    return dict(y=y.detach(), stats=stats, running_mean=rm, running_var=rv, dx=x.grad, dres=None if res is None else res.grad,
                dweight=w.grad, dbias=b.grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PI.BN_SHAPES, ids=[PI.case_id(s) for s in PI.BN_SHAPES])
def test_nhwc_bn_act_edges(device, shape, dtype):
    """Forward, running statistics (updated once per sub-batch, in order), dx, dres, dgamma, dbeta against F.batch_norm
    in fp64 per sub-batch + residual + ReLU: P below the row-lane count, one row lane, C = 128 / 512 / 2048, three
    sub-batches, the MAX_SLABS cap with its re-derived row count (last slab full, and ragged), a residual.
    Tolerances of test_nhwc_bn_act; at P = 2 alone, where dx vanishes but for eps, dx also gets 1e-6 of its cancelling terms."""
    from ppeadepth import _abi
    groups = shape[4]
    P = (shape[0] // groups) * shape[2] * shape[3]
    assert _abi.lib.ppea_nhwc_bn_slabs(P, shape[1]) == PI.bn_plan(P, shape[1])[3]     # the plan restated for the CPU test
    c = PI.bn_case(shape, dtype)
    ref = PI.bn_reference(c, groups)
    got = _run_bn(device, c, groups, 1, dtype)
    tf, tb = (3e-5, 3e-4) if dtype == torch.float32 else (1e-2, 3e-2)
    figs = {k: rel_err(got[k].float().cpu(), ref[k]) for k in ("y", "running_mean", "running_var", "dweight", "dbias")}
    figs["dx"] = PI.dx_err(got["dx"].float().cpu(), ref, tb, cancelling=P <= 4)
    print({k: "%.3g" % v for k, v in figs.items()})
    assert figs["y"] < tf
    assert figs["running_mean"] < 1e-5 and figs["running_var"] < 1e-4
    assert figs["dx"] < 1
    assert figs["dweight"] < tb and figs["dbias"] < tb
    if ref["dres"] is not None:
        assert rel_err(got["dres"].float().cpu(), ref["dres"]) < tb


@pytest.mark.parametrize("case", PI.LARGE_MEAN_CASES, ids=[PI.case_id(c) for c in PI.LARGE_MEAN_CASES])
def test_nhwc_bn_variance_with_a_large_mean(device, case):
    """var = E[x^2] - mean^2 from fp32 slab partials combined in fp64, on channels with |mean| / std of 1, 10, 30 and 100
    (P = 6000): relative error against fp64 within 3e-7 (1 + (mean / std)^2) + 1e-6, the bound
    test_bn_statistics_from_epilogue_sums_with_a_large_mean holds the other BatchNorm family to; mean to 1e-6; the output
    within what that variance error allows.  C = 16: 128 row lanes, whose sum nhwc_reduce_kernel takes in double (in
    fp32 it measured 1.05 of the bound on a channel 30 std off zero); C = 64: the 32 lanes of the trunk's conv1 width, fp32
    (0.29 of the bound), also at the MAX_SLABS cap (P = 66820)."""
    C, N, H, W = case
    c = PI.bn_large_mean_case(case)
    P = N * H * W
    ref = PI.bn_reference(c, 1, act=0)
    got = _run_bn(device, c, 1, 0, torch.float32)
    x = c["x"].double()
    mean, var = x.mean((0, 2, 3)), ref["var"][0]
    bound = PI.large_mean_bound(mean, var)
    stats = got["stats"].double().cpu()
    rel = (stats[0, 2] * (P - 1) / P - var).abs() / var
    print("variance rel err / bound per channel:", ["%.3g" % v for v in (rel / bound).tolist()])
    assert bool((rel <= bound).all()), (rel / bound).max()
    assert rel_err(stats[0, 0], mean) < 1e-6
    rv = (got["running_var"].double().cpu() - 0.9) / 0.1 * (P - 1) / P
    assert bool(((rv - var).abs() / var <= bound + 1e-5).all())                      # (0.9 + 0.1 v in fp32)
    assert rel_err(got["running_mean"].double().cpu() / 0.1, mean) < 1e-6
    yr = ref["y"]
    allow = (0.5 * bound).view(1, C, 1, 1) * (yr - c["bias"].double().view(1, C, 1, 1)).abs() + 3e-5 * yr.abs().max()
    assert bool(((got["y"].double().cpu() - yr).abs() <= allow).all())


# ---- C. maxpool3x3s2 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", PI.POOL_KINDS)
def test_maxpool3x3s2_edges(device, kind, dtype):
    """1- and 2-pixel axes; all-negative windows (the `first` flag), constant planes (every window a tie: the first element
    in scan order takes the gradient), a +-0 checkerboard (bits compared), -inf entries and whole -inf windows, one NaN
    per image (it wins every window it is in, torch's rule).  fp32: y and dx exactly; bf16: y exactly, dx to the one
    rounding of its fp32 sum."""
    ops = _ops()
    for shape in PI.POOL_SHAPES:
        x, go = PI.pool_case(shape, kind, dtype)
        yr, dxr = PI.pool_reference(x, go)
        xd = x.to(device).contiguous(memory_format=CL).requires_grad_(True)
        y = ops.maxpool3x3s2(xd)
        assert y is not None, shape
        assert y.shape == yr.shape and y.is_contiguous(memory_format=CL)
        y.backward(go.to(device))
        yc, dx = y.detach().cpu(), xd.grad.cpu()
        if kind == "nan":
            assert torch.equal(torch.isnan(yc), torch.isnan(yr)) and bool(torch.isnan(yc).any()), shape
            assert torch.allclose(yc.float(), yr.float(), rtol=0, atol=0, equal_nan=True), shape
        else:
            assert torch.equal(PI.bits(yc), PI.bits(yr)), shape
        if dtype == torch.float32:
            assert torch.equal(PI.bits(dx), PI.bits(dxr)), shape
        else:
            _, exact = PI.pool_reference(x.double(), go.double())
            assert bool(((dx.double() - exact).abs() <= 2.0 ** -8 * exact.abs()).all()), shape


# ---- D. the trunk in isolation -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trunk_reference(cfg):
    return PI.trunk_reference(*cfg)


def _run_trunk(device, cfg, bf16):
    """The product's trunk on the inputs of trunk_reference -> dict with its keys, and the kernel entry points called."""
    from ppeadepth import ops
    from ppeadepth.networks import PoseDecoder, ResnetEncoder
    H, W, groups = cfg
    enc, dec = ResnetEncoder(18, False, num_input_images=2), PoseDecoder([64, 64, 128, 256, 512], 1, 2)
    esd, dsd = PI.split_state(PI.trunk_state(cfg))
    enc.load_state_dict(esd)
    dec.load_state_dict(dsd)
    enc, dec = enc.to(device).train(), dec.to(device).train()
    pairs = PI.trunk_pairs(H, W).to(device)
    ca, ct = (t.to(device) for t in PI.trunk_cotangent())
    called, real_call = set(), ops.call

    def spy(name, *args):
        called.add(name)
        return real_call(name, *args)
    ops.call = spy
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else contextlib.nullcontext():
            feats = enc(pairs, groups=groups)
            aa, tt = dec([feats])
        ((aa.float() * ca).sum() + (tt.float() * ct).sum()).backward()
    finally:
        ops.call = real_call
    out = {"axisangle": aa.detach(), "translation": tt.detach()}
    out.update({f"feature.{i}": f.detach() for i, f in enumerate(feats)})
    for prefix, mod in (("pose_encoder.", enc), ("pose.", dec)):
        for k, p in mod.named_parameters():
            if ".fc." not in k:
                out["grad." + prefix + k] = p.grad
        for k, b in mod.named_buffers():
            if ".fc." not in k:
                out[prefix + k] = b
    return {k: v.detach().cpu() for k, v in out.items()}, called


@pytest.mark.parametrize("cfg", PI.TRUNK_CONFIGS, ids=[PI.config_name(c) for c in PI.TRUNK_CONFIGS])
def test_pose_trunk_fp32_vs_fp64_oracle(device, cfg):
    """ResNet-18 + PoseDecoder in training mode on four frame pairs, one batch with `groups` sub-batches, against
    RefRepDepth.pose_net in fp64 called once per sub-batch in order: both outputs, the five encoder features, every
    parameter gradient (whole tensors), every running mean / variance to rel_err <= 1e-3 each, num_batches_tracked
    exactly.  72x104: the deep maps are 9x13, 5x7, 3x4 (every stride-2 layer ragged)."""
    ref = _trunk_reference(cfg)
    got, called = _run_trunk(device, cfg, False)
    assert set(got) == set(ref)
    assert {"ppea_nhwc_bn_stats_f32", "ppea_nhwc_bn_bwd_apply_f32", "ppea_nhwc_maxpool3x3s2_fwd_f32", "ppea_conv2d_f32_fwd",
            "ppea_conv2d_f32_wgrad"} <= called
    figs = {k: rel_err(got[k], v) for k, v in ref.items() if v.is_floating_point()}
    worst = sorted(figs.items(), key=lambda kv: -kv[1])[:5]
    print("worst rel_err:", [(k, "%.3g" % v) for k, v in worst])
    for k, v in ref.items():
        if not v.is_floating_point():
            assert torch.equal(got[k], v), k
    assert all(v <= 1e-3 for v in figs.values()), worst


@pytest.mark.parametrize("cfg", PI.TRUNK_CONFIGS, ids=[PI.config_name(c) for c in PI.TRUNK_CONFIGS])
def test_pose_trunk_bf16_within_the_floor_band(device, cfg):
    """The same trunk as the bf16 step runs it (image_to_nhwc, conv_image, fused NHWC BatchNorm, conv_nhwc; fp32
    parameters under bf16 autocast).  Every compared tensor -- outputs, features, running statistics and all 68 parameter
    gradients, whole -- stays within PI.band() of its own floor: 2x the rel_err and 4x the 1 - cos (+ 1e-6) that the oracle
    itself shows when its operands and layer outputs are rounded to bf16 at the product's rounding points
    (tests/golden/pose_trunk_bf16_floor.json; the kernels' accumulation order is a second noise of that size, and 1 - cos
    goes with its square), 1 - cos never above 0.5.  The forward keys and a few gradients have floors under the caps
    (1 - cos <= 0.02); most gradients do not (0.05 to 0.15: gates flip under the forward rounding, with more pairs or a
    larger map just as much, CPU test), and for those the band is what a bf16 execution can be held to."""
    ref = _trunk_reference(cfg)
    floor = PI.load_floor()["floor"][PI.config_name(cfg)]
    got, called = _run_trunk(device, cfg, True)
    assert {"ppea_image_to_nhwc_bf16", "ppea_conv_image_bf16", "ppea_conv_image_wgrad_bf16", "ppea_nhwc_bn_stats_bf16",
            "ppea_nhwc_bn_bwd_apply_bf16", "ppea_nhwc_maxpool3x3s2_fwd_bf16", "ppea_nhwc_maxpool3x3s2_bwd_bf16",
            "ppea_conv_nhwc_bf16", "ppea_conv_wgrad_nhwc_bf16"} <= called
    assert not any(n.startswith("ppea_conv2d_") for n in called)
    assert set(floor) == {k for k, v in ref.items() if v.is_floating_point()}
    assert sum(k.startswith("grad.") for k in floor) == 68
    bad, worst = [], {False: (0.0, None), True: (0.0, None)}
    for k, (frel, fcos) in floor.items():
        assert got[k].shape == ref[k].shape and bool(torch.isfinite(got[k]).all()), k
        rel, cos = rel_err(got[k], ref[k]), PI.one_minus_cos(got[k], ref[k])
        brel, bcos = PI.band(frel, fcos)
        ratio = max(rel / brel, cos / bcos)
        g = k.startswith("grad.")
        worst[g] = max(worst[g], (ratio, k))
        if ratio > 1:
            bad.append((k, rel, brel, cos, bcos))
    print("worst share of the band: forward %.3g at %s; gradients %.3g at %s" % (worst[False] + worst[True]))
    for k, v in ref.items():
        if not v.is_floating_point():
            assert torch.equal(got[k], v), k
    assert not bad, bad
