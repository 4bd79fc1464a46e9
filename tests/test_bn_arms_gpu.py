"""Every arm of the training-mode BatchNorm kernels (csrc/bn_fused.hip) against the float64 reference of
oracle/bn_inputs.py, at the smallest shape of every register-tile instantiation of the one-launch channel kernels and at
every branch of the general path.  The reference sees the values as stored; tests/test_bn_arms_cpu.py proves the reference,
the case tables and the ReLU-kink condition.

Tolerances (benign channels; the project's existing numbers): fp32 tensors 2e-5 forward and 2e-4 backward of the tensor's
maximum, statistics 1e-5, running variance 1e-4; bf16 tensors |ref| * 2^-7 + max|ref| * 1e-3 per element; the fp32
statistics and d gamma / d beta sums of a bf16 case at the fp32 numbers."""
import functools

import pytest
import torch

from conftest import rel_err
from oracle import bn_inputs as B

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL, STAT_TOL, RVAR_TOL = 2e-5, 2e-4, 1e-5, 1e-4
DTYPES = ["f32", "bf16"]
CHANNEL_SHAPES = [c[0] for c in B.CHANNEL_CASES]
GENERAL_SHAPES = [c[0] for c in B.GENERAL_CASES] + list(B.REFUSED_CASES)
CHANNEL_IDS = ["x".join(map(str, s)) + f"-nv{i}" for s, i, _ in B.CHANNEL_CASES]
GENERAL_IDS = ["x".join(map(str, s)) for s in GENERAL_SHAPES]
COMBO_IDS = [f"{'two' if t else 'one'}-act{a}-{'res' if r else 'plain'}" for t, a, r in B.COMBOS]
# the front end (batchnorm.fused_bn_act) drives these combinations, ops.* the others
FRONT = {(False, 1, False), (True, 1, True)}
STORED = ("y", "y2", "dz1", "dz2", "dr1", "dr2", "dy")


def _tol(name):
    if name.startswith("running_var"):
        return RVAR_TOL
    if name.startswith(("mean", "invstd", "running_mean")):
        return STAT_TOL
    if name.startswith("var"):
        return 2 * STAT_TOL                                  # 1e-5 on invstd is 2e-5 on the variance
    return FWD_TOL if name in ("y", "y2") else BWD_TOL


def _figure(name, got, ref, dtype):
    """-> (error, bound): fp32 tensors, statistics and parameter sums by rel_err; bf16 tensors per element, as the worst
    ratio of |got - ref| to |ref| * 2^-7 + max|ref| * 1e-3 (bound 1)."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), name
    if dtype == "bf16" and name in STORED:
        allowed = ref.abs() * 2.0 ** -7 + ref.abs().max() * 1e-3
        err = (got - ref).abs()
        return float((err / allowed.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0, 1.0
    return rel_err(got, ref), _tol(name)


def _compare(tag, got, ref, dtype, names=None, sink=None):
    """Prints every figure, then asserts; with `sink` the misses are appended to it and the caller asserts at the end."""
    bad = []
    for name in (names or got):
        err, bound = _figure(name, got[name], ref[name], dtype)
        print(f"{tag} {name}: {err:.3e} (bound {bound:.0e})")
        if not err < bound:
            bad.append((tag, name, err, bound))
    if sink is not None:
        sink.extend(bad)
        return
    assert not bad, bad


@functools.lru_cache(maxsize=4)
def _case(shape, dtype, two, act, res, extra=False):
    """Inputs and float64 reference of one case, computed once (the general-API test reuses the channel test's)."""
    inp = B.make_inputs(shape, dtype, two, act, res, extra)
    ref = B.reference_of(inp, act=act)
    if act == B.ACT_RELU:
        assert B.kink_count(ref) == 0
    return inp, ref


def _bn(C, gamma, beta, device, zero_running=False):
    from ppeadepth.batchnorm import BatchNorm2d
    bn = BatchNorm2d(C, eps=B.EPS, momentum=B.MOMENTUM).to(device).train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
        if zero_running:
            bn.running_var.zero_()
    return bn


def _leaves(inp, device, keys=("z1", "z2", "r1", "r2")):
    return {k: inp[k].to(device).requires_grad_(True) for k in keys if k in inp}


def _res_kw(inp, d, device):
    return dict(mask=inp["mask"].to(device), r1=d["r1"], r2=d["r2"], r2_scale=0.5) if "mask" in inp else {}


def _unbiased_ok(tag, bn, ref, k):
    """The batch's UNBIASED variance, recovered from the running variance (which started at 1), within the variance bound
    (2e-5 of the largest channel; + the fp32 rounding of the stored running variance, 4 * 2^-24 / momentum of it).  Sharper
    than 1e-4 of the blended value: n / (n - 1) differs from 1 by 6.1e-5 at the 16384-element cap, so a biased / unbiased
    mix-up shows at every shape."""
    rv = bn.running_var.double().cpu()
    got = (rv - (1 - B.MOMENTUM)) / B.MOMENTUM
    want = (ref["running_var" + k] - (1 - B.MOMENTUM)) / B.MOMENTUM
    err = float((got - want).abs().max())
    bound = 2 * STAT_TOL * float(want.abs().max()) + 4 * 2.0 ** -24 * float(rv.abs().max()) / B.MOMENTUM
    print(f"{tag} unbiased{k}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (tag, "unbiased" + k, err, bound)


def _collect(d, bn1, bn2, two, res):
    got = dict(dz1=d["z1"].grad, dg1=bn1.weight.grad, db1=bn1.bias.grad, running_mean1=bn1.running_mean,
               running_var1=bn1.running_var)
    if two:
        got.update(dz2=d["z2"].grad, dg2=bn2.weight.grad, db2=bn2.bias.grad, running_mean2=bn2.running_mean,
                   running_var2=bn2.running_var)
    if res:
        got.update(dr1=d["r1"].grad, dr2=d["r2"].grad)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("two,act,res", B.COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("shape", CHANNEL_SHAPES, ids=CHANNEL_IDS)
def test_channel_kernels_against_fp64(device, shape, two, act, res, dtype):
    """bn_fwd_channel / bn_bwd_channel at every instantiation (NV = 1, 2, 3, 4, 8; bn_nv = 5 on the 8; the exact cap;
    hv = 1; odd C): y, saved mean / invstd, both BNs' running statistics and dz1, dz2, dr1, dr2, d gamma, d beta."""
    from ppeadepth import ops
    from ppeadepth.batchnorm import fused_bn_act
    N, C, H, W = shape
    inp, ref = _case(shape, dtype, two, act, res)
    d = _leaves(inp, device)
    assert ops.bn_channel_ok(d["z1"]) and B.channel_ok(N, C, H * W)
    bn1 = _bn(C, inp["g1"], inp["b1"], device)
    bn2 = _bn(C, inp["g2"], inp["b2"], device) if two else None
    kw = dict(z2=d["z2"], bn2=bn2) if two else {}
    kw.update(_res_kw(inp, d, device))
    got = {}
    if (two, act, res) in FRONT:
        y = fused_bn_act(d["z1"], bn1, act=act, **kw)
    else:
        y, st = ops.bn_act_channel(d["z1"], bn1, act=act, **kw)
        got.update(mean1=st[0], invstd1=st[1])
        if two:
            got.update(mean2=st[2], invstd2=st[3])
    (y.float() * inp["go"].to(device).float()).sum().backward()
    got.update(y=y, **_collect(d, bn1, bn2, two, res))
    tag = f"channel {shape} nv={B.nv_instance(N, H * W)} {dtype} {(two, act, res)}"
    _compare(tag, got, ref, dtype)
    _unbiased_ok(tag, bn1, ref, "1")
    if two:
        _unbiased_ok(tag, bn2, ref, "2")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("two,act,res", B.COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("shape", GENERAL_SHAPES, ids=GENERAL_IDS)
def test_general_path_against_fp64(device, shape, two, act, res, dtype):
    """bn_stats_wave | bn_stats -> bn_finalize -> bn_apply_flat | bn_apply (1, 2, 4 chunks) and bn_bwd_reduce_wave |
    bn_bwd_reduce -> bn_bwd_finalize -> bn_bwd_apply_flat | bn_bwd_apply: both sides of the HW = 4096 switch, a last block
    with one live wave, scalar tails, the chunked planes, and the two shapes the channel kernels refuse."""
    from ppeadepth import ops
    from ppeadepth.batchnorm import fused_bn_act
    N, C, H, W = shape
    inp, ref = _case(shape, dtype, two, act, res)
    d = _leaves(inp, device)
    assert not ops.bn_channel_ok(d["z1"]) and not B.channel_ok(N, C, H * W)
    bn1 = _bn(C, inp["g1"], inp["b1"], device)
    bn2 = _bn(C, inp["g2"], inp["b2"], device) if two else None
    got = {}
    if (two, act, res) in FRONT:
        kw = dict(z2=d["z2"], bn2=bn2) if two else {}
        y = fused_bn_act(d["z1"], bn1, act=act, **kw, **_res_kw(inp, d, device))
    else:
        y = _stats_then_apply(ops, d, bn1, bn2, inp, act, device, got)
    (y.float() * inp["go"].to(device).float()).sum().backward()
    got.update(y=y, **_collect(d, bn1, bn2, two, res))
    tag = f"general {shape} {dtype} {(two, act, res)}"
    _compare(tag, got, ref, dtype)
    _unbiased_ok(tag, bn1, ref, "1")
    if two:
        _unbiased_ok(tag, bn2, ref, "2")


def _stats_then_apply(ops, d, bn1, bn2, inp, act, device, got):
    mean1, var1, invstd1 = ops.bn_batch_stats(d["z1"].detach(), B.EPS, B.MOMENTUM, bn1.running_mean, bn1.running_var)
    got.update(mean1=mean1, var1=var1, invstd1=invstd1)
    kw = {}
    if bn2 is not None:
        mean2, var2, invstd2 = ops.bn_batch_stats(d["z2"].detach(), B.EPS, B.MOMENTUM, bn2.running_mean, bn2.running_var)
        got.update(mean2=mean2, invstd2=invstd2)
        kw.update(z2=d["z2"], g2=bn2.weight, b2=bn2.bias, mean2=mean2, invstd2=invstd2)
    return ops.bn_act_apply(d["z1"], bn1.weight, bn1.bias, mean1, invstd1, act=act, **kw, **_res_kw(inp, d, device))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CHANNEL_SHAPES, ids=CHANNEL_IDS)
def test_statistics_and_reduce_in_one_launch_against_fp64(device, shape, dtype):
    """ops.bn_batch_stats + ops.bn_act_apply called directly on the channel-eligible shapes: the one-launch statistics
    (bn_stats_channel) and backward sums (bn_bwd_reduce_channel) with their fixed 8-vector loop, which fused_bn_act never
    takes on one rank, then the flat apply kernels.  Two BNs, ReLU, mask and residuals."""
    from ppeadepth import ops
    two, act, res = True, 1, True
    N, C, H, W = shape
    inp, ref = _case(shape, dtype, two, act, res)
    d = _leaves(inp, device)
    assert ops.bn_channel_ok(d["z1"])
    bn1, bn2 = _bn(C, inp["g1"], inp["b1"], device), _bn(C, inp["g2"], inp["b2"], device)
    got = {}
    y = _stats_then_apply(ops, d, bn1, bn2, inp, act, device, got)
    (y.float() * inp["go"].to(device).float()).sum().backward()
    got.update(y=y, **_collect(d, bn1, bn2, two, res))
    _compare(f"stats_final {shape} {dtype}", got, ref, dtype)
    _unbiased_ok(f"stats_final {shape} {dtype}", bn1, ref, "1")
    _unbiased_ok(f"stats_final {shape} {dtype}", bn2, ref, "2")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["skip", "dup", "skip+dup"])
@pytest.mark.parametrize("nv", [1, 2, 4, 8])
def test_channel_skip_and_dup_against_fp64(device, nv, mode, dtype):
    """`skip`: a second gradient arrives at z1 and is added in the backward launch; `dup`: a second gradient arrives at y and
    is merged in front of it.  Reference: the fp64 sum of both uses.  (ReLU and a DropPath mask, no residuals: the form a
    block's first BatchNorm takes.  The gradients of y lie on a 2^-4 grid, so their bf16 sum is exact; the skip gradient is
    4 x larger, as the residual gradient is in the network, and a bf16 kernel rounds dz to bf16 before it adds.)"""
    from ppeadepth import ops
    shape = B.PER_NV[nv]
    N, C, H, W = shape
    act = B.ACT_RELU
    inp, _ = _case(shape, dtype, False, act, True, True)
    inp = {k: v for k, v in inp.items() if k not in ("r1", "r2")}
    skip, dup = "skip" in mode, "dup" in mode
    ref = B.reference_of(inp, act=act, dup=dup, skip=skip)
    assert B.kink_count(ref) == 0
    leaf = inp["z1"].to(device).requires_grad_(True)
    x = leaf * 1                                                 # a non-leaf input, like a block's
    bn1 = _bn(C, inp["g1"], inp["b1"], device)
    outs = ops.bn_act_channel(x, bn1, mask=inp["mask"].to(device), act=act, skip=skip, dup=dup)
    y = outs[0]
    loss = (y.float() * inp["go"].to(device).float()).sum()
    if skip:
        loss = loss + (outs[2].float() * inp["g_skip"].to(device).float()).sum()
    if dup:
        assert outs[-1].data_ptr() == y.data_ptr()
        loss = loss + (outs[-1].float() * inp["go_b"].to(device).float()).sum()
    loss.backward()
    got = dict(y=y, mean1=outs[1][0], invstd1=outs[1][1], dz1=leaf.grad, dg1=bn1.weight.grad, db1=bn1.bias.grad)
    _compare(f"{mode} {shape} nv={nv} {dtype}", got, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nv", [1, 2, 3, 4, 8])
def test_channel_next_against_fp64(device, nv, dtype):
    """bn_fwd_channel_next / bn_bwd_channel_next(_dup): y = mask * BN_A(z) + r1 + 0.5 * r2 and y2 = BN_B(y) in one launch.
    Stage A against the reference; stage B against the reference fed the kernel's own stored y (the kernel takes BN_B's
    statistics of the rounded values).  Backward with `dup` (two gradients of y2) and a gradient arriving at y: the total
    gradient of y (= d r1, and d r2 after scaling) and BN_B's parameter gradients against the reference, then stage A's
    backward against the reference fed the kernel's own stored gradient of y -- the same isolation, backward."""
    from ppeadepth import ops
    shape = B.PER_NV[nv]
    N, C, H, W = shape
    inp, ref0 = _case(shape, dtype, False, 0, True, True)        # ref0: stage A forward in float64
    g = torch.Generator().manual_seed(1000 + nv)
    gB, bB = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    d = _leaves(inp, device)
    bnA, bnB = _bn(C, inp["g1"], inp["b1"], device), _bn(C, gB, bB, device)
    y, y2, st, y2b = ops.bn_act_channel_next(d["z1"], bnA, bnB, **_res_kw(inp, d, device), dup=True)
    assert y2b.data_ptr() == y2.data_ptr()
    dev = lambda k: inp[k].to(device).float()
    ((y2.float() * dev("go")).sum() + (y2b.float() * dev("go_b")).sum() + (y.float() * dev("g_skip")).sum()).backward()
    dy = d["r1"].grad
    refA, refB = B.reference_next(inp["z1"], inp["g1"], inp["b1"], gB, bB, y.detach().cpu(), mask=inp["mask"], r1=inp["r1"],
                                  r2=inp["r2"], r2_scale=0.5, go2=inp["go"], go2_b=inp["go_b"], go_y=inp["g_skip"],
                                  dy_in=dy.cpu())
    tag = f"next {shape} nv={nv} {dtype}"
    gotA = dict(y=y, mean1=st[0], invstd1=st[1], running_mean1=bnA.running_mean, running_var1=bnA.running_var,
                dz1=d["z1"].grad, dg1=bnA.weight.grad, db1=bnA.bias.grad)
    gotB = dict(y=y2, mean1=st[2], invstd1=st[3], running_mean1=bnB.running_mean, running_var1=bnB.running_var,
                dy=dy, dg1=bnB.weight.grad, db1=bnB.bias.grad)
    bad = []                                                    # every miss of the case is reported, not the first
    _compare(tag + " B", gotB, refB, dtype, sink=bad)
    _compare(tag + " A", gotA, refA, dtype, sink=bad)
    _compare(tag + " dr2", dict(dr2=d["r2"].grad), dict(dr2=0.5 * refB["dy"]), dtype, sink=bad)
    # ... and the gradients against the WHOLE chain in float64 (stage B on the reference's own y), which also holds the
    # backward to the forward's y: fp32 every gradient; bf16 the stored tensors (the 2^-9 rounding of y moves BN_B's xhat,
    # and with it the d gamma_B sum, by more than the fp32 bound of a sum)
    chA, chB = B.reference_next(inp["z1"], inp["g1"], inp["b1"], gB, bB, ref0["y"], mask=inp["mask"], r1=inp["r1"],
                                r2=inp["r2"], r2_scale=0.5, go2=inp["go"], go2_b=inp["go_b"], go_y=inp["g_skip"])
    names = (lambda g: [k for k in g if k in STORED]) if dtype == "bf16" else (lambda g: list(g))
    gradB, gradA = {k: gotB[k] for k in ("dy", "dg1", "db1")}, {k: gotA[k] for k in ("dz1", "dg1", "db1")}
    _compare(tag + " chain B", gradB, chB, dtype, names(gradB), sink=bad)
    _compare(tag + " chain A", gradA, chA, dtype, names(gradA), sink=bad)
    _compare(tag + " chain dr2", dict(dr2=d["r2"].grad), dict(dr2=0.5 * chB["dy"]), dtype, sink=bad)
    assert not bad, bad
    _unbiased_ok(tag + " A", bnA, refA, "1")
    _unbiased_ok(tag + " B", bnB, refB, "1")


@pytest.mark.parametrize("nv,shape", [(1, (2, 64, 32, 32)), (2, (4, 64, 32, 32)), (8, (5, 64, 8, 205))])
def test_channel_statistics_from_epilogue_sums_against_fp64(device, nv, shape):
    """bn_fwd_channel_sums at NV = 1, 2 and 8 (bn_nv = 5): z and its per-channel partial sums from the 1x1 conv's epilogue
    (bf16, M = 64; channels shifted by 1, 10, 30 and 100 standard deviations as in
    test_bn_statistics_from_epilogue_sums_with_a_large_mean), BatchNorm + GELU + mask + residuals in one launch.  Reference:
    the fp64 BatchNorm of the stored z; variance within that test's 3e-7 * (1 + (mean / std)^2) + 1e-6."""
    from ppeadepth import ops
    from ppeadepth.networks import replknet_adapter as rka
    N, M, H, W = shape
    K = 64
    assert B.nv_instance(N, H * W) == nv
    g = torch.Generator().manual_seed(41 + nv)
    conv = rka.PointwiseConv(K, M, 1, 1, 0, 1, 1, False)
    ratio = torch.tensor([1.0, 10.0, 30.0, 100.0]).repeat(M // 4)
    x = torch.randn(N, K, H, W, generator=g)
    x[:, 0] = 1.0                                           # a constant input channel: its weight column shifts the outputs
    with torch.no_grad():
        conv.weight.copy_(torch.randn(M, K, 1, 1, generator=g) / K ** 0.5)
        conv.weight[:, 0, 0, 0] = ratio
    conv.weight.requires_grad_(False)
    conv = conv.to(device)
    conv.weight.data = conv.weight.data.bfloat16()
    z, sums = conv.forward_sums(x.to(device).bfloat16(), always=True)
    assert sums is not None and z.dtype == torch.bfloat16
    inp = B.make_inputs(shape, "bf16", res=True)
    inp["z1"] = z.detach().cpu()
    ref = B.reference_of(inp, act=B.ACT_GELU)
    assert float((ref["mean1"].abs() / ref["var1"].sqrt()).max()) > 60
    bn = _bn(M, inp["g1"], inp["b1"], device, zero_running=True)
    d = _leaves(inp, device, ("r1", "r2"))
    y, st = ops.bn_act_channel(z, bn, act=B.ACT_GELU, sums=sums, **_res_kw(inp, d, device))
    (y.float() * inp["go"].to(device).float()).sum().backward()
    n = N * H * W
    got_var = bn.running_var.double().cpu() / B.MOMENTUM * (n - 1) / n
    rel = (got_var - ref["var1"]).abs() / ref["var1"]
    bound = 3e-7 * (1 + ref["mean1"] ** 2 / ref["var1"]) + 1e-6
    print(f"sums nv={nv}: variance error / bound {float((rel / bound).max()):.3f}")
    assert bool((rel <= bound).all()), float((rel / bound).max())
    assert rel_err(st[0].cpu(), ref["mean1"]) < 1e-6
    assert bool(((st[1].double().cpu() - ref["invstd1"]).abs() <= ref["invstd1"] * (0.5 * bound + 1e-6)).all())
    _compare(f"sums {shape} nv={nv}", dict(y=y, running_mean1=bn.running_mean, dr1=d["r1"].grad, dr2=d["r2"].grad),
             dict(ref, running_mean1=B.MOMENTUM * ref["mean1"]), "bf16")


# ---------------------------------------------------------------------------------------------
# ill-conditioned channels
# ---------------------------------------------------------------------------------------------
# (4,64,64,64) holds exactly 16384 elements per channel, so ops.bn_batch_stats serves it with the one-launch statistics
# (bn_stats_channel) and the backward sums with bn_bwd_reduce_channel; 63 channels put the same planes on the wave kernels.
VALUE_ARMS = {"channel": (4, 64, 32, 32), "stats_channel": (4, 64, 64, 64), "wave": (4, 63, 64, 64),
              "block": (4, 64, 8, 513), "next": (4, 64, 32, 32)}
# Measured on the MI355X: max |got - ref| / (max|ref| * (1 + ratio) * 2^-24) per arm, storage type and channel class, for
# (y, dz); ratio = |mean| * invstd of the class's worst channel in the float64 reference.  The test asserts 4 x these.
VALUE_MEASURED = {
    ("channel", "f32"): {"ratio0": (1.83, 1.86), "ratio1": (0.904, 0.864), "ratio30": (0.525, 0.0418), "ratio300": (0.71,
        0.0232), "constant": (1.93, 0.00121), "tiny_std": (1.28, 2.09), "outlier": (3.35, 3.78), "gamma0": (0.0, 0.0),
        "neg_gamma": (2.1, 2.44)},
    ("channel", "bf16"): {"ratio0": (50100.0, 47400.0), "ratio1": (21900.0, 26400.0), "ratio30": (1450.0, 1470.0),
        "constant": (24.3, 40.5), "tiny_std": (35800.0, 38600.0), "outlier": (35200.0, 39000.0), "gamma0": (10700.0, 0.0),
        "neg_gamma": (47600.0, 49100.0)},
    ("stats_channel", "f32"): {"ratio0": (1.73, 1.69), "ratio1": (1.1, 1.08), "ratio30": (0.655, 0.0435), "ratio300":
        (0.464, 0.0312), "constant": (1.59, 0.00107), "tiny_std": (0.968, 1.83), "outlier": (0.918, 1.44), "gamma0": (0.0,
        0.0), "neg_gamma": (2.66, 2.71)},
    ("stats_channel", "bf16"): {"ratio0": (44400.0, 48600.0), "ratio1": (21300.0, 22500.0), "ratio30": (1540.0, 1640.0),
        "constant": (26.2, 45.5), "tiny_std": (36000.0, 40900.0), "outlier": (29900.0, 36500.0), "gamma0": (42600.0, 0.0),
        "neg_gamma": (42800.0, 49300.0)},
    ("wave", "f32"): {"ratio0": (2.03, 2.02), "ratio1": (1.18, 1.05), "ratio30": (0.361, 0.056), "ratio300": (0.433,
        0.0239), "constant": (2.47, 0.00175), "tiny_std": (1.3, 1.74), "outlier": (8.94, 9.52), "gamma0": (0.0, 0.0),
        "neg_gamma": (1.89, 2.25)},
    ("wave", "bf16"): {"ratio0": (41100.0, 43500.0), "ratio1": (26400.0, 24900.0), "ratio30": (1540.0, 1610.0),
        "constant": (28.1, 37.7), "tiny_std": (47500.0, 35800.0), "outlier": (25400.0, 36100.0), "gamma0": (46900.0, 0.0),
        "neg_gamma": (44200.0, 50000.0)},
    ("block", "f32"): {"ratio0": (1.94, 2.2), "ratio1": (0.832, 0.875), "ratio30": (0.501, 0.0761), "ratio300": (0.564,
        0.021), "constant": (2.54, 0.00138), "tiny_std": (1.22, 2.19), "outlier": (1.23, 1.34), "gamma0": (0.0, 0.0),
        "neg_gamma": (2.19, 2.63)},
    ("block", "bf16"): {"ratio0": (41100.0, 49200.0), "ratio1": (19500.0, 23600.0), "ratio30": (1240.0, 1480.0),
        "constant": (15.3, 37.9), "tiny_std": (36300.0, 36800.0), "outlier": (33800.0, 34800.0), "gamma0": (49500.0, 0.0),
        "neg_gamma": (46600.0, 49600.0)},
    ("next", "f32"): {"ratio0": (1.83, 1.86), "ratio1": (0.904, 0.864), "ratio30": (0.525, 0.0418), "ratio300": (0.71,
        0.0232), "constant": (1.93, 0.00121), "tiny_std": (1.28, 2.09), "outlier": (3.35, 3.78), "gamma0": (0.0, 0.0),
        "neg_gamma": (2.1, 2.44)},
    ("next", "bf16"): {"ratio0": (50100.0, 47400.0), "ratio1": (21900.0, 26400.0), "ratio30": (1450.0, 1470.0),
        "constant": (24.3, 40.5), "tiny_std": (35800.0, 38600.0), "outlier": (35200.0, 39000.0), "gamma0": (10700.0, 0.0),
        "neg_gamma": (47600.0, 49100.0)},
}


def _value_run(device, arm, dtype):
    """-> (got, ref, inp): forward + backward of one arm over the VALUE_CASES channels (no activation; running variance
    started at 0 so that the batch variance is recovered from it to fp32 precision)."""
    from ppeadepth import ops
    shape = VALUE_ARMS[arm]
    C = shape[1]
    inp = B.value_inputs(shape, dtype)
    z = inp["z1"].to(device).requires_grad_(True)
    bn = _bn(C, inp["g1"], inp["b1"], device, zero_running=True)
    go = inp["go"].to(device).float()
    if arm == "next":
        g = torch.Generator().manual_seed(7)
        gB, bB = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
        bnB = _bn(C, gB, bB, device, zero_running=True)
        y, y2, st = ops.bn_act_channel_next(z, bn, bnB)
        (y.float() * go).sum().backward()                   # y2 unused: BN_B's backward contributes zero
        mean, invstd = st[0], st[1]
        refB = B.reference(y.detach().cpu(), gB, bB, rv0=0.0)
        extra = dict(y2=y2, varB=bnB.running_var, invstdB=st[3], refB=refB)
    elif arm == "channel":
        assert ops.bn_channel_ok(z)
        y, st = ops.bn_act_channel(z, bn)
        (y.float() * go).sum().backward()
        mean, invstd, extra = st[0], st[1], {}
    else:
        assert ops.bn_channel_ok(z) == (arm == "stats_channel")
        assert B.wave_kernel(shape[2] * shape[3]) == (arm != "block")
        mean, _, invstd = ops.bn_batch_stats(z.detach(), B.EPS, B.MOMENTUM, bn.running_mean, bn.running_var)
        y = ops.bn_act_apply(z, bn.weight, bn.bias, mean, invstd)
        (y.float() * go).sum().backward()
        extra = {}
    ref = B.reference(inp["z1"], inp["g1"], inp["b1"], go=inp["go"], rv0=0.0)
    got = dict(y=y.detach(), dz1=z.grad, mean1=mean, invstd1=invstd, running_var1=bn.running_var, **extra)
    return got, ref, inp


def _value_constants(got, ref, inp):
    """{class: (c_y, c_dz)}: max |got - ref| / (max|ref| * (1 + ratio) * 2^-24) over the channels of each class."""
    out = {}
    ratio = ref["mean1"].abs() * ref["invstd1"]
    for name in dict.fromkeys(inp["recipes"]):
        ch = [c for c, r in enumerate(inp["recipes"]) if r == name]
        unit = (1 + float(ratio[ch].max())) * 2.0 ** -24
        cs = []
        for k in ("y", "dz1"):
            a, b = got[k].double().cpu()[:, ch], ref[k][:, ch]
            err, top = float((a - b).abs().max()), float(b.abs().max())
            cs.append(0.0 if err == 0.0 else err / (max(top, 1e-30) * unit))
        out[name] = tuple(cs)
    return out


def _two_pass(tag, running_var, invstd, ref, n):
    """(a): batch variance (from a running variance started at 0) within 2e-5 and invstd within 1e-5 of float64, per
    channel; a channel of variance 0: variance <= 1e-12 * mean^2, invstd within 1e-5 of eps^-1/2."""
    var = running_var.double().cpu() / B.MOMENTUM * (n - 1) / n
    invstd = invstd.double().cpu()
    flat = ref["var1"] == 0
    rel = (var - ref["var1"]).abs()[~flat] / ref["var1"][~flat]
    isd = (invstd - ref["invstd1"]).abs() / ref["invstd1"]
    print(f"{tag}: variance {float(rel.max()):.3e} invstd {float(isd.max()):.3e}")
    assert float(rel.max()) <= 2e-5 and float(isd.max()) <= 1e-5
    assert bool((var[flat] <= 1e-12 * ref["mean1"][flat] ** 2).all())
    assert bool(((invstd[flat] * B.EPS ** 0.5 - 1).abs() <= 1e-5).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("arm", list(VALUE_ARMS))
def test_ill_conditioned_channels(device, arm, dtype):
    """Channels with |mean| / std of 0, 1, 30 (fp32: and 300), a constant channel, one with variance below eps, one that is
    zero but for an outlier, gamma = 0 and gamma < 0, through the channel, one-launch statistics, wave, block and next arms.
    (a) The kernels that read the activation take two-pass statistics: the batch variance (recovered from the running
    variance) is within 2e-5 and invstd within 1e-5 of float64 at EVERY ratio -- no growth with (mean / std)^2 --, and the
    constant channel has variance <= 1e-12 * mean^2 and invstd within 1e-5 of eps^-1/2.
    (b) y and dz: the a * x + o form loses about (1 + |mean| / std) * 2^-24 of the channel's maximum; the constant in front
    is measured per arm, storage type and class (VALUE_MEASURED) and 4 x the measured value is asserted (different summation
    orders across instantiations and compiler versions).  bf16 tensors also keep the per-element bound of a stored tensor.
    Measured (MI355X), fp32, over the five arms: y 1.7 .. 2.0 at ratio 0, 0.83 .. 1.2 at ratio 1, 0.36 .. 0.66 at ratio 30,
    0.43 .. 0.71 at ratio 300, 1.6 .. 2.5 for the constant channel (|mean| * invstd = 949), 0.9 .. 8.9 for the outlier channel:
    the constant does not grow with the ratio, the error is the linear model's.  dz (which uses x - mean): 1.7 .. 2.2 at ratio
    0, 0.02 .. 0.08 at ratios 30 and 300.  bf16: the storage rounding 2^-9 dominates (y 4.1e4 .. 5.0e4 at ratio 0, 1.2e3 ..
    1.5e3 at ratio 30).  Variance error 1.4e-7 .. 1.1e-6 and invstd error 9e-8 .. 5.6e-7 over the arms, worst channel (bounds 2e-5, 1e-5)."""
    got, ref, inp = _value_run(device, arm, dtype)
    n = got["y"].numel() // got["y"].shape[1]
    assert [c for c, r in enumerate(inp["recipes"]) if r == "constant"] == torch.nonzero(ref["var1"] == 0).flatten().tolist()
    _two_pass(f"value {arm} {dtype}", got["running_var1"], got["invstd1"], ref, n)
    print(f"value {arm} {dtype}: mean {rel_err(got['mean1'].cpu(), ref['mean1']):.3e}")
    assert rel_err(got["mean1"].cpu(), ref["mean1"]) < STAT_TOL
    if arm == "next":                                        # BN_B reads the stored y from registers: two-pass as well
        _two_pass(f"value next {dtype} B", got["varB"], got["invstdB"], got["refB"], n)
        _compare(f"value next {dtype} B", dict(y=got["y2"]), got["refB"], dtype)
    cs = _value_constants(got, ref, inp)
    for name, (cy, cdz) in cs.items():
        print(f"value {arm} {dtype} {name}: y {cy:.3g} dz {cdz:.3g}")
    if dtype == "bf16":
        _compare(f"value {arm} bf16", dict(y=got["y"], dz1=got["dz1"]), ref, dtype)
    measured = VALUE_MEASURED.get((arm, dtype))
    assert measured is not None, "no measured constants for this arm"
    bad = [(name, c, measured[name]) for name, c in cs.items()
           if c[0] > 4 * measured[name][0] or c[1] > 4 * measured[name][1]]
    assert not bad, bad
