"""CPU proofs behind tests/test_bn_arms_gpu.py: the float64 reference of oracle/bn_inputs.py is nn.BatchNorm2d in double,
the case tables reach the kernels and branches they name, no ReLU case has an element at the kink, and the ill-conditioned
channels have the ratios they claim in the values as stored."""
import pytest
import torch

from oracle import bn_inputs as B

ALL_SHAPES = [c[0] for c in B.CHANNEL_CASES] + list(B.REFUSED_CASES) + [c[0] for c in B.GENERAL_CASES]


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max()))


@pytest.mark.parametrize("shape,two,act,res", [((3, 65, 4, 8), True, 1, True), ((2, 3, 1, 7), False, 2, True),
                                               ((1, 64, 8, 257), True, 0, False)])
def test_reference_is_torch_batchnorm_in_double(shape, two, act, res):
    """Outputs, running statistics and every gradient of `reference` against torch.nn.BatchNorm2d(...).double() composed
    with torch's own activation, mask and residuals under autograd."""
    C = shape[1]
    inp = B.make_inputs(shape, "f32", two, act, res)
    ref = B.reference_of(inp, act=act)
    bns = [torch.nn.BatchNorm2d(C, eps=B.EPS, momentum=B.MOMENTUM).double().train() for _ in range(2)]
    leaves = {k: inp[k].double().clone().requires_grad_(True) for k in ("z1", "z2", "r1", "r2") if k in inp}
    with torch.no_grad():
        bns[0].weight.copy_(inp["g1"]); bns[0].bias.copy_(inp["b1"])
        if two:
            bns[1].weight.copy_(inp["g2"]); bns[1].bias.copy_(inp["b2"])
    u = bns[0](leaves["z1"])
    if two:
        u = u + bns[1](leaves["z2"])
    y = torch.relu(u) if act == 1 else (torch.nn.functional.gelu(u) if act == 2 else u)
    if res:
        y = y * inp["mask"].double().view(-1, 1, 1, 1) + leaves["r1"] + 0.5 * leaves["r2"]
    (y * inp["go"].double()).sum().backward()
    assert _close(ref["u"], u.detach()) and _close(ref["y"], y.detach())
    assert _close(ref["running_mean1"], bns[0].running_mean) and _close(ref["running_var1"], bns[0].running_var)
    assert _close(ref["dz1"], leaves["z1"].grad) and _close(ref["dg1"], bns[0].weight.grad)
    assert _close(ref["db1"], bns[0].bias.grad)
    if two:
        assert _close(ref["running_mean2"], bns[1].running_mean) and _close(ref["running_var2"], bns[1].running_var)
        assert _close(ref["dz2"], leaves["z2"].grad) and _close(ref["dg2"], bns[1].weight.grad)
        assert _close(ref["db2"], bns[1].bias.grad)
    if res:
        assert _close(ref["dr1"], leaves["r1"].grad) and _close(ref["dr2"], leaves["r2"].grad)
    z = inp["z1"].double()
    assert _close(ref["mean1"], z.mean((0, 2, 3))) and _close(ref["var1"], z.var((0, 2, 3), unbiased=False))
    assert _close(ref["invstd1"], (ref["var1"] + B.EPS).rsqrt())


def test_reference_sums_both_uses_and_chains_the_next_form():
    """`go_b` / `g_skip` are further uses under autograd; reference_next equals the two stages composed in one graph."""
    shape = (3, 64, 8, 171)
    inp = B.make_inputs(shape, "f32", res=True, extra=True)
    both = B.reference_of(inp, dup=True, skip=True)
    one = B.reference_of(inp)
    lin = B.reference(inp["z1"], inp["g1"], inp["b1"], mask=inp["mask"], r1=inp["r1"], r2=inp["r2"], r2_scale=0.5,
                      go=inp["go"].double() + inp["go_b"].double())
    assert _close(both["dz1"], lin["dz1"] + inp["g_skip"].double()) and _close(both["dr2"], lin["dr2"])
    assert not _close(both["dz1"], one["dz1"], 1e-3)
    gB, bB = inp["g1"].flip(0), inp["b1"].flip(0)
    A0 = B.reference_of(inp)
    A, Bs = B.reference_next(inp["z1"], inp["g1"], inp["b1"], gB, bB, A0["y"], mask=inp["mask"], r1=inp["r1"], r2=inp["r2"],
                             r2_scale=0.5, go2=inp["go"], go2_b=inp["go_b"], go_y=inp["g_skip"])
    z = inp["z1"].double().requires_grad_(True)
    bnA, bnB = (torch.nn.BatchNorm2d(64, eps=B.EPS).double().train() for _ in range(2))
    with torch.no_grad():
        bnA.weight.copy_(inp["g1"]); bnA.bias.copy_(inp["b1"]); bnB.weight.copy_(gB); bnB.bias.copy_(bB)
    y = bnA(z) * inp["mask"].double().view(-1, 1, 1, 1) + inp["r1"].double() + 0.5 * inp["r2"].double()
    y2 = bnB(y)
    ((y2 * (inp["go"].double() + inp["go_b"].double())).sum() + (y * inp["g_skip"].double()).sum()).backward()
    assert _close(A["y"], y.detach()) and _close(Bs["y"], y2.detach()) and _close(A["dz1"], z.grad, 1e-11)
    assert _close(A["dg1"], bnA.weight.grad, 1e-11) and _close(Bs["dg1"], bnB.weight.grad, 1e-11)
    assert _close(Bs["running_var1"], bnB.running_var)


def test_case_tables_reach_the_branches_they_name():
    seen, raw = set(), set()
    for (N, C, H, W), inst, nv in B.CHANNEL_CASES:
        assert B.channel_ok(N, C, H * W), (N, C, H, W)
        assert B.bn_nv(N, H * W) == nv and B.nv_instance(N, H * W) == inst, (N, C, H, W)
        assert N * C * H * W <= 1 << 20
        seen.add(inst); raw.add(nv)
    assert seen == set(B.NV_INSTANCES) and raw & {5, 6, 7}
    assert any(N * H * W == B.CHANNEL_ELEMS for (N, C, H, W), _, _ in B.CHANNEL_CASES)          # the exact cap
    assert any(H * W == B.VEC and N > 1 for (N, C, H, W), _, _ in B.CHANNEL_CASES)              # hv = 1
    assert any(C % 2 for (N, C, H, W), _, _ in B.CHANNEL_CASES)
    for N, C, H, W in B.REFUSED_CASES:
        assert not B.channel_ok(N, C, H * W)
    assert B.REFUSED_CASES[0][2] * B.REFUSED_CASES[0][3] == B.CHANNEL_ELEMS + 8 and B.REFUSED_CASES[1][1] == 63
    for (N, C, H, W), stats, apply in B.GENERAL_CASES:
        assert not B.channel_ok(N, C, H * W)
        assert ("wave" if B.wave_kernel(H * W) else "block") == stats, (N, C, H, W)
        assert B.apply_kernel(N, C, H * W) == apply, (N, C, H, W)
    hw = {H * W for (N, C, H, W), _, _ in B.GENERAL_CASES}
    assert B.SMALL_PLANE in hw and B.SMALL_PLANE + 8 in hw                                       # the switch, straddled
    assert any(s == "wave" and (N * C) % 4 == 1 for (N, C, H, W), s, _ in B.GENERAL_CASES)       # one live wave at the end
    assert {a for _, _, a in B.GENERAL_CASES} >= {"flat", 1, 2, 4}
    for nv, (N, C, H, W) in B.PER_NV.items():
        assert B.channel_ok(N, C, H * W) and B.nv_instance(N, H * W) == nv
    assert B.PER_NV[8] == (5, 64, 8, 205) and B.bn_nv(5, 8 * 205) == 5
    # the chunked apply cuts (1,3,5,821) into 4 uneven pieces of whole vectors
    per = -(-(-(-4105 // 4)) // 8) * 8
    assert per == 1032 and 4105 - 3 * per == 1009


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_no_relu_case_has_an_element_at_the_kink(shape, dtype):
    """Zero elements with |u| < 64 * 2^-24 * (|a x| + |o|) in the float64 reference of every ReLU case, and the inputs are
    still of the storage type (the moves were whole ulps)."""
    for two, act, res in B.COMBOS:
        if act != B.ACT_RELU:
            continue
        inp = B.make_inputs(shape, dtype, two, act, res)
        assert inp["z1"].dtype == B.storage(dtype)
        ref = B.reference_of(inp, act=act)
        assert B.kink_count(ref) == 0
        assert 0.2 < float((ref["u"] > 0).double().mean()) < 0.8           # ... and ReLU still cuts about half


def test_settling_moves_a_planted_kink():
    inp = B.make_inputs((1, 64, 1, 8), "f32")
    for _ in range(60):                                                   # (the statistics move with the element: iterate)
        ref = B.reference_of(inp)
        a = inp["g1"].double() * ref["invstd1"]
        o = inp["b1"].double() - ref["mean1"] * a
        inp["z1"][0, 5, 0, 3] = float(-o[5] / a[5])                       # pre-activation ~ 0
    assert B.kink_count(B.reference_of(inp, act=B.ACT_RELU)) >= 1
    assert B.settle_kinks(inp) >= 1
    assert B.kink_count(B.reference_of(inp, act=B.ACT_RELU)) == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(4, 64, 32, 32), (4, 64, 8, 513)])
def test_value_cases_hold_the_ratios_they_claim(shape, dtype):
    """In the values AS STORED: |mean| / std within 5 % of the claim (below 0.05 for the ratio-0 channels), variance 0 for
    the constant channel and below eps for the small one, one non-zero element in the outlier channel."""
    inp = B.value_inputs(shape, dtype)
    ratios = dict(B.VALUE_CASES[dtype])
    assert set(inp["recipes"]) == set(ratios) and inp["z1"].dtype == B.storage(dtype)
    z = inp["z1"].double()
    mean, std = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False).sqrt()
    for c, name in enumerate(inp["recipes"]):
        if ratios[name] is not None:
            got = float(mean[c].abs() / std[c])
            assert abs(got - ratios[name]) <= 0.05 * max(ratios[name], 1.0), (c, name, got)
        elif name == "constant":
            assert float(std[c]) == 0.0 and abs(float(mean[c])) == B.CONSTANT_VALUE
        elif name == "tiny_std":
            assert 0.25 * B.TINY_STD ** 2 < float(std[c]) ** 2 < B.EPS / 100
        elif name == "outlier":
            assert int((z[:, c] != 0).sum()) == 1 and float(z[:, c].abs().max()) == B.OUTLIER_VALUE
        elif name == "gamma0":
            assert float(inp["g1"][c]) == 0.0
        elif name == "neg_gamma":
            assert float(inp["g1"][c]) < 0
    if dtype == "f32":
        assert max(r for r in ratios.values() if r is not None) == 300.0
