"""CPU proofs behind tests/test_conv_arms_gpu.py: the float64 reference of oracle/conv_inputs.py is torch.nn.Conv2d /
ReflectionPad2d / ConvTranspose2d in double under autograd, every table row reaches the kernel arm it names according to the
library's own plan queries (the functions the launches go by) and the rows reach every arm there is, an fp32 evaluation with
the kernels' rounding points stays inside the per-element bound on every row, no row is larger than 16 M elements and no ReLU
row has a pre-activation at the kink."""
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_inputs as C

ROWS = {c.name: c for c in C.all_cases()}
T_ROWS = {c.name: c for c in C.TRANSPOSE_CASES}


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max()))


def _plans(c):
    from ppeadepth import ops
    a = C.launch_args(c)
    return ops.conv_nhwc_plan(*a["fwd"]), ops.conv_nhwc_plan(*a["dgrad"]), ops.conv_wgrad_plan(*a["wgrad"])


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reflect_ragged", "dil2_k7_bn32", "elu_bf16_nhwc_co12", "sigmoid_f32_nchw_co1",
                                  "relu_f32_nhwc_co24", "wg_s2k1_co40_ci24"])
def test_reference_is_torch_conv2d_in_double(name):
    c = ROWS[name]
    inp = C.make_inputs(c)
    ref = C.reference(c, inp)
    conv = torch.nn.Conv2d(c.Cin, c.Cout, c.k, c.stride, 0 if c.reflect else c.pad, bias=c.bias is not None).double()
    with torch.no_grad():
        conv.weight.copy_(inp["w"])
        if c.bias is not None:
            conv.bias.copy_(inp["b"])
    x = inp["x"].double().requires_grad_(True)
    z = conv(torch.nn.ReflectionPad2d(c.pad)(x) if c.reflect else x)
    y = {"none": lambda t: t, "relu": torch.relu, "elu": torch.nn.ELU(), "sigmoid": torch.sigmoid}[c.act](z)
    (y * inp["go"].double()).sum().backward()
    assert _close(ref["y"][0], y.detach()) and _close(ref["z"], z.detach())
    assert _close(ref["dx"][0], x.grad) and _close(ref["dw"][0], conv.weight.grad)
    if c.bias is not None:
        assert _close(ref["db"][0], conv.bias.grad)
    # the magnitude maps are the same sums over absolute values: they dominate the references
    assert bool((ref["A_y"] >= ref["z"].abs() * (1 - 1e-12)).all())
    for k in ("y", "dx", "dw"):
        assert bool((ref[k][1] >= 0).all())


@pytest.mark.parametrize("name", list(T_ROWS))
def test_reference_is_torch_conv_transpose2d_in_double(name):
    c = T_ROWS[name]
    inp = C.make_inputs(c, transposed=True)
    ref = C.reference_transposed(c, inp)
    m = torch.nn.ConvTranspose2d(c.Cin, c.Cout, 3, 2, 1, output_padding=1, bias=c.bias is not None).double()
    with torch.no_grad():
        m.weight.copy_(inp["w"])
        if c.bias is not None:
            m.bias.copy_(inp["b"])
    x = inp["x"].double().requires_grad_(True)
    y = m(x)
    assert tuple(y.shape[2:]) == C.transpose_out_hw(c)
    (y * inp["go"].double()).sum().backward()
    assert _close(ref["y"][0], y.detach()) and _close(ref["dx"][0], x.grad) and _close(ref["dw"][0], m.weight.grad)
    if c.bias is not None:
        assert _close(ref["db"][0], m.bias.grad)


def test_reflection_fold_is_the_adjoint_of_the_pad():
    c = ROWS["reflect_ragged"]
    g = torch.Generator().manual_seed(3)
    dpad = torch.randn(c.N, c.Cin, c.H + 2, c.W + 2, generator=g, dtype=torch.float64)
    x = torch.randn(c.N, c.Cin, c.H, c.W, generator=g, dtype=torch.float64)
    lhs = float((F.pad(x, (1,) * 4, mode="reflect") * dpad).sum())
    assert abs(lhs - float((x * C.fold64(dpad, c)).sum())) <= 1e-9 * abs(lhs)
    # reference(): dx of a reflection row is the fold of the padded-domain gradient it also returns
    inp = C.make_inputs(c)
    ref = C.reference(c, inp)
    assert _close(C.fold64(ref["dpad"], c), ref["dx"][0])


# ---------------------------------------------------------------------------------------------
# the tables reach the arms they name, and every arm there is
# ---------------------------------------------------------------------------------------------
def test_forward_rows_reach_every_instantiation():
    seen = set()
    for c in C.FWD_CASES:
        fwd, _, _ = _plans(c)
        arm = C.arm_of_plan(fwd, c.stride, c.k, c.nchw)
        assert arm == c.arm, (c.name, arm, c.arm)
        seen.add(arm)
    assert len(C.ALL_FWD_ARMS) == 43
    assert seen == C.ALL_FWD_ARMS, seen ^ C.ALL_FWD_ARMS
    # ragged extents where the arm allows it
    for c in C.FWD_CASES:
        fwd, _, _ = _plans(c)
        Ho, Wo = C.out_hw(c)
        assert Ho % fwd["TR"] and Wo % fwd["TC"] or (c.nchw and Wo % 4 == 0), c.name
        assert (c.Cin % 32 and c.Cout % 32) or c.arm[0] == "resident", c.name
    assert any(c.Cin % 32 and c.Cout % 16 for c in C.FWD_CASES if c.arm[0] == "resident")
    assert any(c.N > 1 for c in C.FWD_CASES)
    nchw = [c for c in C.FWD_CASES if c.nchw]
    # both NCHW stores (8-byte at Wo % 4 == 0, scalar otherwise) under every filter size, every BN, RPS 3 and both strides
    for pick in ([lambda c, k=k: c.k == k for k in (1, 3, 7)] + [lambda c, bn=bn: c.arm[1] == bn for bn in (32, 64, 128)]
                 + [lambda c: c.arm[5] == 3] + [lambda c, s=s: c.stride == s for s in (1, 2)]):
        assert {C.out_hw(c)[1] % 4 == 0 for c in nchw if pick(c)} == {False, True}
    for c in nchw:                                     # the scalar NCHW store forces the 8 x 16 tile
        if C.out_hw(c)[1] % 4:
            fwd, _, _ = _plans(c)
            assert (fwd["TR"], fwd["TC"]) == (8, 16), c.name
    assert any(c.reflect for c in C.FWD_CASES if c.arm[0] == "resident")
    assert any(not c.reflect for c in C.FWD_CASES if c.arm[0] == "resident")


def test_tile_rows_take_every_pick_tile_outcome():
    from ppeadepth import ops
    tags = set()
    for c, tag, trtc in C.TILE_CASES:
        fwd, _, _ = _plans(c)
        Ho, Wo = C.out_hw(c)
        assert (fwd["TR"], fwd["TC"]) == trtc, (c.name, fwd)
        tags.add((tag, c.stride))
        tiles = -(-Ho // trtc[0]) * -(-Wo // trtc[1])
        if tag == "default":
            assert trtc == (8, 16)
        elif tag in ("full_width", "full_width_clamped"):
            assert trtc[1] == Wo <= 64 and trtc[0] == min(128 // Wo, Ho)
            assert (128 // Wo > Ho) == (tag == "full_width_clamped")
        elif tag == "halo_rejected":
            # the library's own word: the same output map under a 1 x 1 filter (whose halo is the tile itself, under every
            # cap) takes a tile with fewer workgroups -- the filter size enters pick_tile through the halo cap alone
            a = list(C.launch_args(c)["fwd"])
            a[5], a[7] = 1, 0
            twin = ops.conv_nhwc_plan(*a)
            assert c.k > 1 and (twin["TR"], twin["TC"]) != trtc
            assert -(-Ho // twin["TR"]) * -(-Wo // twin["TC"]) < tiles, (c.name, twin)
        elif tag == "nchw_skipped":
            assert c.nchw and Wo % 4 and Wo <= 64
            a = list(C.launch_args(c)["fwd"])
            a[-1] = 0
            twin = ops.conv_nhwc_plan(*a)                      # the channels-last twin takes the full-width tile
            assert twin["TC"] == Wo and (fwd["TR"], fwd["TC"]) != (twin["TR"], twin["TC"])
    want = {"default", "4x32", "2x64", "full_width", "full_width_clamped", "halo_rejected", "nchw_skipped"}
    assert tags == {(t, s) for t in want for s in (1, 2)}


def test_dgrad_rows_reach_the_dilated_and_the_reflection_path():
    seen = set()
    for c in C.DGRAD_CASES:
        _, dg, _ = _plans(c)
        arm = C.arm_of_plan(dg, 1, c.k, False)
        assert arm == c.arm, (c.name, arm)
        args = C.launch_args(c)["dgrad"]
        if c.reflect:
            Ho, Wo = C.out_hw(c)
            assert args[6:10] == (1, c.k - 1, 0, 1) and args[10:12] == (Ho + 2, Wo + 2)      # full correlation, then the fold
        else:
            assert c.stride == 2 and args[9] == 2 and c.H % 2 and c.W % 2                   # dil = 2, odd H and W
            seen.add((c.k, arm[1], arm[5]))
    assert {(k, bn, 1) for k in (1, 3, 7) for bn in (32, 64)} <= seen and any(r == 3 for _, _, r in seen)
    refl = [c for c in C.DGRAD_CASES if c.reflect]
    assert any((c.H, c.W) == (3, 3) for c in refl) and any(c.H != c.W and c.N > 1 and c.Cin % 32 for c in refl)


def test_wgrad_rows_reach_every_instantiation_and_plan_outcome():
    arms, rules, reducers, slabs = set(), set(), set(), set()
    deep = 0
    for c, claims in C.WGRAD_CASES:
        _, _, p = _plans(c)
        arm = (c.stride, c.k, p["BM"], p["BN"])
        assert arm == c.arm, (c.name, arm)
        assert p["split_rule"] == claims["rule"], (c.name, p)
        for key in ("slabs", "rgroups"):
            assert key not in claims or p[key] == claims[key], (c.name, key, p)
        assert "tree" not in claims or p["tree_reduce"] == claims["tree"], (c.name, p)
        assert p["n_patches"] // p["splits"] >= claims.get("ppw", 1), (c.name, p)
        deep += p["n_patches"] // p["splits"] >= 3
        arms.add(arm); rules.add(p["split_rule"]); reducers.add(p["tree_reduce"]); slabs.add((p["slabs"], p["tree_reduce"]))
        if c.k == 7:
            assert p["rows_per_block"] == 1 and p["rgroups"] == 7
    assert len(C.ALL_WGRAD_ARMS) == 24 and arms == C.ALL_WGRAD_ARMS, arms ^ C.ALL_WGRAD_ARMS
    assert rules == set(C.SPLIT_RULES)
    assert reducers == {0, 1} and (16, 0) in slabs and (17, 1) in slabs          # the boundary, straddled
    assert deep >= 3
    rows = [c for c, _ in C.WGRAD_CASES]
    assert any(c.stride == 2 for c, cl in C.WGRAD_CASES if cl.get("ppw", 1) >= 3)
    assert {c.reflect for c in rows} == {False, True} and {c.wdtype for c in rows} == {"f32", "bf16"}
    assert {c.stride for c in rows if c.k == 7} == {1, 2}


def test_epilogue_and_transpose_rows_cover_their_factors():
    rows = C.EPILOGUE_CASES
    assert {(c.act, c.bias, c.nchw) for c in rows} == {(a, b, n) for a in C.ACTS for b in (None, "f32", "bf16") for n in (False, True)}
    assert {c.Cout for c in rows} == {1, 12, 24} and len({(c.N, c.Cin, c.H, c.W) for c in rows}) == 2
    for act in C.ACTS:
        assert {c.Cout for c in rows if c.act == act} == {1, 12, 24}
    assert {(c.N, c.Cin, c.H, c.W) for c in C.TRANSPOSE_CASES} == {(1, 8, 3, 5), (2, 40, 7, 9)}
    assert {((c.N, c.Cin), c.bias is not None) for c in C.TRANSPOSE_CASES} == {((n, ci), b) for n, ci in ((1, 8), (2, 40))
                                                                                for b in (False, True)}


def test_existing_wgrad_plan_numbers_hold_through_the_query():
    """The numbers tests/test_host_cpu.py reads off the workspace size, from the plan itself."""
    from ppeadepth import _abi, ops
    for args, slabs, rule in (((12, 512, 256, 3, 1, 24, 80), 8, "fill"), ((12, 256, 128, 3, 1, 48, 160), 32, "fill"),
                              ((12, 1024, 512, 3, 1, 12, 40), 4, "floor")):
        p = ops.conv_wgrad_plan(*args)
        assert (p["slabs"], p["split_rule"]) == (slabs, rule), p
        N, Cin, Cout, K, s, Ho, Wo = args
        per_slab = K * K * (-(-Cout // p["BM"]) * p["BM"]) * (-(-Cin // p["BN"]) * p["BN"]) * 4
        assert _abi.lib.ppea_conv_wgrad_workspace_bytes(N, Cin, Cout, K, K, s, Ho, Wo) == per_slab * p["slabs"]
    assert ops.conv_wgrad_plan(12, 64, 64, 3, 1, 96, 320)["splits"] >= 256
    # layers of the benchmarked step (batch 12 at 192 x 640, pose trunk at 24 images) that take arms only these tables pin:
    # a stride-2 ResNet conv and its 1 x 1 downsample at BN = 64, 256 -> 512 stride 2 with the whole weight slice per step,
    # the dilated data gradient of 128 -> 256 stride 2 likewise, the 768 -> 256 decoder conv at the workspace cap
    assert C.arm_of_plan(ops.conv_nhwc_plan(24, 48, 160, 64, 128, 3, 2, 1, 0, 1, 24, 80, 0), 2, 3, 0) == C.tile(64, 2, 3)
    assert C.arm_of_plan(ops.conv_nhwc_plan(24, 48, 160, 64, 128, 1, 2, 0, 0, 1, 24, 80, 0), 2, 1, 0) == C.tile(64, 2, 1)
    assert C.arm_of_plan(ops.conv_nhwc_plan(24, 24, 80, 256, 512, 3, 2, 1, 0, 1, 12, 40, 0), 2, 3, 0) == C.tile(64, 2, 3, rps=3)
    assert C.arm_of_plan(ops.conv_nhwc_plan(24, 24, 80, 256, 128, 3, 1, 1, 0, 2, 48, 160, 0), 1, 3, 0) == C.tile(64, 1, 3, 0, 3)
    assert ops.conv_wgrad_plan(12, 768, 256, 3, 1, 24, 80)["split_rule"] == "cap"
    # refusals are those of the launches
    with pytest.raises(_abi.PpeaKernelError):
        ops.conv_nhwc_plan(1, 8, 8, 12, 8, 3, 1, 1, 0, 1, 8, 8, 0)            # Cin % 8
    with pytest.raises(_abi.PpeaKernelError):
        ops.conv_wgrad_plan(1, 8, 8, 5, 1, 8, 8)                              # 5 x 5


# ---------------------------------------------------------------------------------------------
# sizes and kinks
# ---------------------------------------------------------------------------------------------
def test_no_case_tensor_exceeds_16m_elements():
    for c in C.all_cases():
        assert C.elements(c) <= 16 << 20, c.name
    for c in C.TRANSPOSE_CASES:
        assert C.elements(c, transposed=True) <= 16 << 20
    assert len({c.name for c in C.all_cases()}) == len(C.all_cases())


def test_no_relu_row_has_an_element_at_the_kink():
    relu = [c for c in C.all_cases() if c.act == "relu"]
    assert len(relu) >= 6
    for c in relu:
        inp = C.make_inputs(c)
        assert C.kink_count(c, inp) == 0, c.name
        assert torch.equal(inp["w"].float(), inp["w"].float().bfloat16().float())          # the moves were whole bf16 ulps
        z = C.reference(c, inp)["z"]
        assert 0.2 < float((z > 0).double().mean()) < 0.8                                   # ... and ReLU still cuts about half


def test_settling_moves_a_planted_kink():
    c = ROWS["relu_f32_nhwc_co24"]
    inp = C.make_inputs(c)
    assert C.kink_count(c, inp) == 0
    z = C.reference(c, inp)["z"]
    b = inp["b"].double()
    b[3] -= z[1, 3, 2, 4]                                  # one pre-activation of channel 3 is now zero up to fp32 rounding
    inp["b"] = b.float()
    assert C.kink_count(c, inp) >= 1
    assert C.settle_kinks(c, inp) >= 1 and C.kink_count(c, inp) == 0


# ---------------------------------------------------------------------------------------------
# the bound holds for an fp32 evaluation with the kernels' rounding points: every row, every element
# ---------------------------------------------------------------------------------------------
def _bf(t):
    return t.bfloat16().float()


def _fp32_standin(c, inp):
    """What a correct kernel family computes, in fp32 on the CPU: bf16 operands, fp32 sums, one rounding per stored tensor
    (y; dz = go * act'(y) in bf16 arithmetic; the padded-domain gradient of a reflection row before its fold; dx; dw; db)."""
    x = inp["x"].float().requires_grad_(True)
    w = inp["w"].float().clone().requires_grad_(True)
    b = None if inp["b"] is None else inp["b"].float()
    xp = F.pad(x, (c.pad,) * 4, mode="reflect") if c.reflect else x
    if c.reflect:
        xp.retain_grad()
    z = F.conv2d(xp, w, b, c.stride, 0 if c.reflect else c.pad)
    y = _bf({"none": z, "relu": torch.relu(z), "elu": F.elu(z), "sigmoid": torch.sigmoid(z)}[c.act].detach())
    dz, dz_b = (t.float() for t in C.stored_dz(c, inp["go"], y, C.elu_fused(c)))
    z.backward(dz)
    if c.reflect:
        t = torch.zeros_like(x, requires_grad=True)
        dx = torch.autograd.grad(F.pad(t, (c.pad,) * 4, mode="reflect"), t, grad_outputs=_bf(xp.grad))[0]
    else:
        dx = x.grad
    out = dict(y=y, dx=_bf(dx), dw=_bf(w.grad) if c.wdtype == "bf16" else w.grad)
    if b is not None:
        db = dz_b.sum((0, 2, 3))
        out["db"] = _bf(db) if c.bias == "bf16" else db
    return out


@pytest.mark.parametrize("act", ["relu", "elu", "sigmoid"])
def test_stored_dz_is_the_rounded_product(act):
    """stored_dz is go * act'(y) up to the roundings it names (0, 2, 3; one for the fused ELU kernel), stays on the bf16
    grid, and the fused form's bias operand is the unrounded fp32 product."""
    c = next(r for r in C.EPILOGUE_CASES if r.act == act and r.bias)
    g = torch.Generator().manual_seed(11)
    y = (torch.rand(2, 8, 5, 7, generator=g) * 1.6 - 0.8).bfloat16()
    if act == "sigmoid":
        y = y.abs()
    go = torch.randn(2, 8, 5, 7, generator=g).bfloat16()
    exact = go.double() * C.act_grad64(y.double(), act)
    for fused, k in ((False, {"relu": 0, "elu": 2, "sigmoid": 3}[act]),) + (((True, 1),) if act == "elu" else ()):
        dz, dz_b = C.stored_dz(c, go, y, fused)
        assert torch.equal(dz, dz.bfloat16().double())
        assert bool(((dz - exact).abs() <= ((1 + C.U_BF16) ** k - 1) * exact.abs()).all())
        if fused:
            assert not torch.equal(dz_b, dz) and bool(((dz_b - exact).abs() <= 2.0 ** -22 * exact.abs()).all())
        else:
            assert torch.equal(dz_b, dz)


@pytest.mark.parametrize("name", list(ROWS))
def test_fp32_evaluation_stays_inside_the_bound(name):
    c = ROWS[name]
    inp = C.make_inputs(c)
    got = _fp32_standin(c, inp)
    ref = C.reference(c, inp, y_saved=got["y"])
    for key, g in got.items():
        r, bound = ref[key]
        assert g.shape == r.shape
        ratio, outside = C.worst(g, r, bound)
        assert outside == 0, (name, key, ratio, outside)


@pytest.mark.parametrize("name", list(T_ROWS))
def test_fp32_transposed_evaluation_stays_inside_the_bound(name):
    c = T_ROWS[name]
    inp = C.make_inputs(c, transposed=True)
    x = inp["x"].float().requires_grad_(True)
    w = inp["w"].float().clone().requires_grad_(True)
    b = None if inp["b"] is None else inp["b"].float().clone().requires_grad_(True)
    y = F.conv_transpose2d(x, w, b, 2, 1, output_padding=1)
    y.backward(inp["go"].float())
    got = dict(y=_bf(y.detach()), dx=_bf(x.grad), dw=_bf(w.grad) if c.wdtype == "bf16" else w.grad)
    if b is not None:
        got["db"] = _bf(b.grad) if c.bias == "bf16" else b.grad
    ref = C.reference_transposed(c, inp)
    for key, g in got.items():
        ratio, outside = C.worst(g, *ref[key])
        assert outside == 0, (name, key, ratio, outside)


def test_the_bound_refuses_a_subtly_wrong_result():
    """One output element off by a single bf16 ulp of its neighbourhood's scale, one tap dropped, a transposed filter:
    each leaves the bound."""
    c = ROWS["reflect_ragged"]
    inp = C.make_inputs(c)
    got = _fp32_standin(c, inp)
    ref = C.reference(c, inp, y_saved=got["y"])
    y = got["y"].clone()
    big = int(ref["y"][0].abs().flatten().argmax())
    y.view(-1)[big] *= 1 + 2.0 ** -6                                 # two bf16 ulps on one element
    assert C.worst(y, *ref["y"])[1] == 1
    # an element that is not a number, or not finite, is outside its bound: in y, dx, the fp32-typed dw and db alike
    for key in got:
        for poison in (float("nan"), float("inf"), -float("inf")):
            g = got[key].clone()
            g.view(-1)[g.numel() // 2] = poison
            ratio, outside = C.worst(g, *ref[key])
            assert outside == 1 and ratio == float("inf"), (key, poison, ratio, outside)
        assert C.worst(got[key], *ref[key])[1] == 0
    bad = dict(inp, w=inp["w"].transpose(2, 3).contiguous())
    assert C.worst(_fp32_standin(c, bad)["y"], *ref["y"])[1] > 0
    drop = dict(inp, w=inp["w"].clone())
    drop["w"][:, -1, 2, 2] = 0                                       # the last channel of one tap: the `ch < Cin` mask's edge
    g = _fp32_standin(c, drop)
    assert C.worst(g["y"], *ref["y"])[1] > 0 and C.worst(g["dx"], *ref["dx"])[1] > 0
