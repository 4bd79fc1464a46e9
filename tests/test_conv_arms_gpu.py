"""Every instantiation and plan outcome of the dense-convolution kernels (csrc/conv_nhwc.hip, csrc/conv_wgrad.hip) against
the float64 reference of oracle/conv_inputs.py, element by element: output, data gradient, weight gradient and bias gradient
of every table row through ops.conv2d_nhwc / ops.conv_module / ops.conv_transpose_module, each element held to the bound
derived there (tests/test_conv_arms_cpu.py proves the reference, the bound and that the rows reach the arms they name).
A failure names the arm the launch took, from the library's plan query on the arguments of the recorded launch."""
import contextlib

import pytest
import torch

from oracle import conv_inputs as C

pytestmark = pytest.mark.gpu


def _ids(rows):
    return [r.name for r in rows]


@contextlib.contextmanager
def _record(ops):
    """The shape arguments of every dense-conv launch, as the plan queries take them."""
    log, real_call = {"conv": [], "wgrad": [], "elu_bwd": 0}, ops.call

    def spy(name, *a):
        if name == "ppea_conv_nhwc_bf16":       # x w bias flag y | N H W Cin Cout R S stride pad reflect dil Ho Wo act nchw | stream
            log["conv"].append(tuple(a[5:11]) + tuple(a[12:18]) + (a[19],))
        elif name == "ppea_conv_wgrad_nhwc_bf16":   # dz x dw flag ws | N H W Cin Cout R S stride pad reflect Ho Wo | stream
            log["wgrad"].append((a[5], a[8], a[9], a[10], a[12], a[15], a[16]))
        elif name == "ppea_nhwc_bias_elu_bwd_bf16":     # the fused dz = dy * elu'(y) + bias sums of the backward
            log["elu_bwd"] += 1
        return real_call(name, *a)
    ops.call = spy
    try:
        yield log
    finally:
        ops.call = real_call


def _arms(ops, log):
    """-> the arms of the recorded launches: (forward, data gradient, weight gradient)."""
    fwd, dg = log["conv"]
    (wg,) = log["wgrad"]
    pw = ops.conv_wgrad_plan(*wg)
    return (C.arm_of_plan(ops.conv_nhwc_plan(*fwd), fwd[6], fwd[5], fwd[12]), C.arm_of_plan(ops.conv_nhwc_plan(*dg), dg[6], dg[5], dg[12]),
            (wg[4], wg[3], pw["BM"], pw["BN"]), pw)


def _check(name, got, ref, arms):
    arm_of = {"y": arms[0], "dx": arms[1], "dw": (arms[2], arms[3]), "db": "torch sum"}
    for key, g in got.items():
        r, bound = ref[key]
        assert tuple(g.shape) == tuple(r.shape), (name, key, g.shape, r.shape)
        ratio, outside = C.worst(g.cpu(), r, bound)
        print(f"{name} {key}: worst err / bound {ratio:.3f}")
        assert outside == 0, f"{name} {key}: arm {arm_of[key]}, worst err / bound {ratio:.3f}, {outside} of {r.numel()} elements outside"


def _formats(c, y, dx, dw, db, x_shape, w_shape):
    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16 and tuple(dx.shape) == tuple(x_shape)
    if c.nchw:
        assert y.stride(3) == 1 and (c.Cout % 8 != 0 or y.is_contiguous())
    else:
        assert y.stride(1) == 1 and (c.Cout % 8 != 0 or y.is_contiguous(memory_format=torch.channels_last))
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert tuple(dw.shape) == tuple(w_shape) and dw.dtype == {"f32": torch.float32, "bf16": torch.bfloat16}[c.wdtype]
    if c.bias is not None:
        assert tuple(db.shape) == (c.Cout,) and db.dtype == {"f32": torch.float32, "bf16": torch.bfloat16}[c.bias]


def _run(device, c, via="conv2d_nhwc"):
    """One row on the device -> (got, ref, arms)."""
    from ppeadepth import ops
    inp = C.make_inputs(c)
    xd = inp["x"].to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = inp["w"].to(device).requires_grad_(True)
    bd = None if inp["b"] is None else inp["b"].to(device).requires_grad_(True)
    assert ops.conv_supported(xd, wd)
    with _record(ops) as log:
        if via == "conv_module":
            conv = torch.nn.Conv2d(c.Cin, c.Cout, c.k, c.stride, 0 if c.reflect else c.pad, bias=bd is not None)
            conv.weight = torch.nn.Parameter(wd.detach())
            if bd is not None:
                conv.bias = torch.nn.Parameter(bd.detach())
            y = ops.conv_module(conv, xd, c.act, c.reflect, c.nchw)
            assert y is not None
            wd, bd = conv.weight, conv.bias
        else:
            y = ops.conv2d_nhwc(xd, wd, bd, c.stride, c.pad, c.reflect, c.act, c.nchw)
        y.backward(inp["go"].to(device))
    torch.cuda.synchronize()
    want = C.launch_args(c)
    assert log["conv"] == [want["fwd"], want["dgrad"]] and log["wgrad"] == [want["wgrad"]], (log, want)
    assert log["elu_bwd"] == int(C.elu_fused(c)), (c.name, log["elu_bwd"])
    arms = _arms(ops, log)
    _formats(c, y, xd.grad, wd.grad, None if bd is None else bd.grad, xd.shape, inp["w"].shape)
    got = dict(y=y.detach(), dx=xd.grad, dw=wd.grad)
    if bd is not None:
        got["db"] = bd.grad
    ref = C.reference(c, inp, y_saved=y.detach().cpu(), fused=bool(log["elu_bwd"]))
    return got, ref, arms


@pytest.mark.parametrize("c", C.FWD_CASES, ids=_ids(C.FWD_CASES))
def test_forward_instantiations(device, c):
    """One row per conv_nhwc_kernel<BN, stride, KS, layout, RPS> and per conv3x3_resident_kernel<NTC>, on ragged maps."""
    got, ref, arms = _run(device, c)
    assert arms[0] == c.arm, arms
    _check(c.name, got, ref, arms)


@pytest.mark.parametrize("row", C.TILE_CASES, ids=[r[0].name for r in C.TILE_CASES])
def test_pixel_tile_outcomes(device, row):
    """Every outcome of pick_tile at both strides."""
    from ppeadepth import ops
    c, _, trtc = row
    p = ops.conv_nhwc_plan(*C.launch_args(c)["fwd"])
    assert (p["TR"], p["TC"]) == trtc
    got, ref, arms = _run(device, c)
    _check(c.name, got, ref, arms)


@pytest.mark.parametrize("c", C.DGRAD_CASES, ids=_ids(C.DGRAD_CASES))
def test_data_gradient_paths(device, c):
    """The dilated read (the backward of a stride-2 layer) per filter size and BN, and the reflection path: full correlation
    onto the padded domain, then the fold."""
    got, ref, arms = _run(device, c)
    assert arms[1] == c.arm, arms
    _check(c.name, got, ref, arms)


@pytest.mark.parametrize("row", C.WGRAD_CASES, ids=[r[0].name for r in C.WGRAD_CASES])
def test_weight_gradient_instantiations_and_plans(device, row):
    """All 24 conv_wgrad_kernel<stride, KS, BM, BN>, every outcome of the split plan, both slab reducers and their boundary,
    the row groups of the 7 x 7, several patches per workgroup."""
    c, claims = row
    got, ref, arms = _run(device, c)
    assert arms[2] == c.arm and arms[3]["split_rule"] == claims["rule"], arms
    assert "tree" not in claims or arms[3]["tree_reduce"] == claims["tree"]
    _check(c.name, got, ref, arms)


@pytest.mark.parametrize("c", C.EPILOGUE_CASES, ids=_ids(C.EPILOGUE_CASES))
def test_epilogues(device, c):
    """act x bias x layout with Cout in {1, 12, 24} (the zero-pad wrapper, the non-vector store) through ops.conv_module;
    the backward reference forms act'(y) from the device's own stored y."""
    got, ref, arms = _run(device, c, via="conv_module")
    _check(c.name, got, ref, arms)


@pytest.mark.parametrize("c", C.TRANSPOSE_CASES, ids=_ids(C.TRANSPOSE_CASES))
def test_transposed_conv(device, c):
    """ConvTranspose2d(3, stride 2, pad 1, output_padding 1) through ops.conv_transpose_module against F.conv_transpose2d in
    double: output and all gradients."""
    from ppeadepth import ops
    inp = C.make_inputs(c, transposed=True)
    m = torch.nn.ConvTranspose2d(c.Cin, c.Cout, 3, 2, 1, output_padding=1, bias=c.bias is not None)
    m.weight = torch.nn.Parameter(inp["w"].to(device))
    if c.bias is not None:
        m.bias = torch.nn.Parameter(inp["b"].to(device))
    xd = inp["x"].to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with _record(ops) as log:
        y = ops.conv_transpose_module(m, xd)
        assert y is not None
        y.backward(inp["go"].to(device))
    torch.cuda.synchronize()
    want = C.transpose_launch_args(c)
    assert log["conv"] == [want["fwd"], want["dgrad"]] and log["wgrad"] == [want["wgrad"]], (log, want)
    arms = _arms(ops, log)
    Ho, Wo = C.transpose_out_hw(c)
    assert tuple(y.shape) == (c.N, c.Cout, Ho, Wo) and y.is_contiguous(memory_format=torch.channels_last)
    _formats(c, y, xd.grad, m.weight.grad, None if m.bias is None else m.bias.grad, xd.shape, inp["w"].shape)
    got = dict(y=y.detach(), dx=xd.grad, dw=m.weight.grad)
    if c.bias is not None:
        got["db"] = m.bias.grad
    _check(c.name, got, C.reference_transposed(c, inp), arms)


@pytest.mark.parametrize("c", C.SENTINEL_CASES, ids=_ids(C.SENTINEL_CASES))
def test_nothing_is_written_past_a_ragged_edge(device, c):
    """The scalar store paths (channels-last with Cout % 4 != 0; NCHW with Wo % 4 != 0) into a view of a longer buffer
    filled with a pattern: the guard elements before and after the tensor keep the pattern, and the tensor equals the one a
    plain launch returns."""
    from ppeadepth import ops
    N, Cin, H, W, Cout, nchw = c.N, c.Cin, c.H, c.W, c.Cout, c.nchw
    GUARD, PATTERN = 4096, -1234.0
    inp = C.make_inputs(c)
    xd = inp["x"].to(device).contiguous(memory_format=torch.channels_last)
    wp = ops._conv_packed(inp["w"].to(device), False)
    assert (W % 4 != 0) if nchw else (Cout % 4 != 0)
    numel = N * Cout * H * W
    buf = torch.full((numel + 2 * GUARD,), PATTERN, device=device, dtype=torch.bfloat16)
    body = buf[GUARD:GUARD + numel]
    out = body.view(N, Cout, H, W) if nchw else body.view(N, H, W, Cout).permute(0, 3, 1, 2)
    y = ops.conv_nhwc_raw(xd, wp, None, Cout, 3, 3, 1, 1, False, 1, H, W, 0, nchw, out=out)
    plain = ops.conv_nhwc_raw(xd, wp, None, Cout, 3, 3, 1, 1, False, 1, H, W, 0, nchw)
    torch.cuda.synchronize()
    assert y.data_ptr() == body.data_ptr()
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + numel:] == PATTERN).all())
    assert torch.equal(y, plain) and not bool((body == PATTERN).any())
    ref = C.reference(c, inp)
    ratio, outside = C.worst(y.cpu(), *ref["y"])
    assert outside == 0, ratio
