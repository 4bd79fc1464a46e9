"""Full fine-tuning (--fullft_reb): the weight-gradient kernels and the trainable 1x1 convolution, each against float64
on the CPU.

Two kinds of check per kernel:
  * EXACT.  Inputs are integers from {-2 .. 2}: every product and every partial sum is an integer below 2^24
    (|sum| <= 4 n), exactly representable in fp32 whatever the summation order, so the kernel must EQUAL float64.
  * REAL VALUES.  randn rounded to the storage type, against float64 on those rounded values.  Per entry
    |got - ref| <= 2 n 2^-24 sum|dy x| with n the number of summed products: the a-priori bound of fp32 summation in any
    order (n u sum|terms|, u = 2^-24), doubled because the matrix instruction's internal adder is not specified to round
    every addition to nearest.
"""
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

BWD_TOL = 2e-4          # tests/test_kernels_gpu.py:18
# library convolution / GEMM kernels (tests/test_e2e_gpu.py::test_bf16_step_launches_no_library_convolution_or_gemm)
LIB = re.compile(r"Cijk_|igemm|ck::|ck_tile|miopen|MIOpen|naive_conv|SubTensorOp|gemm_|Gemm|wmma|batched_transpose")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, seed, dtype):
    return torch.randint(-2, 3, shape, generator=_g(seed)).to(dtype)


def _dw_ref(x, dy, K, stride, pad):
    """float64 depthwise filter gradient [C,1,K,K] by autograd of F.conv2d (linear in the filter: exact)."""
    C = x.shape[1]
    w = torch.zeros(C, 1, K, K, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double(), w, None, stride, pad, 1, C)
    assert y.shape == dy.shape
    (y * dy.double()).sum().backward()
    return w.grad


def _bound(x, dy, K, stride, pad):
    n = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return 2.0 * n * 2.0 ** -24 * _dw_ref(x.abs(), dy.abs(), K, stride, pad)


# ---------------------------------------------------------------------------------------------
# large-kernel depthwise filter gradient on the matrix cores
# ---------------------------------------------------------------------------------------------
LK_SHAPES = [(1, 1, 1, 1, 13), (1, 2, 5, 7, 31), (2, 3, 6, 20, 13), (3, 2, 12, 40, 27), (2, 2, 24, 80, 29),
             (1, 1, 48, 160, 31), (5, 1, 9, 13, 31)]


def _lk_run(device, x, dyb, dys, K):
    from ppeadepth import ops
    got = ops.dwconv_lk_bwd_filter(x.to(device), dyb.to(device), None if dys is None else dys.to(device), K)
    assert got is not None
    assert got[0].dtype == torch.float32 and (dys is None) == (got[1] is None)
    return got[0].cpu().unsqueeze(1), None if dys is None else got[1].cpu().unsqueeze(1)


@pytest.mark.parametrize("KS", [5, 0])
@pytest.mark.parametrize("N,C,H,W,K", LK_SHAPES)
def test_dwconv_lk_filter_gradient_is_exact_on_integers(device, N, C, H, W, K, KS):
    bf = torch.bfloat16
    x, dyb = _ints((N, C, H, W), K + H, bf), _ints((N, C, H, W), K + W + 1, bf)
    dys = _ints((N, C, H, W), 77, bf) if KS else None
    gb, gs = _lk_run(device, x, dyb, dys, K)
    ref = _dw_ref(x, dyb, K, 1, K // 2)
    assert torch.equal(gb.double(), ref), float((gb.double() - ref).abs().max())
    # taps that no (output pixel, input pixel) pair reaches are exactly zero
    u = torch.arange(K) - K // 2
    unreached = (u.abs().view(K, 1) >= H) | (u.abs().view(1, K) >= W)
    assert float(gb[..., unreached].abs().max() if unreached.any() else 0.0) == 0.0
    if KS:
        assert torch.equal(gs.double(), _dw_ref(x, dys, 5, 1, 2))
    # a bitwise function of the inputs: fixed-order sum of the parts, no atomics
    gb2, gs2 = _lk_run(device, x, dyb, dys, K)
    assert torch.equal(gb, gb2) and (gs is None or torch.equal(gs, gs2))


@pytest.mark.parametrize("KS", [5, 0])
@pytest.mark.parametrize("N,C,H,W,K", LK_SHAPES)
def test_dwconv_lk_filter_gradient_real_values(device, N, C, H, W, K, KS):
    bf = torch.bfloat16
    x, dyb = torch.randn(N, C, H, W, generator=_g(K + H)).to(bf), torch.randn(N, C, H, W, generator=_g(K + W + 1)).to(bf)
    dys = torch.randn(N, C, H, W, generator=_g(77)).to(bf) if KS else None
    gb, gs = _lk_run(device, x, dyb, dys, K)
    err, bound = (gb.double() - _dw_ref(x, dyb, K, 1, K // 2)).abs(), _bound(x, dyb, K, 1, K // 2)
    print("lk big  max err / bound", float(err.max()), float(bound.max()))
    assert bool((err <= bound).all()), float((err - bound).max())
    if KS:
        err, bound = (gs.double() - _dw_ref(x, dys, 5, 1, 2)).abs(), _bound(x, dys, 5, 1, 2)
        assert bool((err <= bound).all()), float((err - bound).max())


def test_dwconv_lk_autograd_takes_both_filter_gradients_from_the_mfma_launch(device):
    """ops.dwconv_lk on bf16 activations with trainable filters: weight.grad of both branches is what the one launch
    gives (fp32, parameter shape), also when only the large filter is trainable."""
    from ppeadepth import ops
    N, C, H, W, K = 2, 3, 6, 20, 13
    bf = torch.bfloat16
    x = _ints((N, C, H, W), 1, bf).to(device)
    dyb, dys = _ints((N, C, H, W), 2, bf).to(device), _ints((N, C, H, W), 3, bf).to(device)
    wb = torch.nn.Parameter((torch.randn(C, 1, K, K, generator=_g(4)) / K).to(device))
    ws = torch.nn.Parameter((torch.randn(C, 1, 5, 5, generator=_g(5)) / 5).to(device))
    yb, ys = ops.dwconv_lk(x, wb, ws)
    torch.autograd.backward([yb, ys], [dyb, dys])
    assert wb.grad.dtype == torch.float32 and wb.grad.shape == wb.shape and ws.grad.shape == ws.shape
    assert torch.equal(wb.grad.cpu().double(), _dw_ref(x.cpu(), dyb.cpu(), K, 1, K // 2))
    assert torch.equal(ws.grad.cpu().double(), _dw_ref(x.cpu(), dys.cpu(), 5, 1, 2))
    wb.grad = None
    yb, ys = ops.dwconv_lk(x, wb, ws.detach())
    torch.autograd.backward([yb, ys], [dyb, dys])
    assert torch.equal(wb.grad.cpu().double(), _dw_ref(x.cpu(), dyb.cpu(), K, 1, K // 2))


def test_dwconv_lk_unserved_kernel_size_keeps_the_fp32_kernel(device):
    """K = 7 is not served: PPEA_ERR_UNSUPPORTED through try_call, and ops.dwconv_lk's backward on bf16 activations still
    yields the fp32 kernel's gradient (on fp32 copies of x and dy that live until the launch has them)."""
    from ppeadepth import _abi, ops
    N, C, H, W, K = 2, 3, 6, 20, 7
    bf = torch.bfloat16
    x, dy = _ints((N, C, H, W), 1, bf).to(device), _ints((N, C, H, W), 2, bf).to(device)
    assert _abi.lib.ppea_dwconv_lk_bwd_filter_workspace_bytes(N, C, H, W, K, 0) == -1
    dw = torch.empty(C, K, K, device=device)
    scratch = torch.empty(1024, device=device)
    served = _abi.try_call("ppea_dwconv_lk_bwd_filter_bf16", _abi.ptr(x), _abi.ptr(dy), None, _abi.ptr(dw), None,
                           _abi.ptr(scratch), N, C, H, W, K, 0, _abi.stream_ptr())
    assert served is False and ops.dwconv_lk_bwd_filter(x, dy, None, K) is None
    w = torch.nn.Parameter((torch.randn(C, 1, K, K, generator=_g(4)) / K).to(device))
    y, _ = ops.dwconv_lk(x, w, None)
    y.backward(dy)
    want = torch.empty(C, 1, K, K, device=device)
    xf, dyf = x.float(), dy.float()
    _abi.call("ppea_dwconv_lk_bwd_filter_f32", _abi.ptr(xf), _abi.ptr(dyf), _abi.ptr(want), N, C, H, W, K,
              _abi.stream_ptr())
    assert torch.equal(w.grad, want)
    assert torch.equal(w.grad.cpu().double(), _dw_ref(x.cpu(), dy.cpu(), K, 1, K // 2))


# ---------------------------------------------------------------------------------------------
# depthwise 3x3 filter gradient
# ---------------------------------------------------------------------------------------------
DW3_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (2, 3, 6, 9), (1, 4, 24, 40)]


def _dw3_run(device, x, dy, stride):
    from ppeadepth import ops
    C = x.shape[1]
    w = torch.nn.Parameter((torch.randn(C, 1, 3, 3, generator=_g(9)) / 3).to(device))
    y = ops.dwconv3x3(x.to(device), w, stride)
    assert y.shape == dy.shape
    y.backward(dy.to(device))
    assert w.grad is not None and w.grad.dtype == torch.float32 and w.grad.shape == w.shape
    return w.grad.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("N,C,H,W", DW3_SHAPES)
def test_dwconv3x3_filter_gradient(device, N, C, H, W, stride, dtype):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, dy = _ints((N, C, H, W), H + stride, dtype), _ints((N, C, Ho, Wo), W + stride, dtype)
    got = _dw3_run(device, x, dy, stride)
    assert torch.equal(got.double(), _dw_ref(x, dy, 3, stride, 1)), "integer inputs: exact"
    assert torch.equal(got, _dw3_run(device, x, dy, stride)), "two calls: bitwise equal"
    x = torch.randn(N, C, H, W, generator=_g(H + stride)).to(dtype)
    dy = torch.randn(N, C, Ho, Wo, generator=_g(W + stride)).to(dtype)
    err = (_dw3_run(device, x, dy, stride).double() - _dw_ref(x, dy, 3, stride, 1)).abs()
    bound = _bound(x, dy, 3, stride, 1)
    print("dw3 max err / bound", float(err.max()), float(bound.max()))
    assert bool((err <= bound).all()), float((err - bound).max())


def test_dwconv3x3_frozen_filter_gets_no_gradient(device):
    from ppeadepth import ops
    x = torch.randn(2, 3, 6, 9, generator=_g(1)).to(device).requires_grad_(True)
    w = (torch.randn(3, 1, 3, 3, generator=_g(2)) / 3).to(device)
    y = ops.dwconv3x3(x, w, 2)
    y.sum().backward()
    assert x.grad is not None and w.grad is None


def test_small_dw_module_runs_a_trainable_filter_on_the_hip_kernels(device):
    """SmallDW (stem[1], stem[3], transitions[.][1]) with a trainable filter: no library grouped convolution -- the
    gradients are the kernels' (equal to ops.dwconv3x3's), fp32 and bf16 activations."""
    from ppeadepth import ops
    from ppeadepth.networks import replknet_adapter as rka
    for dtype in (torch.float32, torch.bfloat16):
        m = rka.get_conv2d(4, 4, 3, 2, 1, 1, 4, False).to(device)
        assert isinstance(m, rka.SmallDW) and m.weight.requires_grad
        x = torch.randn(2, 4, 6, 9, generator=_g(3)).to(dtype).to(device)
        go = torch.randn(2, 4, 3, 5, generator=_g(4)).to(dtype).to(device)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            m(xa).backward(go)
            torch.cuda.synchronize()
        names = [e.key for e in prof.key_averages()]
        assert any("dwconv3x3_bwd_filter" in n for n in names), names
        assert not any(LIB.search(n) for n in names), names
        w2 = m.weight.detach().clone().requires_grad_(True)
        ops.dwconv3x3(xb, w2, 2).backward(go)
        assert torch.equal(m.weight.grad, w2.grad) and torch.equal(xa.grad, xb.grad)


# ---------------------------------------------------------------------------------------------
# trainable 1x1 convolution on the bf16 GEMM
# ---------------------------------------------------------------------------------------------
PW_SHAPES = [(1, 32, 32, 2, 4), (2, 64, 32, 6, 20), (3, 32, 96, 3, 8), (2, 128, 512, 6, 20)]


@pytest.mark.parametrize("B,Cin,Cout,H,W", PW_SHAPES)
def test_pwconv_trainable_forward_and_input_gradient_equal_the_frozen_path(device, B, Cin, Cout, H, W):
    from ppeadepth import ops
    g = _g(Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g).bfloat16().to(device)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5).to(device)
    go = torch.randn(B, Cout, H, W, generator=g).bfloat16().to(device)
    for wdt in (torch.float32, torch.bfloat16):                # fp32 parameter / bf16 parameter (with an fp32 master)
        p = torch.nn.Parameter(w.to(wdt))
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        y = ops.pwconv_trainable(xa, p)
        y0 = ops.pwconv_frozen(xb, p.detach().clone())
        assert y is not None and y0 is not None and torch.equal(y, y0)
        y.backward(go)
        y0.backward(go)
        assert torch.equal(xa.grad, xb.grad)
        assert p.grad is not None and p.grad.dtype == wdt and p.grad.shape == p.shape
        ref = torch.einsum("bmhw,bkhw->mk", go.double().cpu(), x.double().cpu())
        absref = torch.einsum("bmhw,bkhw->mk", go.double().cpu().abs(), x.double().cpu().abs())
        n = B * H * W
        err = (p.grad.double().cpu().view(Cout, Cin) - ref).abs()
        bound = 2.0 * n * 2.0 ** -24 * absref
        if wdt == torch.bfloat16:                               # + one rounding to bf16 (8 significant bits: u = 2^-8)
            bound = bound + 2.0 ** -8 * (ref.abs() + bound)
        assert bool((err <= bound).all()), (wdt, float((err - bound).max()))
        # want_sums: the same output bytes, and the epilogue's partial sums give the stored tensor's statistics
        # (bounds of test_pwconv_epilogue_sums_give_the_batchnorm_statistics)
        ys, sums = ops.pwconv_trainable(x, p, want_sums=True)
        assert torch.equal(ys, y) and sums.shape[0] == Cout and sums.shape[2] == 2 and bool(torch.isfinite(sums).all())
        mean, var, _ = ops.bn_batch_stats_from_sums(sums, n, 1e-5, 0.1, None, None)
        yf = ys.double()
        assert rel_err(mean.cpu(), yf.mean((0, 2, 3)).cpu()) < 1e-6
        assert rel_err(var.cpu(), yf.var((0, 2, 3), unbiased=False).cpu()) < 1e-5
        _, sums0 = ops.pwconv_frozen(x, p.detach().clone(), want_sums=True)
        assert torch.equal(sums, sums0)


@pytest.mark.parametrize("B,Cin,Cout,H,W", PW_SHAPES)
def test_pwconv_trainable_weight_gradient_is_exact_on_integers(device, B, Cin, Cout, H, W):
    from ppeadepth import ops
    bf = torch.bfloat16
    x = _ints((B, Cin, H, W), Cin, bf).to(device)
    go = _ints((B, Cout, H, W), Cout + 1, bf).to(device)
    ref = torch.einsum("bmhw,bkhw->mk", go.double().cpu(), x.double().cpu()).view(Cout, Cin, 1, 1)
    p = torch.nn.Parameter(_ints((Cout, Cin, 1, 1), 5, torch.float32).to(device))
    ops.pwconv_trainable(x, p).backward(go)
    assert p.grad.dtype == torch.float32 and torch.equal(p.grad.double().cpu(), ref)
    # bf16 parameter: the exact fp32 sum, rounded once to the parameter's dtype
    q = torch.nn.Parameter(p.detach().to(bf))
    ops.pwconv_trainable(x, q).backward(go)
    assert q.grad.dtype == bf and torch.equal(q.grad.cpu(), ref.float().to(bf))


def test_pwconv_trainable_reads_the_weight_on_every_use(device):
    """Flat Adam updates weights through raw pointers (no version bump): no image of a trainable weight is cached --
    the stale-image case of test_dwconv_trainable_filter_is_repacked."""
    from ppeadepth import ops
    x = torch.randn(2, 64, 6, 20, generator=_g(1)).bfloat16().to(device)
    for wdt in (torch.float32, torch.bfloat16):
        p = torch.nn.Parameter((torch.randn(32, 64, 1, 1, generator=_g(2)) / 8).to(wdt).to(device))
        y1 = ops.pwconv_trainable(x, p)
        v = p._version
        p.data.mul_(2.0)
        assert p._version == v
        y2 = ops.pwconv_trainable(x, p)
        assert torch.equal(y2.float(), 2.0 * y1.float())          # a power of two: exact in every rounding


def test_pointwise_conv_module_unserved_width_falls_back(device):
    """Cin = 48 is no multiple of 32: ops.pwconv_trainable returns None and PointwiseConv keeps ops.Conv2d.  Output, input
    gradient and weight gradient against float64: within BWD_TOL for fp32 tensors; for bf16 activations the stored bf16
    tensors (output, input gradient) within one rounding (2^-8 of the maximum) and the fp32 weight gradient within the
    summation bound of this file."""
    from ppeadepth import ops
    from ppeadepth.networks import replknet_adapter as rka
    B, Cin, Cout, H, W = 2, 48, 32, 6, 20
    g = _g(48)
    x = torch.randn(B, Cin, H, W, generator=g)
    go = torch.randn(B, Cout, H, W, generator=g)
    m = rka.get_conv2d(Cin, Cout, 1, 1, 0, 1, 1, False).to(device)
    assert isinstance(m, rka.PointwiseConv) and m.weight.requires_grad
    assert ops.pwconv_trainable(x.bfloat16().to(device), m.weight) is None
    for dtype in (torch.float32, torch.bfloat16):
        xs, gs = x.to(dtype), go.to(dtype)
        wr = m.weight.detach().double().cpu().requires_grad_(True)
        xr = xs.double().requires_grad_(True)
        yr = F.conv2d(xr, wr)
        yr.backward(gs.double())
        xd = xs.to(device).requires_grad_(True)
        m.weight.grad = None
        y = m(xd)
        y.backward(gs.to(device))
        assert y.dtype == dtype and m.weight.grad.dtype == torch.float32
        if dtype == torch.float32:
            assert rel_err(y.cpu(), yr.detach()) < BWD_TOL
            assert rel_err(xd.grad.cpu(), xr.grad) < BWD_TOL
            assert rel_err(m.weight.grad.cpu(), wr.grad) < BWD_TOL
        else:
            assert rel_err(y.float().cpu(), yr.detach()) < 2.0 ** -8
            assert rel_err(xd.grad.float().cpu(), xr.grad) < 2.0 ** -8
            absw = torch.einsum("bmhw,bkhw->mk", gs.double().abs(), xs.double().abs()).view(Cout, Cin, 1, 1)
            err = (m.weight.grad.double().cpu() - wr.grad).abs()
            assert bool((err <= 2.0 * B * H * W * 2.0 ** -24 * absw).all()), float(err.max())


def test_pointwise_conv_module_takes_the_trainable_gemm(device):
    """PointwiseConv.forward / forward_sums with a trainable weight and bf16 activations: the bf16 GEMM (epilogue sums
    included), no kernel of csrc/conv_f32.hip."""
    from ppeadepth import ops
    from ppeadepth.networks import replknet_adapter as rka
    m = rka.get_conv2d(64, 128, 1, 1, 0, 1, 1, False).to(device)
    x = torch.randn(2, 64, 6, 20, generator=_g(1)).bfloat16().to(device).requires_grad_(True)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        z, sums = m.forward_sums(x, always=True)
        assert sums is not None
        z.backward(torch.ones_like(z))
        y = m(x.detach())
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert any("pwconv" in n for n in names) and any("pwgrad" in n for n in names), names
    assert not any("conv_f32" in n or "conv2d_f32" in n for n in names), names
    assert torch.equal(y, z.detach()) and m.weight.grad.shape == m.weight.shape
    assert torch.equal(y, ops.pwconv_frozen(x.detach(), m.weight.detach().clone()))
