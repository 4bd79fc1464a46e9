"""Full fine-tuning (--fullft_reb): the product MODULES with every parameter trainable -- convolution weights included --
against the functional oracle (oracle/ref_model.py) on CPU autograd: RepLKBlock, ConvFFN, the stem and a transition.
`ref_model.leaf_state_dict` follows the adapter freeze rule, so the leaves are made here."""
import types

import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from oracle import ref_model as RM, synth

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5          # tests/test_kernels_gpu.py:17-18
BWD_TOL = 2e-4
# a ReLU input this close to zero (relative to the tensor's maximum) may change sign between two correct fp32 executions:
# 64 fp32 roundings (u = 2^-24; the pre-activations are sums of a few hundred to a few thousand terms, error ~ sqrt(n) u)
GATE_MARGIN = 64 * 2.0 ** -24


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


class _Stem(nn.Module):
    def __init__(self, C):
        super().__init__()
        from ppeadepth.networks import replknet_adapter as rka
        self.stem = nn.ModuleList([rka.conv_bn_relu(3, C, 3, 2, 1, 1), rka.conv_bn_relu(C, C, 3, 1, 1, C),
                                   rka.conv_bn_relu(C, C, 1, 1, 0, 1), rka.conv_bn_relu(C, C, 3, 2, 1, C)])

    def forward(self, x):
        for layer in self.stem:
            x = layer(x)
        return x


class _Transition(nn.Module):
    def __init__(self, C, C2):
        super().__init__()
        from ppeadepth.networks import replknet_adapter as rka
        self.transitions = nn.ModuleList([nn.Sequential(rka.conv_bn_relu(C, C2, 1, 1, 0, 1),
                                                        rka.conv_bn_relu(C2, C2, 3, 2, 1, C2))])

    def forward(self, x):
        return self.transitions[0](x)


def _make(kind, C, K):
    from ppeadepth.networks import replknet_adapter as rka
    if kind == "blk":
        m = rka.RepLKBlock(C, C, K, 5, drop_path=0.0, adpt_test=4, ratio=0.25)
    elif kind == "ffn":
        m = rka.ConvFFN(C, 4 * C, C, drop_path=0.0, adpt_test=4)
    elif kind == "stem":
        m = _Stem(C)
    else:
        m = _Transition(C, 2 * C)
    synth.fill_state_dict(m)
    for p in m.parameters():
        assert p.requires_grad                   # full fine-tuning: nothing is frozen
    return m


def _oracle(kind, C, K, sd, x, go):
    """Output, input gradient and the gradient of EVERY parameter from the functional oracle (fp32, CPU autograd), and the
    smallest |input| any ReLU gate saw, relative to that input's maximum."""
    opt = types.SimpleNamespace(rep_size="b", g_blk=1.0, g_ffn=1.0, use_checkpoint=False)
    ref = RM.RefRepDepth(sd, opt)
    ref.ch = [C, 2 * C, 4 * C, 8 * C]             # (the stem / transition helpers read their widths from here)
    xr = x.clone().requires_grad_(True)
    margin, real_f = [float("inf")], RM.F

    class _Watched:
        """torch.nn.functional as the ORACLE MODULE sees it, with relu recording its input's margin (only ref_model's
        global name `F` is rebound, and only for this call; torch itself is untouched)."""

        def __getattr__(self, name):
            return getattr(real_f, name)

        @staticmethod
        def relu(t, *a, **k):
            margin[0] = min(margin[0], float(t.detach().abs().min() / t.detach().abs().max()))
            return real_f.relu(t, *a, **k)
    RM.F = _Watched()
    try:
        if kind == "blk":
            yr = ref._replk_block(xr, "m", K, 0.0)
        elif kind == "ffn":
            yr = ref._conv_ffn(xr, "m", 0.0)
        elif kind == "stem":
            yr = ref._stem(xr, "m")
        else:
            yr = ref._transition(xr, "m", 0)
    finally:
        RM.F = real_f
    assert yr.shape == go.shape
    yr.backward(go)
    return yr.detach(), xr.grad, margin[0]


def _case(kind, C, K, B, H, W, gate_margin=0.0):
    """gate_margin: the input is the first of the seeded candidates on which no ReLU gate of the ORACLE sees an input
    closer to zero than this share of its maximum.  A correct fp32 execution may put such an input on the other side
    of the gate, which moves the gradients by O(1) (the input of test_replk_modules_bf16_vs_oracle at C = 64, 6 x 20 has
    one at 3e-8: its docstring records 0.2 in max-norm between two fp32 executions) -- a max-norm comparison of gradients is
    only posed on inputs without one.  The choice reads the oracle alone, never the code under test."""
    m = _make(kind, C, K)
    names = [n for n, _ in m.named_parameters()]
    half = lambda v: (v - 1) // 2 + 1                                                          # noqa: E731
    shape = {"stem": (B, C, half(half(H)), half(half(W))), "trans": (B, 2 * C, half(H), half(W))}.get(kind, (B, C, H, W))
    go = torch.randn(shape, generator=_g(7))
    for candidate in range(40):
        sd = {"m." + k: v.clone() for k, v in m.state_dict().items()}
        for n in names:
            sd["m." + n].requires_grad_(True)
        x = torch.randn(B, 3 if kind == "stem" else C, H, W, generator=_g(C + H + 1000 * candidate))
        yr, dxr, margin = _oracle(kind, C, K, sd, x, go)
        if margin >= gate_margin:
            return names, sd, x, go, yr, dxr
    raise AssertionError("no candidate input keeps the oracle's ReLU gates clear")


FP32_CASES = [("blk", 64, 13, 3, 6, 20), ("blk", 32, 31, 2, 9, 13), ("ffn", 64, 0, 3, 6, 20), ("stem", 32, 0, 2, 24, 40),
              ("stem", 32, 0, 2, 18, 22), ("trans", 32, 0, 2, 6, 20), ("trans", 32, 0, 2, 5, 7)]


@pytest.mark.parametrize("kind,C,K,B,H,W", FP32_CASES)
def test_fullft_modules_fp32_vs_oracle(device, kind, C, K, B, H, W):
    """fp32 step arithmetic: output within FWD_TOL, input gradient and every parameter gradient (1x1, depthwise k x k / 5x5 /
    3x3 and dense stem filters, BatchNorm affine, adapters) within BWD_TOL of the oracle."""
    names, sd, x, go, yr, dxr = _case(kind, C, K, B, H, W, gate_margin=GATE_MARGIN)
    mod = _make(kind, C, K).to(device).train()
    xd = x.to(device).requires_grad_(True)
    y = mod(xd)
    y.backward(go.to(device))
    assert rel_err(y.detach().cpu(), yr) < FWD_TOL
    assert rel_err(xd.grad.cpu(), dxr) < BWD_TOL
    params = dict(mod.named_parameters())
    errs = {n: rel_err(params[n].grad.cpu(), sd["m." + n].grad) for n in names}
    print({n: e for n, e in errs.items() if "conv.weight" in n})
    bad = {n: e for n, e in errs.items() if not e < BWD_TOL}
    assert not bad, bad


@pytest.mark.parametrize("kind,C,K,H,W", [("blk", 64, 13, 6, 20), ("ffn", 128, 0, 6, 20)])
def test_fullft_modules_bf16_vs_oracle(device, kind, C, K, H, W):
    """The bf16 execution with every parameter trainable (trainable 1x1 GEMM with epilogue statistics, MFMA depthwise filter
    gradient, fused BN kernels) against the fp32 oracle, with the comparator and factors of
    tests/test_kernels_gpu.py::test_replk_modules_bf16_vs_oracle: ConvFFN (smooth) within 3e-2 of each tensor's maximum;
    RepLKBlock (two ReLU gates) in L2, no further from the oracle than 1.5x torch's own bf16 autocast of the module + 1e-2."""
    from ppeadepth import ops
    from ppeadepth.networks import replknet_adapter as rka
    B = 3
    names, sd, x, go, yr, dxr = _case(kind, C, K, B, H, W)

    def run():
        mod = _make(kind, C, K).to(device).train()
        xd = x.to(device).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(xd.bfloat16())
        y.backward(go.to(device).bfloat16())
        params = dict(mod.named_parameters())
        return y, xd.grad, {n: params[n].grad for n in names}

    y, dx, dw = run()
    assert y.dtype == torch.bfloat16 and all(dw[n] is not None for n in names)
    assert rel_err(y.float().cpu(), yr) < 3e-2
    if kind == "ffn":
        assert rel_err(dx.cpu(), dxr) < 3e-2
        errs = {n: rel_err(dw[n].float().cpu(), sd["m." + n].grad) for n in names}
        print(errs)
        bad = {n: e for n, e in errs.items() if not e < 3e-2}
        assert not bad, bad
        return
    saved = (rka.FUSE_BN, rka.PW_MFMA, rka.ADAPTER_MFMA, ops._MFMA_K)
    try:
        rka.FUSE_BN = rka.PW_MFMA = rka.ADAPTER_MFMA = False
        ops._MFMA_K = ()
        _, dx_t, dw_t = run()
    finally:
        rka.FUSE_BN, rka.PW_MFMA, rka.ADAPTER_MFMA, ops._MFMA_K = saved
    e, et = _l2(dx.cpu(), dxr), _l2(dx_t.cpu(), dxr)
    assert e < 1.5 * et + 1e-2 and e < 0.3, ("dx", e, et)
    bad = {}
    for n in names:
        e, et = _l2(dw[n].float().cpu(), sd["m." + n].grad), _l2(dw_t[n].float().cpu(), sd["m." + n].grad)
        print(n, e, et)
        if not (e < 1.5 * et + 1e-2 and e < 0.3):
            bad[n] = (e, et)
    assert not bad, bad
