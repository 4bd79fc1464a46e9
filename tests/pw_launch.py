"""TEST INFRASTRUCTURE ONLY -- one launch of each entry point of the pointwise GEMM family (csrc/pwconv.hip, csrc/pwgrad.hip,
csrc/tapsum.hip) on one row of oracle/pw_inputs.py, into NaN-filled views of guarded buffers, under the row's hook variables.
tests/test_pw_arms_gpu.py holds the results to the float64 references; tools/gen_pw_bits_golden.py and
tests/test_pw_bits_gpu.py hash them.  Every launcher returns (served, outputs by name, guarded buffers)."""
import ctypes

import torch

from oracle import pw_inputs as P

BF16, F32 = torch.bfloat16, torch.float32
HOOKS = ("PPEA_PW_TILE", "PPEA_PW_V2", "PPEA_PWGRAD_V2")


class hooks:
    """The row's hook variables for the calls inside, removed after (`monkeypatch`: pytest's fixture or a pytest.MonkeyPatch())."""

    def __init__(self, monkeypatch, env):
        self.mp, self.env = monkeypatch, env

    def __enter__(self):
        for k in HOOKS:
            self.mp.delenv(k, raising=False)
        for k, v in self.env.items():
            self.mp.setenv(k, v)

    def __exit__(self, *exc):
        for k in self.env:
            self.mp.delenv(k, raising=False)


def to(inp, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _dt(name):
    return None if name is None else (BF16 if name == "bf16" else F32)


def launch_pw(ops, c, inp, plan):
    """One row through its entry point into guarded outputs -> (served, outputs, guarded buffers)."""
    dev = inp["x"].device
    shape = (c.B, c.M, 1, c.HW)
    ptr, st = ops.ptr, ops.stream_ptr()
    buf, y = P.guarded(shape, BF16, dev)
    bufs, out = [(buf, BF16)], dict(y=y)
    bp, bflag = ops._bias_arg(inp["bias"])
    if c.epi == 4:
        Pn = plan["partials"] if plan else 1
        buf, sums = P.guarded((c.M, Pn, 2), F32, dev)
        bufs.append((buf, F32))
        out["sums"] = sums
        served = ops.try_call("ppea_pwconv_stats_bf16", ptr(inp["a_arg"]), ptr(inp["x"]), bp, ptr(y), ptr(sums), c.B, c.M, c.K, c.HW, st)
    elif c.epi == 0 and not c.ta and not bflag:
        served = ops.try_call("ppea_pwconv_bf16", ptr(inp["a_arg"]), ptr(inp["x"]), bp, ptr(y), c.B, c.M, c.K, c.HW, st)
    else:
        y2 = None
        if c.epi == 1:
            buf, y2 = P.guarded(shape, BF16, dev)
            bufs.append((buf, BF16))
            out["y2"] = y2
        served = ops.try_call("ppea_pwconv_ex_bf16", ptr(inp["a_arg"]), ptr(inp["x"]), bp, bflag, c.epi, ptr(inp["aux"]), ptr(y), ptr(y2),
                              c.B, c.M, c.K, c.HW, int(c.ta), st)
    return served, out, bufs


def launch_infer(ops, inp):
    """An EPI 5 row through ops.pwconv_table -> (y, y2) or None."""
    return ops.pwconv_table(inp["x"], inp["a"], torch.stack([inp["s"], inp["o"]]), inp["act"], inp["r1"], inp["r2"], inp["r2_scale"],
                            torch.stack([inp["s2"], inp["o2"]]))


def workspace(nbytes, device):
    buf, ws = P.guarded((max(nbytes // 4, 1),), F32, device)
    return buf, ws


def launch_pwgrad(ops, c, inp, device, plan):
    """ppea_pwgrad_bf16 into a guarded `out` of M * N + M floats -> (served, dict(out=...), [out's buffer, the workspace's])."""
    M, N, HW = c.M, c.N, c.H * c.W
    wbuf, ws = workspace(plan["workspace_bytes"], device)
    obuf, out = P.guarded((M * N + M,), F32, device)
    served = ops.try_call("ppea_pwgrad_bf16", ops.ptr(inp["p"]), ops.ptr(inp["q"]), ops.ptr(out), ops.ptr(ws), c.B, M, N, HW, int(c.rowsum),
                          ops.stream_ptr())
    return served, dict(out=out), [(obuf, F32), (wbuf, F32)]


def _into_outputs(c, device):
    wdt, bdt = _dt(c.wdt), _dt(c.bdt)
    dbuf, dw = P.guarded((c.Ch, c.N, 3, 3) if c.taps == 9 else (c.Ch, c.N), wdt, device)
    bufs, out = [(dbuf, wdt)], dict(dw=dw)
    if bdt is not None:
        bbuf, db = P.guarded((P.bias_window(c)[1],), bdt, device)
        bufs.append((bbuf, bdt))
        out["db"] = db
    return out, bufs


def launch_into(ops, c, inp, device, plan):
    """ppea_pwgrad_ex_bf16 into guarded parameter-layout outputs -> (served, outputs, guarded buffers)."""
    M, HW = c.taps * c.Ch, c.H * c.W
    r0, rn = P.bias_window(c) if c.bdt is not None else (0, 0)
    wbuf, ws = workspace(plan["workspace_bytes"], device)
    out, bufs = _into_outputs(c, device)
    served = ops.try_call("ppea_pwgrad_ex_bf16", ops.ptr(inp["p"]), ops.ptr(inp["q"]), ops.ptr(ws), c.B, M, c.N, HW, ops.ptr(out["dw"]),
                          int(c.wdt == "bf16"), c.taps, ops.ptr(out.get("db")), int(c.bdt == "bf16"), r0, rn, ops.stream_ptr())
    return served, out, [(wbuf, F32)] + bufs


def op_args(c, inp):
    """The row as arguments of ops.pwgrad_into / one problem of ops.pwgrad_into_pair."""
    return (inp["p"], inp["q"], (c.Ch, c.N, 3, 3) if c.taps == 9 else (c.Ch, c.N), _dt(c.wdt), c.taps,
            P.bias_window(c) if c.bdt is not None else None, _dt(c.bdt))


def launch_pair(ops, a, b, inps, device, plan):
    """ppea_pwgrad_ex_pair_bf16 on problems a, b -> (served, [outputs of a, outputs of b], guarded buffers, the workspace's first)."""
    i2, vp2 = ctypes.c_int * 2, ctypes.c_void_p * 2
    wbuf, ws = workspace(plan["workspace_bytes"] if plan else 4096, device)
    bufs, outs = [(wbuf, F32)], []
    for c in (a, b):
        o, bf = _into_outputs(c, device)
        outs.append(o)
        bufs += bf
    p_ = lambda ts: vp2(*(None if t is None else t.data_ptr() for t in ts))                  # noqa: E731
    wins = [P.bias_window(c) if c.bdt is not None else (0, 0) for c in (a, b)]
    served = ops.try_call("ppea_pwgrad_ex_pair_bf16", p_([i["p"] for i in inps]), p_([i["q"] for i in inps]), ops.ptr(ws), a.B,
                          i2(a.taps * a.Ch, b.taps * b.Ch), i2(a.N, b.N), a.H * a.W, p_([o["dw"] for o in outs]),
                          i2(*(int(c.wdt == "bf16") for c in (a, b))), i2(a.taps, b.taps), p_([o.get("db") for o in outs]),
                          i2(*(int(c.bdt == "bf16") for c in (a, b))), i2(wins[0][0], wins[1][0]), i2(wins[0][1], wins[1][1]),
                          ops.stream_ptr())
    return served, outs, bufs


def launch_tapsum(ops, c, inp, device):
    """ppea_tapsum_fwd_bf16 and ppea_tapsum_bwd_bf16 -> (both served, dict(pre, h, dT), guarded buffers)."""
    shape = (c.B, c.Ch, c.H, c.W)
    ptr, st = ops.ptr, ops.stream_ptr()
    pbuf, pre = P.guarded(shape, BF16, device)
    hbuf, h = P.guarded(shape, BF16, device)
    tbuf, dT = P.guarded((c.B, 9 * c.Ch, c.H, c.W), BF16, device)
    bp, bflag = ops._bias_arg(inp["bias"])
    served = (ops.try_call("ppea_tapsum_fwd_bf16", ptr(inp["T"]), bp, bflag, ptr(pre), ptr(h), c.B, c.Ch, c.H, c.W, st)
              and ops.try_call("ppea_tapsum_bwd_bf16", ptr(inp["g"]), ptr(dT), c.B, c.Ch, c.H, c.W, st))
    return served, dict(pre=pre, h=h, dT=dT), [(pbuf, BF16), (hbuf, BF16), (tbuf, BF16)]
