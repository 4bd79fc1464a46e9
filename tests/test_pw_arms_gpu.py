"""Every instantiation of the pointwise GEMM family an exported entry point can launch -- csrc/pwconv.hip (v1 and the v2 LDS-DMA
ring, both A modes, every tile and epilogue), csrc/pwgrad.hip (both main kernels, the pair form, the two reduce kernels) and
csrc/tapsum.hip -- against the float64 references of oracle/pw_inputs.py, element by element, each element held to the bound
derived there.  Outputs (and the split workspace and the statistics partials) are NaN-filled views into guarded buffers: an
element never stored is outside its bound, a store past either end changes a guard.  Every row asserts that the entry point
served it exactly when the library's plan query has a plan for it; a failure names the arm from that query on the launch's own
arguments (tests/test_pw_arms_cpu.py proves that the plan names the arm the row is there for, the references, the bounds, and
that the bounds catch index faults).  Hook rows set their variables for the one call; the hooks are read per call."""
import pytest
import torch

import pw_launch as L
from oracle import pw_inputs as P
from pw_launch import hooks as _hooks, to as _to

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _ids(rows):
    return [r.name for r in rows]


def _hold(tag, arm, got, ref, bufs=()):
    """Every output element inside its bound, every guard intact; prints the worst ratio per output."""
    for key, (ref_t, bound) in ref.items():
        g = got[key]
        assert tuple(g.shape) == tuple(ref_t.shape), (tag, key, arm)
        ratio, outside = P.worst(g, ref_t, bound)
        print(f"PWARM {arm} | {tag} {key}: worst err / bound {ratio:.3f}")
        assert outside == 0, f"{tag} {key} ({arm}): worst err / bound {ratio:.3f}, {outside} of {ref_t.numel()} elements outside"
    for buf, dtype in bufs:
        assert P.guards_intact(buf, dtype), f"{tag} ({arm}): a guard element was overwritten"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ---------------------------------------------------------------------------------------------
# pwconv
# ---------------------------------------------------------------------------------------------
def _pw_row(device, monkeypatch, c):
    from ppeadepth import _abi, ops
    inp = _to(P.make_pw_inputs(c), device)
    with _hooks(monkeypatch, c.env):
        plan = ops.pwconv_plan(c.B, c.M, c.K, c.HW, c.ta)
        served, got, bufs = L.launch_pw(ops, c, inp, plan)
        torch.cuda.synchronize()
        if c.epi == 4:
            assert _abi.lib.ppea_pwconv_stats_partials(c.B, c.M, c.K, c.HW) == plan["partials"]
    assert served == (plan is not None), plan
    arm = P.arm_of_plan(plan, c.ta, c.epi)
    assert c.arm is None or arm == c.arm, (arm, c.arm)
    assert all(t.dtype == (F32 if k == "sums" else BF16) for k, t in got.items())
    ref = P.pw_reference(c, inp, got["y"])
    _hold(c.name, arm, got, ref, bufs)
    if c.epi == 4:
        assert got["sums"].shape[1] == plan["partials"] and bool(torch.isfinite(got["sums"]).all()), arm
        r1, r2, outside = P.stats_check(got["y"], got["sums"], plan["WN"])
        print(f"PWARM {arm} | {c.name} statistics: sum {r1:.3f} squares {r2:.3f} of the bound")
        assert outside == 0, (arm, r1, r2)


def _infer_row(device, monkeypatch, c):
    from ppeadepth import ops
    inp = _to(P.make_pw_inputs(c), device)
    with _hooks(monkeypatch, c.env):
        plan = ops.pwconv_plan(c.B, c.M, c.K, c.HW, False)
        out = L.launch_infer(ops, inp)
        torch.cuda.synchronize()
    arm = P.arm_of_plan(plan, False, 5)
    assert out is not None and arm == c.arm, (arm, c.arm)
    y, y2 = out
    acc, _ = P._acc_and_mag(inp)
    ref, ref2 = P.infer_reference(acc, inp["s"], inp["o"], inp["act"], inp["r1"], inp["r2"], inp["r2_scale"], inp["s2"], inp["o2"])
    assert y.dtype == BF16 and y2.dtype == BF16 and tuple(y.shape) == tuple(ref.shape) == tuple(y2.shape)
    e, e2 = float((y.double() - ref).abs().max() / ref.abs().max()), float((y2.double() - ref2).abs().max() / ref2.abs().max())
    print(f"PWARM {arm} | {c.name}: Y {e:.3e} Y2 {e2:.3e} of the maximum (bound {P.INFER_TOL:.3e})")
    assert e <= P.INFER_TOL and e2 <= P.INFER_TOL, (arm, e, e2)
    again = (inp["s2"].double().view(1, -1, 1, 1) * y.double() + inp["o2"].double().view(1, -1, 1, 1)).float().bfloat16()
    assert (y2.float() - again.float()).abs().max() <= 2 ** -7 * again.float().abs().max(), arm


def _run_pw(device, monkeypatch, c):
    (_infer_row if c.epi == 5 else _pw_row)(device, monkeypatch, c)


def test_device_float64_reference_equals_the_hosts(device):
    c = next(r for r in P.EDGE_CASES if r.name == "v2_gelu_m65")
    inp = P.make_pw_inputs(c)
    host, dev = P.pw_reference(c, inp), P.pw_reference(c, _to(inp, device))
    assert float((host["y"][0] - dev["y"][0].cpu()).abs().max()) <= 1e-12 * float(host["y"][0].abs().max())
    ci = P.INTO_CASES[4]
    ii = P.make_into_inputs(ci)
    host, dev = P.into_reference(ci, ii), P.into_reference(ci, _to(ii, device))
    for key in host:
        assert float((host[key][0] - dev[key][0].cpu()).abs().max()) <= 1e-12 * float(host[key][0].abs().max())


FWD_TILES = [c for c in P.TILE_CASES if c.epi == 0]
EPILOGUES = [c for c in P.TILE_CASES if c.epi != 0]


@pytest.mark.parametrize("c", FWD_TILES, ids=_ids(FWD_TILES))
def test_forward_tile_rows(device, monkeypatch, c):
    """Every (version, A mode, BM, BK) with the plain epilogue: natural rows at the smallest shapes the dispatch picks the tile
    for, hook rows on one small ragged shape."""
    _run_pw(device, monkeypatch, c)


@pytest.mark.parametrize("c", EPILOGUES, ids=_ids(EPILOGUES))
def test_epilogue_rows(device, monkeypatch, c):
    """Every tile x EPI 1 (pre and GELU of the stored pre), 2 (GELU'(aux), aux out to +-6), 4 (statistics partials, P as the plan
    says) and 5 (the inference table through ops.pwconv_table)."""
    _run_pw(device, monkeypatch, c)


@pytest.mark.parametrize("c", P.EDGE_CASES, ids=_ids(P.EDGE_CASES))
def test_edge_rows(device, monkeypatch, c):
    """Per family: M of one row / below a fragment / a last tile of one row, HW 8 / 136 / % 128 in {8, 64, 120}, K of 1-4 steps
    and the zero-filled half step, tile totals 1, 7, 9, 75, 130 (the XCD remap), every bias form."""
    _run_pw(device, monkeypatch, c)


@pytest.mark.parametrize("c", P.UNSUPPORTED_PW, ids=_ids(P.UNSUPPORTED_PW))
def test_unsupported_pwconv_shapes_are_refused_and_nothing_is_written(device, c):
    from ppeadepth import ops
    g = torch.Generator().manual_seed(3)
    inp = dict(x=torch.randn(c.B, c.K, 1, c.HW, generator=g).bfloat16().to(device), bias=None, aux=None)
    inp["a_arg"] = torch.randn((c.K, c.M) if c.ta else (c.M, c.K), generator=g).bfloat16().to(device)
    assert ops.pwconv_plan(c.B, c.M, c.K, c.HW, c.ta) is None
    for epi in ((0, 1) if c.ta else (0, 1, 4)):
        served, got, bufs = L.launch_pw(ops, c._replace(epi=epi), inp, None)
        torch.cuda.synchronize()
        assert not served
        assert all(bool(torch.isnan(t).all()) for t in got.values()) and all(P.guards_intact(b, dt) for b, dt in bufs)
    if not c.ta:
        assert ops.pwconv_table(inp["x"], inp["a_arg"], None) is None


# ---------------------------------------------------------------------------------------------
# pwgrad
# ---------------------------------------------------------------------------------------------
def _pwgrad_arm(p):
    return f"{'pwgrad2_kernel<32>' if p['step'] else 'pwgrad_kernel'} S={p['S']} x{p['steps_per_split']} tiles {p['tiles_m']}x{p['tiles_n']}"


@pytest.mark.parametrize("c", P.PWGRAD_CASES, ids=_ids(P.PWGRAD_CASES))
def test_pwgrad_rows(device, monkeypatch, c):
    """ppea_pwgrad_bf16 (pwgrad_kernel / pwgrad2_kernel<32> + pwgrad_reduce_ex_kernel, fp32, taps = 1): C and the row sums; with the row sums off
    the tail of `out` stays untouched; a second launch is bit-identical."""
    from ppeadepth import ops
    inp = _to(P.make_pwgrad_inputs(c), device)
    M, N, HW = c.M, c.N, c.H * c.W
    runs = []
    with _hooks(monkeypatch, c.env):
        p = ops.pwgrad_plan(c.B, M, N, HW)
        for _ in range(2):
            served, o, bufs = L.launch_pwgrad(ops, c, inp, device, p)
            torch.cuda.synchronize()
            runs.append((served, o["out"], bufs))
    arm = _pwgrad_arm(p)
    served, out, bufs = runs[0]
    assert served and p["step"] == c.claims["step"], arm
    ref = P.pwgrad_reference(inp["p"], inp["q"])
    got = dict(w=out[:M * N].view(M, N))
    if c.rowsum:
        got["rowsum"] = out[M * N:]
    else:
        ref.pop("rowsum")
        assert bool(torch.isnan(out[M * N:]).all()), f"{c.name} ({arm}): the row-sum tail was written with the row sums off"
    _hold(c.name, arm, got, ref, bufs)
    assert torch.equal(_bits(runs[1][1]), _bits(out)), f"{c.name} ({arm}): the second launch differs"
    # through the operator as well
    with _hooks(monkeypatch, c.env):
        w2, r2 = ops.pwgrad(inp["p"], inp["q"], c.rowsum)
        torch.cuda.synchronize()
    assert torch.equal(w2, got["w"]) and (r2 is None) == (not c.rowsum) and (r2 is None or torch.equal(r2, got["rowsum"]))


def _into_row(device, monkeypatch, c, env, tag):
    from ppeadepth import ops
    inp = _to(P.make_into_inputs(c), device)
    with _hooks(monkeypatch, env):
        p = ops.pwgrad_plan(c.B, c.taps * c.Ch, c.N, c.H * c.W)
        served, got, bufs = L.launch_into(ops, c, inp, device, p)
        torch.cuda.synchronize()
        served2, again, _ = L.launch_into(ops, c, inp, device, p)
        dw_op, db_op = ops.pwgrad_into(*L.op_args(c, inp))
        torch.cuda.synchronize()
    arm = _pwgrad_arm(p) + f" reduce_ex taps {c.taps}"
    assert served and served2, arm
    _hold(tag, arm, got, P.into_reference(c, inp), bufs)
    for key in got:
        assert torch.equal(_bits(got[key]), _bits(again[key])), f"{tag} {key} ({arm}): the second launch differs"
    assert torch.equal(dw_op, got["dw"]) and (db_op is None) == (c.bdt is None) and (db_op is None or torch.equal(db_op, got["db"]))
    return inp, got


@pytest.mark.parametrize("c", P.INTO_CASES, ids=_ids(P.INTO_CASES))
def test_pwgrad_into_rows(device, monkeypatch, c):
    """ppea_pwgrad_ex_bf16 (pwgrad_reduce_ex_kernel): the weight as fp32 / bf16, [M][N] or the taps = 9 scatter into Conv2d layout
    against the weight gradient of a float64 F.conv2d(padding=1), the bias window as fp32 / bf16 / none."""
    _into_row(device, monkeypatch, c, c.env, c.name)


@pytest.mark.parametrize("row", P.PAIR_CASES, ids=[r[0] for r in P.PAIR_CASES])
def test_pwgrad_pair_rows(device, monkeypatch, row):
    """ppea_pwgrad_ex_pair_bf16 (pwgrad2_pair_kernel<32> + pwgrad_reduce_ex2_kernel): both problems held to the float64 reference
    independently; where the pair form is not served it is refused, writes nothing, and ops.pwgrad_into_pair's two single
    launches are held to the same bounds."""
    from ppeadepth import ops
    name, a, b, env, claimed = row
    Ms, Ns, HW = (a.taps * a.Ch, b.taps * b.Ch), (a.N, b.N), a.H * a.W
    inps = [_to(P.make_into_inputs(c), device) for c in (a, b)]
    refs = [P.into_reference(c, i) for c, i in zip((a, b), inps)]

    def launch(plan):
        served, outs, bufs = L.launch_pair(ops, a, b, inps, device, plan)
        torch.cuda.synchronize()
        return served, outs, bufs

    with _hooks(monkeypatch, env):
        plan = ops.pwgrad_pair_plan(a.B, Ms, Ns, HW)
        served, outs, bufs = launch(plan)
        served2, again, _ = launch(plan)
        (dwa, dba), (dwb, dbb) = ops.pwgrad_into_pair(L.op_args(a, inps[0]), L.op_args(b, inps[1]))
        torch.cuda.synchronize()
    assert served == served2 == claimed == (plan is not None), plan
    if served:
        arm = f"pwgrad2_pair_kernel<32> S={plan['S']} x{plan['steps_per_split']} tiles {plan['tiles_m']}+{plan['tiles_n']} reduce_ex2"
        for k, (c, got, ref) in enumerate(zip((a, b), outs, refs)):
            _hold(f"{name} problem {k}", arm, got, ref, bufs)
            for key in got:
                assert torch.equal(_bits(got[key]), _bits(again[k][key])), f"{name} problem {k} {key} ({arm}): the second launch differs"
        assert torch.equal(dwa, outs[0]["dw"]) and torch.equal(dwb, outs[1]["dw"])
        for op_b, o in ((dba, outs[0]), (dbb, outs[1])):
            assert (op_b is None) == ("db" not in o) and (op_b is None or torch.equal(op_b, o["db"]))
    else:
        for o in outs:
            assert all(bool(torch.isnan(t).all()) for t in o.values())
        assert all(P.guards_intact(bf, dt) for bf, dt in bufs) and bool(torch.isnan(bufs[0][0][P.GUARD:-P.GUARD].view(F32)).all())
        # the fall-back: two single launches, each into guarded buffers, held to the same bounds
        for k, c in enumerate((a, b)):
            _inp, got = _into_row(device, monkeypatch, c, env, f"{name} problem {k}")
            assert torch.equal((dwa, dwb)[k], got["dw"])
            assert ((dba, dbb)[k] is None) == ("db" not in got) and ((dba, dbb)[k] is None or torch.equal((dba, dbb)[k], got["db"]))


# ---------------------------------------------------------------------------------------------
# tapsum
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.TAPSUM_CASES, ids=_ids(P.TAPSUM_CASES))
def test_tapsum_rows(device, c):
    """ppea_tapsum_fwd_bf16 (the shifted sum in double; h = GELU of the stored pre) and ppea_tapsum_bwd_bf16 (bit equality with
    the gather) down to W = 4, H = 1, Ch = 1, with every bias form."""
    from ppeadepth import ops
    inp = _to(P.make_tapsum_inputs(c), device)
    served, got, bufs = L.launch_tapsum(ops, c, inp, device)
    assert served
    torch.cuda.synchronize()
    pre, h, dT = got["pre"], got["h"], got["dT"]
    _hold(c.name, "tapsum", got, P.tapsum_reference(c, inp, pre), bufs)
    assert torch.equal(dT, P.shift_taps(inp["g"]))
    pre_op, h_op = ops.tapsum_fwd(inp["T"], inp["bias"], c.Ch)
    assert torch.equal(pre_op, pre) and torch.equal(h_op, h) and torch.equal(ops.tapsum_bwd(inp["g"]), dT)


def test_tapsum_refuses_a_width_that_is_no_multiple_of_four(device):
    from ppeadepth import ops
    B, Ch, H, W = 2, 3, 4, 6
    T = torch.randn(B, 9 * Ch, H, W).bfloat16().to(device)
    g = torch.randn(B, Ch, H, W).bfloat16().to(device)
    pbuf, pre = P.guarded((B, Ch, H, W), BF16, device)
    hbuf, h = P.guarded((B, Ch, H, W), BF16, device)
    tbuf, dT = P.guarded((B, 9 * Ch, H, W), BF16, device)
    assert not ops.try_call("ppea_tapsum_fwd_bf16", ops.ptr(T), None, 0, ops.ptr(pre), ops.ptr(h), B, Ch, H, W, ops.stream_ptr())
    assert not ops.try_call("ppea_tapsum_bwd_bf16", ops.ptr(g), ops.ptr(dT), B, Ch, H, W, ops.stream_ptr())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (pre, h, dT)) and all(P.guards_intact(b, BF16) for b in (pbuf, hbuf, tbuf))
