"""Every reachable instantiation and host-plan outcome of the large-kernel depthwise kernels (csrc/dwconv_mfma.hip: row-band,
window-sharing and batch-major; csrc/dwconv_wgrad.hip; csrc/dwconv_lk.hip) against the float64 reference of
oracle/dwconv_inputs.py, element by element, each element held to the bound derived there.  Outputs are NaN-filled views into
guarded buffers: an element never stored is outside its bound, a store past either end changes a guard.  Every row asserts that
the entry point served it exactly when the library's plan names a kernel family for it (tests/test_dwconv_arms_cpu.py proves
that the plan names the arm the row is there for, the reference, the bound, and that the bound catches index faults).
The float64 reference runs F.conv2d in double on the device (checked against the host's once); no PPEA_DW_* switch is set."""
import pytest
import torch

from conftest import rel_err
from oracle import bn_inputs as B
from oracle import dwconv_inputs as D

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
STAT_TOL, RVAR_TOL = 1e-5, 1e-4             # oracle/bn_inputs.py's fp32 figures for statistics (tests/test_bn_arms_gpu.py)
PLAIN_ROWS = [r for r in D.ROWBAND_CASES + D.WS_CASES + D.BM_CASES if r.variant == "plain"]
STATS_ROWS = [r for r in D.mfma_rows() if r.variant == "stats"]
BN_ROWS = [r for r in D.VARIANT_CASES if r.variant == "bn"]
BA_ROWS = [r for r in D.VARIANT_CASES if r.variant == "bias_act"]


def _ids(rows):
    return [r.name for r in rows]


def _plan(ops, r, variant=None):
    return ops.dwconv_lk_plan(r.N, r.C, r.H, r.W, r.K, r.KS, r.mode, variant or r.variant)


def _family(r):
    return {"rb": "window-sharing" if r.arm[6] else "row-band", "bm": "batch-major"}[r.arm[0]]


def _hold(tag, family, got, ref, bufs):
    """Every output element inside its bound, every guard intact; prints the worst ratio per output."""
    for key, (ref_t, bound) in ref.items():
        g = got[key]
        assert tuple(g.shape) == tuple(ref_t.shape), (tag, key)
        ratio, outside = D.worst(g, ref_t, bound)
        print(f"DWARM {family} | {tag} {key}: worst err / bound {ratio:.3f}")
        assert outside == 0, f"{tag} {key} ({family}): worst err / bound {ratio:.3f}, {outside} of {ref_t.numel()} elements outside"
    for buf, dtype in bufs:
        assert D.guards_intact(buf, dtype), f"{tag}: a guard element was overwritten"


def _launch(ops, r, inp, device, variant=None, x=None, bn=None):
    """One row through its entry point into guarded outputs -> (served, outputs, guarded buffers, sums or None)."""
    variant = variant or r.variant
    N, C, H, W, K, KS = r.N, r.C, r.H, r.W, r.K, r.KS
    shape, st = (N, C, H, W), ops.stream_ptr()
    ptr = ops.ptr
    flip = r.mode == 1
    pb = ops.pack_dwconv_filter(inp["wb"].to(device), flip)
    ps = ops.pack_dwconv_filter(inp["ws"].to(device), flip) if KS else None
    bufs, sums = [], None
    if r.mode == 1:
        gb, gs = inp["gb"].to(device), inp["gs"].to(device) if KS else None
        buf, dx = D.guarded(shape, BF16, device)
        bufs.append((buf, BF16))
        served = ops.try_call("ppea_dwconv_lk_bwd_data_bf16p", ptr(gb), ptr(gs), ptr(pb), ptr(ps), ptr(dx), N, C, H, W, K, KS, st)
        return served, dict(dx=dx), bufs, None
    xd = (inp["x"] if x is None else x).to(device)
    buf, yb = D.guarded(shape, BF16, device)
    bufs.append((buf, BF16))
    out = dict(y_big=yb)
    ys = None
    if KS:
        buf, ys = D.guarded(shape, BF16, device)
        bufs.append((buf, BF16))
        out["y_small"] = ys
    if variant == "plain":
        served = ops.try_call("ppea_dwconv_lk_fwd_bf16p", ptr(xd), ptr(pb), ptr(ps), ptr(yb), ptr(ys), N, C, H, W, K, KS, st)
    elif variant == "stats":
        P = _plan(ops, r, "stats")["partials"]
        buf, sums = D.guarded((2, C, max(P, 1), 2), F32, device)
        bufs.append((buf, F32))
        served = ops.try_call("ppea_dwconv_lk_fwd_stats_bf16p", ptr(xd), ptr(pb), ptr(ps), ptr(yb), ptr(ys), ptr(sums), N, C, H, W,
                              K, KS, st)
    elif variant == "bias_act":
        bias = inp["bias"].to(device)
        served = ops.try_call("ppea_dwconv_lk_fwd_bias_act_bf16p", ptr(xd), ptr(pb), ptr(bias), int(r.relu), ptr(yb), N, C, H, W, K, st)
    else:
        served = ops.try_call(
            "ppea_dwconv_lk_fwd_bn_bf16p", ptr(xd), ptr(pb), ptr(ps), ptr(yb), ptr(ys), ptr(bn["sums"], F32), bn["sums"].shape[1],
            N * H * W, ptr(bn["gamma"]), ptr(bn["beta"]), float(B.EPS), float(B.MOMENTUM), ptr(bn["rm"]), ptr(bn["rv"]),
            ptr(bn["mean"]), ptr(bn["invstd"]), N, C, H, W, K, 5, st)
    return served, out, bufs, sums


def test_device_float64_reference_equals_the_hosts(device):
    r = D._r("probe", (3, 5, 9, 21), 13, 5, 0)
    inp = D.make_inputs(r)
    for mode in (0, 1):
        rr = r._replace(mode=mode)
        host, dev = D.reference(rr, inp), D.reference(rr, inp, device=device)
        for key in host:
            for a, b in zip(host[key], dev[key]):
                assert float((a - b.cpu()).abs().max()) <= 1e-12 * float(a.abs().max())
    fh, fd = D.reference_filter(r, inp), D.reference_filter(r, inp, device=device)
    for key in fh:
        assert float((fh[key][0] - fd[key][0].cpu()).abs().max()) <= 1e-12 * float(fh[key][0].abs().max())


@pytest.mark.parametrize("r", PLAIN_ROWS, ids=_ids(PLAIN_ROWS))
def test_forward_and_data_gradient_rows(device, r):
    """Row-band (every K x KS x mode x NSEG, every band / stacking / staging / items-per-wave outcome), window sharing and
    batch-major (every (K, H, NTX) in both modes, the 48-row data gradient) through ppea_dwconv_lk_fwd_bf16p /
    ppea_dwconv_lk_bwd_data_bf16p."""
    from ppeadepth import ops
    inp = D.make_inputs(r)
    p = _plan(ops, r)
    served, got, bufs, _ = _launch(ops, r, inp, device)
    torch.cuda.synchronize()
    assert served == (p["family"] != 0) and D.arm_of_plan(p, r.K, r.KS, r.mode) == r.arm, p
    if r.arm is None:                                   # refused: nothing was written
        for t in got.values():
            assert bool(torch.isnan(t).all())
        assert all(D.guards_intact(b, dt) for b, dt in bufs)
        return
    _hold(r.name, _family(r), got, D.reference(r, inp, device=device), bufs)


@pytest.mark.parametrize("r", STATS_ROWS, ids=_ids(STATS_ROWS))
def test_epilogue_statistics_rows(device, r):
    """ppea_dwconv_lk_fwd_stats_bf16p: the outputs as above; the partials [2][C][P][2], P as the plan says, summed over P in
    double against double sums of the device's own stored y within m * 2^-23 * sum |y| (squares: sum y^2), m = the most
    elements one partial adds up."""
    from ppeadepth import _abi, ops
    inp = D.make_inputs(r)
    p = _plan(ops, r)
    assert p["partials"] == _abi.lib.ppea_dwconv_lk_stats_partials(r.N, r.C, r.H, r.W, r.K, r.KS) > 0
    served, got, bufs, sums = _launch(ops, r, inp, device)
    torch.cuda.synchronize()
    assert served and sums.shape[2] == p["partials"]
    _hold(r.name, _family(r), got, D.reference(r, inp, device=device), bufs)
    if p["family"] == 1:
        m = p["ipw"] * (p["G"] * r.H if p["G"] > 1 else min(p["band"], r.H)) * min(r.W, 16 * p["NSEG"])
    else:
        m = p["NY"] * min(p["gi"], r.N) * min(r.W, 16 * p["cpw"])
    assert bool(torch.isfinite(sums).all())
    for i, key in enumerate(("y_big", "y_small")):
        y = got[key].double()
        s, q = sums[i, :, :, 0].double().sum(1), sums[i, :, :, 1].double().sum(1)
        ws_, wq = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
        bs, bq = m * D.U_ACC * y.abs().sum((0, 2, 3)), m * D.U_ACC * wq
        rs, rq = float(((s - ws_).abs() / bs).max()), float(((q - wq).abs() / bq).max())
        print(f"DWARM statistics | {r.name} {key}: sum {rs:.3f} squares {rq:.3f} of the bound (m = {m})")
        assert bool(((s - ws_).abs() <= bs).all()) and bool(((q - wq).abs() <= bq).all()), (key, rs, rq)


@pytest.mark.parametrize("r", BN_ROWS, ids=_ids(BN_ROWS))
def test_fused_input_batchnorm_rows(device, r):
    """ppea_dwconv_lk_fwd_bn_bf16p equals, bit for bit, the plain launch of the same plan fed relu(BN(z)) from the separate
    BatchNorm kernels (the method of test_dwconv_fused_input_batchnorm_relu_equals_the_separate_launches); the plain launch is
    the one held to float64; mean, invstd and the running statistics against a float64 BatchNorm."""
    from ppeadepth import ops
    inp = D.make_inputs(r)
    N, C = r.N, r.C
    p, pp = _plan(ops, r), _plan(ops, r, "plain")
    assert p["BN"] == 1 and {k: v for k, v in p.items() if k != "BN"} == {k: v for k, v in pp.items() if k != "BN"}
    z = inp["x"].to(device)
    P = min(N, 3)                                       # the producer's partial sums: per chunk of images, fp32
    chunks = torch.chunk(z.double(), P, 0)
    assert len(chunks) == P
    sums = torch.stack([torch.stack([c.sum((0, 2, 3)), (c * c).sum((0, 2, 3))], -1) for c in chunks], 1).float().contiguous()
    gamma, beta = inp["gamma"].to(device), inp["beta"].to(device)
    res = {}
    for fused in (False, True):
        rm, rv = torch.zeros(C, device=device), torch.ones(C, device=device)
        if fused:
            bn = dict(sums=sums, gamma=gamma, beta=beta, rm=rm, rv=rv, mean=torch.empty(C, device=device),
                      invstd=torch.empty(C, device=device))
            served, got, bufs, _ = _launch(ops, r, inp, device, bn=bn)
            mean, invstd = bn["mean"], bn["invstd"]
        else:
            mean, _var, invstd = ops.bn_batch_stats_from_sums(sums, N * r.H * r.W, B.EPS, B.MOMENTUM, rm, rv)
            with torch.no_grad():
                t = ops.bn_act_apply(z, gamma, beta, mean, invstd, act=ops.ACT_RELU)
            served, got, bufs, _ = _launch(ops, r, inp, device, variant="plain", x=t)
            torch.cuda.synchronize()
            _hold(r.name, _family(r), got, D.reference(r, inp, x=t, device=device), bufs)
        torch.cuda.synchronize()
        assert served and all(D.guards_intact(b, dt) for b, dt in bufs)
        res[fused] = dict(got, mean=mean.clone(), invstd=invstd.clone(), running_mean=rm, running_var=rv)
    for key in res[True]:
        assert torch.equal(res[True][key], res[False][key]), key
    _, st, _ = B._bn64(z.double().cpu(), gamma.double().cpu(), beta.double().cpu(), torch.zeros(C).double(), torch.ones(C).double())
    for key, tol in (("mean", STAT_TOL), ("invstd", STAT_TOL), ("running_mean", STAT_TOL), ("running_var", RVAR_TOL)):
        err = rel_err(res[True][key].cpu(), st[key])
        print(f"DWARM fused-bn | {r.name} {key}: {err:.3e} (bound {tol:.0e})")
        assert err < tol, key


@pytest.mark.parametrize("r", BA_ROWS, ids=_ids(BA_ROWS))
def test_bias_activation_rows(device, r):
    """ppea_dwconv_lk_fwd_bias_act_bf16p: every K x NSEG, ReLU on and off."""
    from ppeadepth import ops
    inp = D.make_inputs(r)
    p = _plan(ops, r)
    served, got, bufs, _ = _launch(ops, r, inp, device)
    torch.cuda.synchronize()
    assert served and p["BA"] == 1 and D.arm_of_plan(p, r.K, r.KS, r.mode) == r.arm
    ref = D.reference(r, inp, device=device)
    if r.relu:
        assert 0.05 < float((ref["y_big"][0] == 0).double().mean()) < 0.95         # the ReLU cuts, and not everything
    _hold(r.name, "bias-act", got, ref, bufs)


@pytest.mark.parametrize("row", D.FILTER_CASES, ids=[r.name for r, _ in D.FILTER_CASES])
def test_filter_gradient_rows(device, row):
    """ops.dwconv_lk_bwd_filter at the shapes the plan says reach a ragged last part, a short last round, N * H < 4 and
    W % 8 != 0 / W % 16 != 0: both gradients, fp32, within N*H*W * 2^-23 * A of the float64 one."""
    from ppeadepth import ops
    r, _ = row
    inp = D.make_inputs(r)
    got = ops.dwconv_lk_bwd_filter(inp["x"].to(device), inp["gb"].to(device), inp["gs"].to(device) if r.KS else None, r.K)
    torch.cuda.synchronize()
    assert got is not None and ops.dwconv_lk_bwd_filter_plan(r.N, r.C, r.H, r.W, r.K, r.KS) is not None
    named = dict(dw_big=got[0], **(dict(dw_small=got[1]) if r.KS else {}))
    _hold(r.name, "filter-gradient", named, D.reference_filter(r, inp, device=device), [])


@pytest.mark.parametrize("fr", D.F32_CASES, ids=[fr.row.name for fr in D.F32_CASES])
def test_fp32_vector_kernel_rows(device, fr):
    """ppea_dwconv_lk_{fwd,bwd_data}_{f32,bf16}: every tile of CFGS_<K> that can be picked, and the generic kernel."""
    from ppeadepth import ops
    r = fr.row
    N, C, H, W, K, KS = r.N, r.C, r.H, r.W, r.K, r.KS
    assert (ops.dwconv_lk_f32_plan(H, W, K) if KS in (0, 5) else -1) == fr.index
    inp = D.make_inputs(r)
    dt = F32 if fr.io == "f32" else BF16
    wb, ws = inp["wb"].to(device), inp["ws"].to(device) if KS else None
    ptr, st = ops.ptr, ops.stream_ptr()
    buf, o0 = D.guarded((N, C, H, W), dt, device)
    bufs = [(buf, dt)]
    if r.mode == 0:
        x = inp["x"].to(device).to(dt)
        o1 = None
        if KS:
            buf, o1 = D.guarded((N, C, H, W), dt, device)
            bufs.append((buf, dt))
        ops.call(f"ppea_dwconv_lk_fwd_{fr.io}", ptr(x), ptr(wb), ptr(ws), ptr(o0), ptr(o1), N, C, H, W, K, KS, st)
        got = dict(y_big=o0, **(dict(y_small=o1) if KS else {}))
    else:
        gb, gs = inp["gb"].to(device).to(dt), inp["gs"].to(device).to(dt) if KS else None
        ops.call(f"ppea_dwconv_lk_bwd_data_{fr.io}", ptr(gb), ptr(gs), ptr(wb), ptr(ws), ptr(o0), N, C, H, W, K, KS, st)
        got = dict(dx=o0)
    torch.cuda.synchronize()
    _hold(r.name, "fp32-vector", got, D.reference_f32(fr, inp, device=device), bufs)
