"""What tests/test_glue_arms_gpu.py relies on, proved without a device: every stencil row of oracle/glue_inputs.py reaches the
arm it names according to the library's own query (ops.dwconv3x3_plan, the function both launchers switch on) and the named
arms are the whole census; the restated part / slab / chunk plans equal the library's queries on every row and over a sweep of
small shapes, and every plan outcome the rows are there for is claimed; the float64 references equal torch's own ops in double
(autograd where there is a gradient); a plain fp32 emulation of each kernel's arithmetic, stored into guarded buffers, stays
inside every bound on every row; planted faults do not -- each puts an element outside its bound or breaks a guard on the row
that claims to catch it; E_ELU is what the CPU measures."""
import pytest
import torch
import torch.nn.functional as F

from oracle import glue_inputs as G

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
WORST = {}


def _ids(rows):
    return [r.name for r in rows]


def _place(outs):
    """The emulation's outputs stored into NaN-filled views of guarded buffers, as the launchers hand them to the kernels."""
    got, bufs = {}, []
    for k, t in outs.items():
        if t.dtype == torch.float64:                         # a float64 sum made on the test side, not a kernel's store
            got[k] = t
            continue
        buf, view = G.guarded_u8(tuple(t.shape), "cpu") if t.dtype == U8 else G.guarded(tuple(t.shape), t.dtype, "cpu")
        G.bits(view).copy_(G.bits(t).view(view.shape))
        got[k] = view
        bufs.append((buf, t.dtype))
    return got, bufs


def _outside(got, ref):
    """-> (worst ratio, elements outside) over the outputs `ref` names."""
    ratio, out = 0.0, 0
    for k, (r, b) in ref.items():
        assert tuple(got[k].shape) == tuple(r.shape), k
        w, o = G.check(got[k], r, b)
        ratio, out = max(ratio, w), out + o
    return ratio, out


def _hold(family, tag, outs, ref):
    got, bufs = _place(outs)
    ratio, out = _outside(got, ref)
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"GLUE-CPU {family} | {tag}: worst err / bound of the emulation {ratio:.3f} (so far {WORST[family]:.3f})")
    assert out == 0, (family, tag, ratio, out)
    assert all(G.guards_ok(b, dt) for b, dt in bufs)


def _caught(outs, ref):
    got, bufs = _place(outs)
    return _outside(got, ref)[1] > 0 or not all(G.guards_ok(b, dt) for b, dt in bufs)


def _row(rows, name):
    return next(r for r in rows if r.name == name)


# ---------------------------------------------------------------------------------------------
# census and plans
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.DW_CASES, ids=_ids(G.DW_CASES))
def test_every_stencil_row_reaches_the_arm_it_names(c):
    from ppeadepth import ops
    dt = G.dt_of(c.dt)
    args = (c.N, c.C, c.H, c.W, c.stride)
    assert ops.dwconv3x3_plan(dt, "forward", *args) == c.arm_fwd, c.why
    assert ops.dwconv3x3_plan(dt, "affine_forward", *args) == c.arm_fwd, c.why
    assert ops.dwconv3x3_plan(dt, "data_gradient", *args) == c.arm_bwd, c.why
    Ho, Wo = G.out_hw(c.H, c.W, c.stride)
    if c.name.startswith("130x127"):                         # the data gradient's loop, and at stride 1 the forward's
        assert c.H * c.W > 64 * 256 and (c.stride == 2 or Ho * Wo > 64 * 256)
    if c.name.startswith("259x255"):
        assert Ho * Wo > 64 * 256


def test_the_named_stencil_arms_are_the_census():
    from ppeadepth import _abi, ops
    assert len(ops.DWCONV3X3_ARMS) == len(G.ALL_DW3_ARMS) and len(ops.DWCONV3X3_MODES) == 3
    fwd = {(c.dt, c.stride, c.arm_fwd) for c in G.DW_CASES}
    bwd = {(c.dt, c.stride, c.arm_bwd) for c in G.DW_CASES}
    assert {a for _, _, a in fwd | bwd} == G.ALL_DW3_ARMS | {None}
    # what each (dtype, stride) can reach, forward / affine and data gradient
    for s in (1, 2):
        assert {a for d, st, a in fwd if (d, st) == ("f32", s)} == {G.GENERIC, None} == {a for d, st, a in bwd if (d, st) == ("f32", s)}
    assert {a for d, st, a in fwd if (d, st) == ("bf16", 1)} == {G.GENERIC, G.V_S1, None} == {a for d, st, a in bwd if (d, st) == ("bf16", 1)}
    assert {a for d, st, a in fwd if (d, st) == ("bf16", 2)} == {G.GENERIC, G.V_S2_FWD, None}
    assert {a for d, st, a in bwd if (d, st) == ("bf16", 2)} == {G.GENERIC, G.V_S2_BWD, None}
    # the query over a sweep: no other value, fp32 never on a vector arm, the affine forward goes where the forward goes and the
    # data gradient differs from it only in the stride-2 vector pair
    plan = _abi.lib.ppea_dwconv3x3_plan
    seen = set()
    for eb in (2, 4):
        for s in (0, 1, 2, 3):
            for H in range(0, 9):
                for W in range(0, 50):
                    f, b, a = (plan(eb, m, 2, 3, H, W, s) for m in (0, 1, 2))
                    assert f == a and (b == f or (f, b) == (G.V_S2_FWD, G.V_S2_BWD)), (eb, s, H, W, f, b, a)
                    assert f in (G.GENERIC, G.ERR_UNSUPPORTED) if eb == 4 else f in (-1, 0, 1, 2)
                    assert (f == G.ERR_UNSUPPORTED) == (s not in (1, 2) or H == 0 or W == 0)
                    seen.add(f)
    assert seen == {-1, 0, 1, 2}
    assert plan(2, 0, 255, 257, 4, 8, 1) == G.V_S1 and plan(2, 0, 256, 256, 4, 8, 1) == -1          # 65535 planes, 65536
    assert plan(3, 0, 2, 3, 4, 8, 1) == -1 and plan(2, 3, 2, 3, 4, 8, 1) == -1 and plan(2, -1, 2, 3, 4, 8, 1) == -1
    assert ops.dwconv3x3_plan(BF16, 0, 2, 3, 4, 8, 3) is None


@pytest.mark.parametrize("c", G.WG_CASES, ids=_ids(G.WG_CASES))
def test_filter_gradient_rows_get_the_plan_they_claim(c):
    from ppeadepth import _abi
    p = G.wgrad_plan(c.N, c.H, c.W, c.stride)
    nbytes = _abi.lib.ppea_dwconv3x3_bwd_filter_workspace_bytes(c.N, c.C, c.H, c.W, c.stride)
    assert nbytes == G.wgrad_workspace_bytes(c.N, c.C, c.H, c.W, c.stride) == c.C * p["parts"] * 36
    Ho, Wo = G.out_hw(c.H, c.W, c.stride)
    cl = c.claims
    assert p["parts"] == cl["parts"], p
    assert bool(cl.get("ragged")) == (p["parts"] > 1 and p["rows"] % p["rows_per_part"] != 0) or cl.get("cap"), p
    assert not cl.get("idle_waves") or p["rows"] < 4
    assert not cl.get("lane_loop") or Wo > 64
    assert not cl.get("clamp") or (p["want"] > p["rows"] and p["parts"] == p["rows"])
    assert not cl.get("cap") or (p["want"] > 64 and c.N * Ho * Wo > 64 * 8192 and c.C == 1)
    if c.ints:
        assert 4 * c.N * Ho * Wo < 2 ** 24


def test_restated_plans_equal_the_library_over_a_sweep():
    from ppeadepth import _abi
    lib = _abi.lib
    for s in (1, 2, 3):
        for N in (1, 2, 5):
            for H in (1, 2, 3, 7, 64, 129):
                for W in (1, 5, 64, 65, 200, 4097, 9000):
                    assert lib.ppea_dwconv3x3_bwd_filter_workspace_bytes(N, 3, H, W, s) == G.wgrad_workspace_bytes(N, 3, H, W, s)
    for shape in G.WG_UNSUPPORTED:
        assert lib.ppea_dwconv3x3_bwd_filter_workspace_bytes(*shape) == G.ERR_UNSUPPORTED == G.wgrad_workspace_bytes(*shape)
    for C in (8, 16, 24, 32, 40, 64, 128, 256, 512, 1024, 2048, 4096, 4104):
        for P in list(range(1, 70)) + [255, 256, 257, 2048, 2049, 8191, 8192, 8193, 8200, 262144, 262145, 300000]:
            p = G.slab_plan(P, C)
            assert lib.ppea_nhwc_bias_elu_slabs(P, C) == (G.ERR_UNSUPPORTED if p is None else p["slabs"]), (P, C)
            assert p is None or (p["slabs"] <= 1024 and (p["slabs"] - 1) * p["rows"] < P <= p["slabs"] * p["rows"])
    for C in G.BE_UNSUPPORTED_C:
        assert lib.ppea_nhwc_bias_elu_slabs(64, C) == G.ERR_UNSUPPORTED and G.slab_plan(64, C) is None
    assert lib.ppea_nhwc_bias_elu_slabs(0, 64) == G.ERR_UNSUPPORTED
    for planes in (1, 2, 3, 6, 511, 512, 513, 1024, 2047, 2048, 5000):
        for HW in (1, 5, 63, 64, 2047, 4095, 4096, 4104, 4221, 8191, 8192, 8200, 16384, 100000, 4194312):
            p = G.chunk_plan(planes, HW)
            assert lib.ppea_bias_elu_chunks(planes, 1, HW) == p["chunks"] == lib.ppea_bias_elu_chunks(1, planes, HW), (planes, HW)
            assert p["per"] % 8 == 0 and p["per"] * p["chunks"] >= HW


@pytest.mark.parametrize("c", G.BE_CASES, ids=_ids(G.BE_CASES))
def test_bias_elu_rows_get_the_plan_they_claim(c):
    from ppeadepth import _abi
    p, cl = G.be_plan(c), c.claims
    if c.layout == "nhwc":
        P = c.N * c.HW
        assert _abi.lib.ppea_nhwc_bias_elu_slabs(P, c.C) == p["slabs"] == cl["slabs"] and p["RL"] == cl["RL"], p
        assert bool(cl.get("ragged")) == (p["slabs"] > 1 and P % p["rows"] != 0), p
        assert not cl.get("idle_lanes") or P < p["RL"]
        assert bool(cl.get("cap")) == (p["want"] > 1024)
    else:
        assert _abi.lib.ppea_bias_elu_chunks(c.N, c.C, c.HW) == p["chunks"] == cl["chunks"], p
        assert cl["vector"] == (c.HW % 8 == 0)
        assert bool(cl.get("ragged")) == (p["chunks"] > 1 and c.HW - (p["chunks"] - 1) * p["per"] != p["per"])
    assert G.be_partial_shape(c) == ((p["slabs"], c.C) if c.layout == "nhwc" else (c.N * c.C, p["chunks"]))


def test_every_plan_outcome_is_claimed():
    nhwc = [c for c in G.BE_CASES if c.layout == "nhwc"]
    nchw = [c for c in G.BE_CASES if c.layout == "nchw"]
    for dt in ("f32", "bf16"):
        assert {c.claims["RL"] for c in nhwc if c.dt == dt} == {256, 32, 2, 1}
        assert {c.C for c in nhwc if c.dt == dt} >= {8, 64, 1024, 2048}
        assert any(c.claims["slabs"] == 1 for c in nhwc if c.dt == dt) and any(c.claims.get("ragged") for c in nhwc if c.dt == dt)
        assert any(c.claims.get("idle_lanes") for c in nhwc if c.dt == dt)
        for vec in (True, False):
            assert any(c.claims["vector"] == vec and c.claims["chunks"] == 1 for c in nchw if c.dt == dt)
            assert any(c.claims["vector"] == vec and c.claims["chunks"] > 1 for c in nchw if c.dt == dt)
        assert any(c.N * c.C >= 2048 and c.HW == 1 for c in nchw if c.dt == dt)
        assert {c.bdt for c in G.BE_CASES if c.dt == dt} == {"f32", "bf16"}
        for s in (1, 2):
            wg = [c.claims for c in G.WG_CASES if (c.dt, c.stride) == (dt, s)]
            assert any(k["parts"] == 1 for k in wg) and any(k.get("ragged") for k in wg) and any(k.get("clamp") for k in wg)
            assert any(k.get("idle_waves") for k in wg) and any(k.get("lane_loop") for k in wg)
    assert any(c.claims.get("cap") for c in nhwc if c.dt == "bf16")
    assert {(c.dt, c.stride) for c in G.WG_CASES if c.claims.get("cap") and not c.ints} == {("bf16", 1), ("f32", 2)}
    assert any(c.ints for c in G.WG_CASES)
    for layout in ("nhwc", "nchw"):
        for dt in ("f32", "bf16"):
            fwd = {(c.H, c.W) for c in G.PD_CASES if (c.layout, c.dt, c.bwd) == (layout, dt, False)}
            bwd = {(c.H, c.W) for c in G.PD_CASES if (c.layout, c.dt, c.bwd) == (layout, dt, True)}
            assert {h for h, _ in fwd} >= {2, 3, 4, 7} <= {w for _, w in fwd} and {h for h, _ in bwd} >= {3, 4, 7} <= {w for _, w in bwd}
            assert {(3, 4), (4, 3)} <= bwd
            assert any(c.kind == "bits" for c in G.PD_CASES if (c.layout, c.dt) == (layout, dt))
    assert {c.C for c in G.PD_CASES if c.layout == "nhwc"} == {8, 24, 64}
    for bwd in (False, True):
        assert any(c.layout == "nchw" and c.bwd == bwd and c.B * c.C * (c.H + 2 * (not bwd)) * (c.W + 2 * (not bwd)) > 8192 * 256 for c in G.PD_CASES)
    for dt in ("f32", "bf16"):
        uc = [c for c in G.UC_CASES if c.dt == dt]
        assert any(c.C2 == 0 for c in uc) and any((c.C1, c.C2) == (8, 8) for c in uc) and any((c.C1, c.C2) == (24, 40) for c in uc)
        assert any((c.H, c.W) == (2, 2) for c in uc) and any((c.H // 2) % 2 and (c.W // 2) % 2 for c in uc) and any(c.N >= 2 for c in uc)
        assert any(c.kind == "bits" for c in uc)
        mp = [c for c in G.MP_CASES if c.dt == dt]
        assert {(c.H, c.W) for c in mp} == {(1, 1), (2, 2), (13, 19), (24, 40)} and {c.C for c in mp} == {8, 24}
        assert any(c.kind == "nan" for c in mp)


def test_e_elu_is_four_times_what_the_cpu_measures():
    m = G.measure_e_elu()
    print(f"GLUE-CPU expm1 fp32 against float64 on [-{G.ELU_RANGE:g}, 0): worst |err| {m:.3e}; E_ELU {G.E_ELU:.3e}")
    assert m <= G.E_ELU_MEASURED * 1.001 and G.E_ELU == 4 * G.E_ELU_MEASURED and m >= 0.5 * G.E_ELU_MEASURED
    for c in G.BE_CASES:                                     # the rows' arguments lie inside the measured range
        inp = G.make_be_inputs(c)
        assert float((inp["z"].double() + G._be_bias_view(c, inp["bias"].double())).min()) >= -G.ELU_RANGE


# ---------------------------------------------------------------------------------------------
# the references against torch's own ops in double
# ---------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1.0) if a.numel() else True


@pytest.mark.parametrize("c", [c for c in G.DW_CASES if c.arm_fwd is not None and c.dt == "f32"], ids=lambda c: c.name)
def test_stencil_reference_equals_conv2d_and_its_autograd(c):
    inp = G.make_dw_inputs(c)
    ref = G.dw_reference(c, inp)
    x = inp["x"].double().requires_grad_()
    w = inp["w"].double()
    y = F.conv2d(x, w, stride=c.stride, padding=1, groups=c.C)
    assert _close(ref["fwd"][0], y.detach())
    (dx,) = torch.autograd.grad(y, x, inp["dy"].double())
    assert _close(ref["bwd"][0], dx)
    aff = y.detach() * inp["s"].double().view(1, -1, 1, 1) + inp["o"].double().view(1, -1, 1, 1)
    assert _close(ref["aff0"][0], aff) and _close(ref["aff1"][0], torch.relu(aff))


@pytest.mark.parametrize("c", G.WG_CASES, ids=_ids(G.WG_CASES))
def test_filter_gradient_reference_equals_autograd(c):
    inp = G.make_wg_inputs(c)
    w = torch.zeros(c.C, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(inp["x"].double(), w, stride=c.stride, padding=1, groups=c.C) * inp["dy"].double()).sum().backward()
    assert _close(G.wg_reference(c, inp)["dw"][0], w.grad, 1e-11)


@pytest.mark.parametrize("c", [c for c in G.PD_CASES if c.kind == "randn"], ids=lambda c: c.name)
def test_pad_reference_equals_torch(c):
    inp = G.make_pd_inputs(c)
    ref = G.to_logical(G.pd_reference(c, inp)["out"][0], c.layout)
    a = G.to_logical(inp["a"], c.layout).double()
    if not c.bwd:
        assert torch.equal(ref.double(), F.pad(a, (1, 1, 1, 1), mode="reflect"))
    else:
        x = torch.zeros(c.B, c.C, c.H, c.W, dtype=torch.float64, requires_grad=True)
        (F.pad(x, (1, 1, 1, 1), mode="reflect") * a).sum().backward()
        assert _close(ref, x.grad)


@pytest.mark.parametrize("c", G.BE_CASES, ids=_ids(G.BE_CASES))
def test_bias_elu_reference_equals_torch(c):
    inp = G.make_be_inputs(c)
    z = inp["z"].double().requires_grad_()
    b = inp["bias"].double().requires_grad_()
    y = F.elu(z + G._be_bias_view(c, b))
    ref = G.be_fwd_reference(c, inp)["y"][0]
    assert _close(ref, y.detach())
    dz, db = torch.autograd.grad(y, (z, b), inp["dy"].double())
    bwd = G.be_bwd_reference(c, inp, ref)                    # from the exact y: the stored y differs by its rounding only
    assert _close(bwd["dz"][0], dz, 1e-9) and _close(bwd["db"][0], db, 1e-9)
    # the planted arguments are there: u == 0 and y == -1
    assert bool((ref == 0).any()) and bool((ref == -1).any())
    yp = G.plant_y(ref.to(G.dt_of(c.dt))).view(-1)
    assert float(yp[1]) == 0 and not torch.signbit(yp[1]) and float(yp[3]) == 0 and torch.signbit(yp[3]) and float(yp[5]) == -1


@pytest.mark.parametrize("c", [c for c in G.UC_CASES if c.kind == "randn"], ids=lambda c: c.name)
def test_up2cat_reference_equals_interpolate_and_cat(c):
    inp = G.make_uc_inputs(c)
    ref = G.uc_reference(c, inp)
    nchw = lambda t: t.permute(0, 3, 1, 2).double()          # noqa: E731
    a = nchw(inp["a"]).requires_grad_()
    parts = [F.interpolate(a, scale_factor=2, mode="nearest")]
    if c.C2:
        b = nchw(inp["b"]).requires_grad_()
        parts.append(b)
    out = torch.cat(parts, 1)
    assert torch.equal(nchw(ref["out"][0]), out.detach())
    grads = torch.autograd.grad(out, [a] + ([b] if c.C2 else []), nchw(inp["dout"]))
    assert _close(nchw(ref["da"][0]), grads[0])
    if c.C2:
        assert torch.equal(nchw(ref["db"][0]), grads[1])


@pytest.mark.parametrize("c", G.MP_CASES, ids=_ids(G.MP_CASES))
def test_maxpool_reference_index_equals_torch(c):
    inp = G.make_mp_inputs(c)
    x = inp["x"].permute(0, 3, 1, 2).double().contiguous().requires_grad_()
    y, ind = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    idx, pos = G.mp_index(inp["x"])
    assert torch.equal(pos.permute(0, 3, 1, 2), ind)
    ref = G.mp_reference(c, inp)
    yr = ref["y"][0].permute(0, 3, 1, 2).double()
    assert torch.equal(torch.isnan(yr), torch.isnan(y)) and torch.equal(torch.nan_to_num(yr, 7.0), torch.nan_to_num(y.detach(), 7.0))
    # the window index names the same pixel
    Ho, Wo = G.out_hw(c.H, c.W, 2)
    r, s = (idx // 3).long(), (idx % 3).long()
    iy = 2 * torch.arange(Ho).view(1, Ho, 1, 1) - 1 + r
    ix = 2 * torch.arange(Wo).view(1, 1, Wo, 1) - 1 + s
    assert torch.equal(iy * c.W + ix, pos) and int(idx.max()) <= 8
    (dx,) = torch.autograd.grad(y, x, inp["dy"].permute(0, 3, 1, 2).double())
    assert _close(ref["dx"][0].permute(0, 3, 1, 2), dx)
    if c.kind == "nan":
        assert int(torch.isnan(yr).sum()) > 0 and int(torch.isnan(inp["x"][0, 3:6, 3:6, 0]).sum()) == 2
    elif c.H * c.W >= 4:
        assert bool((G.mp_index(inp["x"], "last")[0] != idx).any()), "no tie in a post-ReLU row"


# ---------------------------------------------------------------------------------------------
# an honest fp32 run stays inside every bound, on every row
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in G.DW_CASES if c.arm_fwd is not None], ids=lambda c: c.name)
def test_stencil_emulation_is_inside_every_bound(c):
    inp = G.make_dw_inputs(c)
    _hold(f"dwconv3x3 {c.dt}", c.name, G.emulate_dw(c, inp), G.dw_reference(c, inp))


@pytest.mark.parametrize("c", G.WG_CASES, ids=_ids(G.WG_CASES))
def test_filter_gradient_emulation_is_inside_every_bound(c):
    inp = G.make_wg_inputs(c)
    em, ref = G.emulate_wg(c, inp), G.wg_reference(c, inp)
    _hold(f"dwconv3x3 filter gradient {c.dt}", c.name, dict(dw=em["dw"]), ref)
    assert bool(torch.isfinite(em["ws"]).all())
    assert G.check(em["ws"].double().sum(1).view(c.C, 1, 3, 3), *ref["dw"])[1] == 0


@pytest.mark.parametrize("c", G.PD_CASES, ids=_ids(G.PD_CASES))
def test_pad_emulation_is_inside_every_bound(c):
    inp = G.make_pd_inputs(c)
    _hold(f"reflect pad {c.layout} {'bwd' if c.bwd else 'fwd'} {c.dt}", c.name, G.emulate_pd(c, inp), G.pd_reference(c, inp))


@pytest.mark.parametrize("c", G.BE_CASES, ids=_ids(G.BE_CASES))
def test_bias_elu_emulation_is_inside_every_bound(c):
    inp = G.make_be_inputs(c)
    fwd = G.emulate_be_fwd(c, inp)
    _hold(f"bias+ELU {c.layout} fwd {c.dt}", c.name, fwd, G.be_fwd_reference(c, inp))
    y_in = G.plant_y(fwd["y"])
    bwd, ref = G.emulate_be_bwd(c, inp, y_in), G.be_bwd_reference(c, inp, y_in)
    assert tuple(bwd["partial"].shape) == G.be_partial_shape(c) and bool(torch.isfinite(bwd["partial"]).all())
    _hold(f"bias+ELU {c.layout} bwd {c.dt}", c.name, dict(dz=bwd["dz"], db=G.be_partial_sum(c, bwd["partial"])), ref)


@pytest.mark.parametrize("c", G.UC_CASES, ids=_ids(G.UC_CASES))
def test_up2cat_emulation_is_inside_every_bound(c):
    inp = G.make_uc_inputs(c)
    _hold(f"up2cat {c.dt}", c.name, G.emulate_uc(c, inp), G.uc_reference(c, inp))


@pytest.mark.parametrize("c", G.MP_CASES, ids=_ids(G.MP_CASES))
def test_maxpool_emulation_is_inside_every_bound(c):
    inp = G.make_mp_inputs(c)
    _hold(f"maxpool {c.dt}", c.name, G.emulate_mp(c, inp), G.mp_reference(c, inp))


# ---------------------------------------------------------------------------------------------
# planted faults fall outside
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fault", [("v_w16_s1_bf16", "halo_drop"), ("v_w40_s1_bf16", "halo_drop"), ("v_w8_s1_bf16", "right_edge"),
                                        ("v_w16_s1_bf16", "right_edge"), ("v_blocks_s1_bf16", "round_twice"), ("7x9_s2_bf16", "round_twice")])
def test_stencil_faults_are_caught(name, fault):
    c = _row(G.DW_CASES, name)
    inp = G.make_dw_inputs(c)
    ref = G.dw_reference(c, inp)
    assert not _caught(G.emulate_dw(c, inp), ref) and _caught(G.emulate_dw(c, inp, fault), ref), (name, fault)


@pytest.mark.parametrize("name", ["ragged_wide_s1_f32", "ragged_wide_s2_bf16", "clamp_s1_bf16", "ints_cap64_s1_f32", "ints_clamp_s2_bf16", "ints_ragged_s1_bf16"])
def test_a_dropped_last_part_of_the_filter_gradient_is_caught(name):
    c = _row(G.WG_CASES, name)
    inp = G.make_wg_inputs(c)
    ref = G.wg_reference(c, inp)
    assert not _caught(dict(dw=G.emulate_wg(c, inp)["dw"]), ref)
    assert _caught(dict(dw=G.emulate_wg(c, inp, "drop_last_part")["dw"]), ref)


@pytest.mark.parametrize("name,fault", [("nhwc_fwd_3x4_c64_bf16", "mirror_off_by_one"), ("nchw_fwd_2x7_c3_f32", "mirror_off_by_one"),
                                        ("nhwc_fwd_bits_bf16", "mirror_off_by_one"), ("nhwc_bwd_3x4_c64_bf16", "skip_second_border"),
                                        ("nchw_bwd_3x3_c3_f32", "skip_second_border"), ("nchw_bwd_3x7_c3_bf16", "skip_second_border")])
def test_pad_faults_are_caught(name, fault):
    c = _row(G.PD_CASES, name)
    inp = G.make_pd_inputs(c)
    ref = G.pd_reference(c, inp)
    assert not _caught(G.emulate_pd(c, inp), ref) and _caught(G.emulate_pd(c, inp, fault), ref), (name, fault)


@pytest.mark.parametrize("name", ["nhwc_c64_ragged_bf16", "nhwc_c8_ragged_f32", "nhwc_c2048_bf16", "nchw_hw4104_ragged_f32",
                                  "nchw_hw67x63_bf16", "nchw_hw8200_ragged_bf16"])
def test_a_dropped_last_slab_or_chunk_of_the_bias_sum_is_caught(name):
    c = _row(G.BE_CASES, name)
    inp = G.make_be_inputs(c)
    y_in = G.plant_y(G.emulate_be_fwd(c, inp)["y"])
    ref = G.be_bwd_reference(c, inp, y_in)
    for fault, want in ((None, False), ("drop_last", True)):
        bwd = G.emulate_be_bwd(c, inp, y_in, fault)
        assert _caught(dict(dz=bwd["dz"], db=G.be_partial_sum(c, bwd["partial"])), ref) == want, (name, fault)


@pytest.mark.parametrize("name", ["nchw_hw63_bf16", "nchw_hw5_f32", "nchw_hw67x63_f32"])
def test_an_unwritten_tail_is_caught(name):
    c = _row(G.BE_CASES, name)
    inp = G.make_be_inputs(c)
    assert _caught(G.emulate_be_fwd(c, inp, "tail_unwritten"), G.be_fwd_reference(c, inp))


def test_a_sum_rounded_twice_is_caught():
    c = _row(G.UC_CASES, "c24_40_6x10_bf16")
    inp = G.make_uc_inputs(c)
    ref = G.uc_reference(c, inp)
    assert not _caught(G.emulate_uc(c, inp), ref) and _caught(G.emulate_uc(c, inp, "round_twice"), ref)


@pytest.mark.parametrize("name", ["2x2_c8_f32", "13x19_c24_bf16", "24x40_c8_f32"])
def test_a_last_maximum_tie_rule_is_caught(name):
    c = _row(G.MP_CASES, name)
    inp = G.make_mp_inputs(c)
    ref = G.mp_reference(c, inp)
    got = G.emulate_mp(c, inp, "last_max")
    assert _caught(got, ref)
    assert G.check(got["idx"], *ref["idx"])[1] > 0 and G.check(got["dx"], *ref["dx"])[1] > 0      # the index and where the gradient goes
    assert G.check(got["y"], *ref["y"])[1] == 0                                                # the value cannot tell


@pytest.mark.parametrize("dtype", [BF16, F32, U8], ids=["bf16", "f32", "u8"])
def test_the_guards_see_an_unwritten_element_and_a_store_past_either_end(dtype):
    shape = (3, 5, 8)
    mk = lambda: G.guarded_u8(shape, "cpu") if dtype == U8 else G.guarded(shape, dtype, "cpu")           # noqa: E731
    buf, view = mk()
    assert G.guards_ok(buf, dtype) and view.data_ptr() % 16 == 0 and buf.numel() == 120 + 2 * G.GUARD
    if dtype == U8:
        assert bool((view == 0xFF).all())
    else:
        ref = torch.zeros(shape, dtype=torch.float64)
        view.zero_()
        assert G.check(view, ref, torch.zeros_like(ref))[1] == 0
        view.view(-1)[-1] = float("nan")                     # the tail element never stored
        assert G.check(view, ref, torch.full_like(ref, 1.0))[1] == 1
    for sl in (slice(G.GUARD + 120, G.GUARD + 128), slice(G.GUARD - 8, G.GUARD)):     # eight elements past the end / before the start
        buf, view = mk()
        buf[sl] = 0
        assert not G.guards_ok(buf, dtype)
