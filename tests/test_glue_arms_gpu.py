"""Every row of oracle/glue_inputs.py on the device: the 3x3 stencil (forward, affine forward, data and filter gradient), the
reflect pads, bias + ELU and upsample-cat in both layouts and the pose max-pool, through the raw ABI (tests/glue_launch.py)
against the float64 references (taken on the host), element by element, each element held to the bound derived in that module.  Outputs -- the
filter-gradient workspace, the bias partials and the max-pool index included -- are NaN-filled views into guarded buffers: an
element never stored is outside its bound, a store past either end changes a guard.  A row is served exactly when the library's
query says so and a refused call writes nothing; the restated part / slab / chunk plans equal the library's on every row; a
failure names the arm.  tests/test_glue_arms_cpu.py proves the census, the references, the bounds and that the bounds catch
faults.  One row per op goes through the autograd wrappers of ppeadepth.ops as well, so that their reshaping and `contiguous`
calls stay covered to the same bounds."""
import pytest
import torch

import glue_launch as L
from oracle import glue_inputs as G

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


def _ids(rows):
    return [r.name for r in rows]


def _hold(family, arm, tag, got, ref, bufs=()):
    """Every output element inside its bound, every guard intact; prints the worst ratio per output."""
    for key, (ref_t, bound) in ref.items():
        g = got[key].to(ref_t.device)
        assert tuple(g.shape) == tuple(ref_t.shape), (tag, key, arm)
        ratio, outside = G.check(g, ref_t, bound)
        print(f"GLUEARM {family} [{arm}] | {tag} {key}: worst err / bound {ratio:.3f}")
        assert outside == 0, f"{tag} {key} ({family}, {arm}): worst err / bound {ratio:.3f}, {outside} of {ref_t.numel()} elements outside"
    for buf, dtype in bufs:
        assert G.guards_ok(buf, dtype), f"{tag} ({family}, {arm}): a guard element was overwritten"


# ---------------------------------------------------------------------------------------------
# 3x3 stencil
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.DW_CASES, ids=_ids(G.DW_CASES))
def test_stencil_rows(device, c):
    """Forward, affine forward with and without ReLU, data gradient: generic kernel (one pixel, one row, odd sizes, the 64-block
    cap), dw3v_s1 (one to five tiles, H 1 and 2), the stride-2 pair and its three fall-backs, C = 1, refused shapes."""
    from ppeadepth import ops
    host = G.make_dw_inputs(c)
    inp = L.to(host, device)
    ref = G.dw_reference(c, host) if c.arm_fwd is not None else None
    dt = G.dt_of(c.dt)
    for what, mode, claimed in (("fwd", G.MODE_FWD, c.arm_fwd), ("aff0", G.MODE_AFFINE, c.arm_fwd), ("aff1", G.MODE_AFFINE, c.arm_fwd),
                                ("bwd", G.MODE_BWD, c.arm_bwd)):
        arm = ops.dwconv3x3_plan(dt, mode, c.N, c.C, c.H, c.W, c.stride)
        assert arm == claimed, (what, arm, claimed)
        served, got, bufs = L.launch_dw(ops, c, inp, what)
        torch.cuda.synchronize()
        assert served == (arm is not None), (what, G.DW3_ARM_NAMES[arm])
        if served:
            _hold(f"dwconv3x3 {what} {c.dt}", G.DW3_ARM_NAMES[arm], c.name, got, {what: ref[what]}, bufs)
        else:
            assert L.untouched(got, bufs), what


@pytest.mark.parametrize("c", G.WG_CASES, ids=_ids(G.WG_CASES))
def test_filter_gradient_rows(device, c):
    """One part, idle waves, a ragged last band, the lane loop, the parts > rows clamp, the 64-part cap; integer-valued rows
    to bound 0.  The workspace holds exactly the queried parts, all finite, and sums to the same bound; a second launch is
    bit-identical."""
    from ppeadepth import _abi, ops
    host = G.make_wg_inputs(c)
    inp = L.to(host, device)
    nbytes = _abi.lib.ppea_dwconv3x3_bwd_filter_workspace_bytes(c.N, c.C, c.H, c.W, c.stride)
    p = G.wgrad_plan(c.N, c.H, c.W, c.stride)
    assert nbytes == G.wgrad_workspace_bytes(c.N, c.C, c.H, c.W, c.stride) == c.C * p["parts"] * 36 and p["parts"] == c.claims["parts"]
    arm = f"dwconv3x3_bwd_filter<{c.dt}, {c.stride}> parts {p['parts']} x {p['rows_per_part']} rows"
    served, got, bufs = L.launch_wg(ops, c, inp, nbytes)
    served2, again, _ = L.launch_wg(ops, c, inp, nbytes)
    torch.cuda.synchronize()
    assert served and served2, arm
    ref = G.wg_reference(c, host)
    assert tuple(got["ws"].shape) == (c.C, p["parts"], 9) and bool(torch.isfinite(got["ws"]).all()), arm
    _hold(f"dwconv3x3 filter gradient {c.dt}", arm, c.name, dict(dw=got["dw"], ws=got["ws"].double().sum(1).view(c.C, 1, 3, 3)),
          dict(dw=ref["dw"], ws=ref["dw"]), bufs)
    assert torch.equal(G.bits(again["dw"]), G.bits(got["dw"])) and torch.equal(G.bits(again["ws"]), G.bits(got["ws"])), arm


def test_filter_gradient_refuses_what_its_query_refuses(device):
    from ppeadepth import _abi, ops
    for N, C, H, W, s in G.WG_UNSUPPORTED:
        assert _abi.lib.ppea_dwconv3x3_bwd_filter_workspace_bytes(N, C, H, W, s) == G.ERR_UNSUPPORTED
        c = G.Wg("refused", "bf16", max(N, 1), C, H, W, s, False, {})
        inp = L.to(G.make_wg_inputs(c._replace(stride=1)), device)
        served, got, bufs = L.launch_wg(ops, c._replace(N=N), inp, 36 * C)
        torch.cuda.synchronize()
        assert not served and L.untouched(got, bufs)


# ---------------------------------------------------------------------------------------------
# reflect pad
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.PD_CASES, ids=_ids(G.PD_CASES))
def test_reflect_pad_rows(device, c):
    """Both layouts, H, W in {2, 3, 4, 7} (2: forward only; 3: both border copies land on one line), C / 8 in {1, 3, 8}, arbitrary
    bit patterns through the copies, and the 8192-block cap of the NCHW kernels."""
    from ppeadepth import ops
    host = G.make_pd_inputs(c)
    served, got, bufs = L.launch_pd(ops, c, L.to(host, device))
    torch.cuda.synchronize()
    arm = f"{'nhwc_pad' if c.layout == 'nhwc' else 'reflect_pad1'}_{'bwd' if c.bwd else 'fwd'}<{c.dt}>"
    assert served, arm
    _hold(f"reflect pad {c.layout} {'bwd' if c.bwd else 'fwd'} {c.dt}", arm, c.name, got, G.pd_reference(c, host), bufs)


def test_reflect_pad_refused_shapes_write_nothing(device):
    from ppeadepth import ops
    for layout, bwd, B, C, H, W in G.PD_UNSUPPORTED:
        c = G.Pd("refused", layout, "bf16", B, C, H, W, bwd, "randn", "")
        served, got, bufs = L.launch_pd(ops, c, L.to(G.make_pd_inputs(c), device))
        torch.cuda.synchronize()
        assert not served and L.untouched(got, bufs), (layout, bwd, H, W, C)


# ---------------------------------------------------------------------------------------------
# bias + ELU
# ---------------------------------------------------------------------------------------------
def _be_query(_abi, c):
    if c.layout == "nhwc":
        return (_abi.lib.ppea_nhwc_bias_elu_slabs(c.N * c.HW, c.C), c.C)
    return (c.N * c.C, _abi.lib.ppea_bias_elu_chunks(c.N, c.C, c.HW))


@pytest.mark.parametrize("c", G.BE_CASES, ids=_ids(G.BE_CASES))
def test_bias_elu_rows(device, c):
    """Forward (u == 0 and u == -100 planted), then the backward on the stored output with +0.0, -0.0 and -1 planted: dz, and
    the partial sums -- exactly as many as the library's query says, every one finite -- added in float64 against the double
    sum of the exact dz.  channels_last: RL 256 / 32 / 2 / 1, idle row lanes, one slab, ragged slabs, the 1024-slab cap; NCHW:
    vector and scalar path, one chunk and several, 2048 planes of one pixel; the bias as fp32 and as bf16."""
    from ppeadepth import _abi, ops
    host = G.make_be_inputs(c)
    inp = L.to(host, device)
    pshape = _be_query(_abi, c)
    assert pshape == G.be_partial_shape(c)
    p = G.be_plan(c)
    arm = (f"nhwc_bias_elu<{c.dt}> RL {p['RL']} slabs {p['slabs']} x {p['rows']} rows" if c.layout == "nhwc"
           else f"bias_elu_kernel<{c.dt}> {'vector' if c.HW % 8 == 0 else 'scalar'} chunks {p['chunks']} x {p['per']}")
    served, fwd, bufs = L.launch_be_fwd(ops, c, inp)
    torch.cuda.synchronize()
    assert served, arm
    _hold(f"bias+ELU {c.layout} fwd {c.dt}", arm, c.name, fwd, G.be_fwd_reference(c, host), bufs)
    y_in = G.plant_y(fwd["y"])
    served, bwd, bufs = L.launch_be_bwd(ops, c, inp, y_in, pshape)
    torch.cuda.synchronize()
    assert served and bool(torch.isfinite(bwd["partial"]).all()), arm
    _hold(f"bias+ELU {c.layout} bwd {c.dt}", arm, c.name, dict(dz=bwd["dz"], db=G.be_partial_sum(c, bwd["partial"])),
          G.be_bwd_reference(c, host, y_in.cpu()), bufs)


def test_channels_last_bias_elu_refuses_the_channel_counts_its_query_refuses(device):
    from ppeadepth import _abi, ops
    for C in G.BE_UNSUPPORTED_C:
        assert _abi.lib.ppea_nhwc_bias_elu_slabs(40, C) == G.ERR_UNSUPPORTED
        c = G.Be("refused", "nhwc", "bf16", "f32", 1, C, 40, {})
        inp = L.to(G.make_be_inputs(c), device)
        served, got, bufs = L.launch_be_fwd(ops, c, inp)
        served2, got2, bufs2 = L.launch_be_bwd(ops, c, inp, inp["z"], (1, C))
        torch.cuda.synchronize()
        assert not served and not served2 and L.untouched(got, bufs) and L.untouched(got2, bufs2), C


# ---------------------------------------------------------------------------------------------
# upsample-cat, max-pool
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.UC_CASES, ids=_ids(G.UC_CASES))
def test_up2cat_rows(device, c):
    """C2 = 0, (8, 8), (24, 40): C / 8 not a power of two; H = W = 2; an odd source; N >= 2; arbitrary bit patterns through
    the copies (out and db; da is a sum)."""
    from ppeadepth import ops
    host = G.make_uc_inputs(c)
    served, got, bufs = L.launch_uc(ops, c, L.to(host, device))
    torch.cuda.synchronize()
    assert served
    _hold(f"up2cat {c.dt}", f"nhwc_up2cat<{c.dt}> C1 {c.C1} C2 {c.C2}", c.name, got, G.uc_reference(c, host), bufs)


@pytest.mark.parametrize("c", G.MP_CASES, ids=_ids(G.MP_CASES))
def test_maxpool_rows(device, c):
    """Values and the one-byte window index bit for bit (first maximum in scan order, every NaN takes over), the gradient
    gathered through the stored index; 1 x 1 to 24 x 40, C / 8 in {1, 3}, post-ReLU ties, planted NaNs."""
    from ppeadepth import ops
    host = G.make_mp_inputs(c)
    served, got, bufs = L.launch_mp(ops, c, L.to(host, device))
    torch.cuda.synchronize()
    assert served
    _hold(f"maxpool {c.dt}", f"nhwc_maxpool<{c.dt}> {c.kind}", c.name, got, G.mp_reference(c, host), bufs)


def test_up2cat_and_maxpool_refused_shapes_write_nothing(device):
    from ppeadepth import ops
    for N, C1, C2, H, W in G.UC_UNSUPPORTED:
        c = G.Uc("refused", "bf16", N, C1, C2, H, W, "randn", "")
        inp = L.to(G.make_uc_inputs(c._replace(C1=max(C1, 8))), device)
        dt, bufs = BF16, []
        out = L._out((N, H, W, max(C1 + C2, 8)), dt, device, bufs)
        da = L._out((N, max(H // 2, 1), max(W // 2, 1), max(C1, 8)), dt, device, bufs)
        db = L._out((N, H, W, max(C2, 8)), dt, device, bufs)
        st = ops.stream_ptr()
        assert not ops.try_call("ppea_nhwc_up2cat_fwd_bf16", ops.ptr(inp["a"]), ops.ptr(inp["b"]), ops.ptr(out), N, H, W, C1, C2, st)
        assert not ops.try_call("ppea_nhwc_up2cat_bwd_bf16", ops.ptr(inp["dout"]), ops.ptr(da), ops.ptr(db), N, H, W, C1, C2, st)
        torch.cuda.synchronize()
        assert L.untouched(dict(out=out, da=da, db=db), bufs), (N, C1, C2, H, W)
    for N, C, H, W in G.MP_UNSUPPORTED:
        c = G.Mp("refused", "bf16", N, C, H, W, "relu", "")
        inp = L.to(G.make_mp_inputs(c._replace(N=max(N, 1))), device)
        served, got, bufs = L.launch_mp(ops, c._replace(N=max(N, 1)), inp) if N > 0 else (None, None, None)
        if N > 0:
            torch.cuda.synchronize()
            assert not served and L.untouched(got, bufs), (N, C, H, W)
        else:
            bufs = []
            y = L._out((1, 2, 2, C), BF16, device, bufs)
            idx = L._out((1, 2, 2, C), U8, device, bufs)
            assert not ops.try_call("ppea_nhwc_maxpool3x3s2_fwd_bf16", ops.ptr(inp["x"]), ops.ptr(y), ops.ptr(idx), N, H, W, C, ops.stream_ptr())
            torch.cuda.synchronize()
            assert L.untouched(dict(y=y, idx=idx), bufs)


# ---------------------------------------------------------------------------------------------
# one row per op through the autograd wrappers
# ---------------------------------------------------------------------------------------------
def _nchw_view(t):
    """Storage [N, H, W, C] as the logical [N, C, H, W] channels_last tensor the wrappers take."""
    return t.permute(0, 3, 1, 2)


def _storage(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _row(rows, name):
    return next(r for r in rows if r.name == name)


@pytest.mark.parametrize("name", ["v_blocks_s2_bf16", "7x9_s1_f32"])
def test_dwconv3x3_wrappers(device, name):
    """ops.dwconv3x3 with a trainable filter (forward, data gradient, filter gradient) on a channels_last input and a
    non-contiguous incoming gradient, and ops.dwconv3x3_affine."""
    from ppeadepth import ops
    c = _row(G.DW_CASES, name)
    host = G.make_dw_inputs(c)
    inp = L.to(host, device)
    ref = G.dw_reference(c, host)
    x = inp["x"].contiguous(memory_format=torch.channels_last).requires_grad_()
    w = inp["w"].clone().requires_grad_()
    y = ops.dwconv3x3(x, w, c.stride)
    dy = inp["dy"].transpose(2, 3).contiguous().transpose(2, 3)
    y.backward(dy)
    tab = torch.stack([inp["s"], inp["o"]])
    got = dict(fwd=y.detach(), bwd=x.grad, aff0=ops.dwconv3x3_affine(x.detach(), inp["w"], tab, False, c.stride),
               aff1=ops.dwconv3x3_affine(x.detach(), inp["w"], tab, True, c.stride))
    torch.cuda.synchronize()
    assert all(t.dtype == G.dt_of(c.dt) for t in got.values()) and w.grad.dtype == F32 and y.is_contiguous()
    _hold(f"dwconv3x3 wrappers {c.dt}", "ops.dwconv3x3 / dwconv3x3_affine", c.name, got, ref)
    cw = G.Wg(c.name, c.dt, c.N, c.C, c.H, c.W, c.stride, False, {})
    _hold(f"dwconv3x3 wrappers {c.dt}", "ops.dwconv3x3 filter gradient", c.name, dict(dw=w.grad), G.wg_reference(cw, dict(x=host["x"], dy=host["dy"])))


@pytest.mark.parametrize("name", ["nhwc_c64_ragged_bf16", "nhwc_c8_ragged_f32", "nchw_hw67x63_bf16", "nchw_hw4104_ragged_f32"])
def test_bias_elu_wrapper(device, name):
    """ops.bias_elu with autograd: y, dz and the bias gradient (the wrapper's fp32 sum of the partials, rounded to the bias
    dtype: the partial bound with the slabs / chunks as further terms, plus that rounding)."""
    from ppeadepth import ops
    c = _row(G.BE_CASES, name)
    host = G.make_be_inputs(c)
    inp = L.to(host, device)
    H, W = c.HW, 1                                           # a one-column map: any pixel count
    if c.layout == "nhwc":
        z = _nchw_view(inp["z"].view(1, H, W, c.C)).detach().requires_grad_()
        dy = _nchw_view(inp["dy"].view(1, H, W, c.C))
        assert ops._is_nhwc(z)
        unview = lambda t: _storage(t).view(c.HW, c.C)                                          # noqa: E731
    else:
        z = inp["z"].view(c.N, c.C, H, W).detach().requires_grad_()
        dy = inp["dy"].view(c.N, c.C, H, W)
        unview = lambda t: t.contiguous().view(c.N, c.C, c.HW)                                  # noqa: E731
    b = inp["bias"].clone().requires_grad_()
    y = ops.bias_elu(z, b)
    assert y.is_contiguous(memory_format=torch.channels_last if c.layout == "nhwc" else torch.contiguous_format)
    y.backward(dy)
    torch.cuda.synchronize()
    ys = unview(y.detach())
    _hold(f"bias+ELU wrapper {c.layout} {c.dt}", "ops.bias_elu", c.name, dict(y=ys), G.be_fwd_reference(c, host))
    ref = G.be_bwd_reference(c, host, ys.cpu())
    parts = G.be_partial_shape(c)[0] if c.layout == "nhwc" else c.N * G.be_partial_shape(c)[1]
    n = c.N * c.HW
    db_ref, db_bound = ref["db"]
    db_bound = db_bound * (n + parts) / n + (G.U_BF16 * db_ref.abs() if c.bdt == "bf16" else 0.0)
    assert b.grad.dtype == inp["bias"].dtype
    _hold(f"bias+ELU wrapper {c.layout} {c.dt}", "ops.bias_elu", c.name, dict(dz=unview(z.grad), db=b.grad), dict(dz=ref["dz"], db=(db_ref, db_bound)))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bias_elu_keeps_the_format_of_a_channels_last_input_it_serves_on_the_nchw_kernel(device, dt):
    """C = 24 is not served by the channels_last kernel (C / 8 = 3 does not divide 256): ops.bias_elu documents `output in the
    same format`, so the result of the NCHW kernel comes back channels_last, values and gradients to the NCHW row's bounds."""
    from ppeadepth import ops
    c = G.Be(f"format_c24_{dt}", "nchw", dt, "f32", 2, 24, 35, {})
    host = G.make_be_inputs(c)
    inp = L.to(host, device)
    z = inp["z"].view(2, 24, 5, 7).contiguous(memory_format=torch.channels_last).requires_grad_()
    assert ops._is_nhwc(z) and not ops._nhwc_c_ok(24)
    b = inp["bias"].clone().requires_grad_()
    y = ops.bias_elu(z, b)
    assert y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous() and tuple(y.shape) == (2, 24, 5, 7)
    y.backward(inp["dy"].view(2, 24, 5, 7))
    torch.cuda.synchronize()
    ys = y.detach().contiguous().view(2, 24, 35)
    _hold(f"bias+ELU wrapper nchw {dt}", "ops.bias_elu channels_last C 24", c.name, dict(y=ys), G.be_fwd_reference(c, host))
    ref = G.be_bwd_reference(c, host, ys.cpu())
    _hold(f"bias+ELU wrapper nchw {dt}", "ops.bias_elu channels_last C 24", c.name, dict(dz=z.grad.contiguous().view(2, 24, 35), db=b.grad),
          dict(dz=ref["dz"], db=(ref["db"][0], ref["db"][1] * 72 / 70)))
    # an NCHW input stays NCHW, a served channels_last one channels_last
    assert ops.bias_elu(z.detach().contiguous(), b.detach()).is_contiguous()
    z64 = torch.randn(2, 64, 5, 7, device=device).to(G.dt_of(dt)).contiguous(memory_format=torch.channels_last)
    y64 = ops.bias_elu(z64, torch.zeros(64, device=device))
    assert y64.is_contiguous(memory_format=torch.channels_last) and not y64.is_contiguous()


@pytest.mark.parametrize("name", ["nhwc_bwd_3x4_c64_bf16", "nhwc_bwd_7x7_c8_f32", "nchw_bwd_4x3_c3_bf16", "nchw_bwd_3x7_c3_f32"])
def test_reflect_pad1_wrapper(device, name):
    from ppeadepth import ops
    c = _row(G.PD_CASES, name)
    cf = c._replace(bwd=False)
    host_f, host_b = G.make_pd_inputs(cf), G.make_pd_inputs(c)
    nhwc = c.layout == "nhwc"
    x = L.to(host_f, device)["a"]
    x = (_nchw_view(x) if nhwc else x).detach().requires_grad_()
    dout = L.to(host_b, device)["a"]
    out = ops.reflect_pad1(x)
    assert out.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
    out.backward(_nchw_view(dout) if nhwc else dout)
    torch.cuda.synchronize()
    st = _storage if nhwc else (lambda t: t.contiguous())
    _hold(f"reflect pad wrapper {c.layout} {c.dt}", "ops.reflect_pad1", c.name, dict(out=st(out.detach())), G.pd_reference(cf, host_f))
    _hold(f"reflect pad wrapper {c.layout} {c.dt}", "ops.reflect_pad1", c.name, dict(out=st(x.grad)), G.pd_reference(c, host_b))


@pytest.mark.parametrize("name", ["c24_40_6x10_bf16", "c16_0_6x4_f32"])
def test_upsample2x_cat_wrapper(device, name):
    from ppeadepth import ops
    c = _row(G.UC_CASES, name)
    host = G.make_uc_inputs(c)
    inp = L.to(host, device)
    a = _nchw_view(inp["a"]).detach().requires_grad_()
    b = _nchw_view(inp["b"]).detach().requires_grad_() if c.C2 else None
    assert ops.up2cat_supported(a, b)
    out = ops.upsample2x_cat(a, b)
    out.backward(_nchw_view(inp["dout"]))
    torch.cuda.synchronize()
    got = dict(out=_storage(out.detach()), da=_storage(a.grad))
    if c.C2:
        got["db"] = _storage(b.grad)
    _hold(f"up2cat wrapper {c.dt}", "ops.upsample2x_cat", c.name, got, G.uc_reference(c, host))


@pytest.mark.parametrize("name", ["13x19_c24_bf16", "nan_13x19_c8_f32"])
def test_maxpool3x3s2_wrapper(device, name):
    from ppeadepth import ops
    c = _row(G.MP_CASES, name)
    host = G.make_mp_inputs(c)
    inp = L.to(host, device)
    x = _nchw_view(inp["x"]).detach().requires_grad_()
    y = ops.maxpool3x3s2(x)
    assert y is not None and y.is_contiguous(memory_format=torch.channels_last)
    y.backward(_nchw_view(inp["dy"]))
    torch.cuda.synchronize()
    ref = G.mp_reference(c, host)
    _hold(f"maxpool wrapper {c.dt}", "ops.maxpool3x3s2", c.name, dict(y=_storage(y.detach()), dx=_storage(x.grad)), dict(y=ref["y"], dx=ref["dx"]))
