"""Edge shapes and edge values for the photometric path's small kernels -- grid_sample (forward, d grid), smooth_loss,
loss_select, loss_tail and cost_volume_reduce -- called through ppeadepth.ops, against fp64 references on the CPU built
from the same seeded fp32 inputs (oracle/edge_inputs.py; tests/test_loss_warp_edges_cpu.py shows the inputs and the
references are fit for it).  Tolerances are the suite's: 2e-5 forward, 2e-4 backward, 1e-6 where the loss_tail test
already holds it; index, mask and confidence tensors bit-exact."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import edge_inputs as E
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5
BWD_TOL = 2e-4
TAIL_TOL = 1e-6


def _ops():
    from ppeadepth import ops
    return ops


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
# grid_sample
# ---------------------------------------------------------------------------------------------
_GRID_REF = {}


def _grid_ref(shape, mode):
    """inputs + fp64 CPU reference (output, d grid), computed once per (shape, mode) and never modified."""
    key = (shape, mode)
    if key not in _GRID_REF:
        Hi, Wi, Ho, Wo, C = shape
        seed = E.GRID_SEEDS[shape]
        blocks = E.grid_blocks(Hi, Wi)
        grid = E.grid_cases(Hi, Wi, Ho, Wo, seed)
        src = E.grid_source(len(blocks), C, Hi, Wi, seed)
        go = torch.randn(len(blocks), C, Ho, Wo, generator=_g(seed + 1))
        if "lattice" in blocks and C > 1:
            go[blocks.index("lattice"), C // 2] = 0           # a channel that must add nothing to d grid
        gr = grid.double().requires_grad_(True)
        out = F.grid_sample(src.double(), gr, mode="bilinear", padding_mode=mode, align_corners=True)
        (out * go.double()).sum().backward()
        _GRID_REF[key] = (blocks, grid, src, go, out.detach(), gr.grad)
    return _GRID_REF[key]


@pytest.mark.parametrize("mode", ["border", "zeros"])
@pytest.mark.parametrize("shape", E.GRID_SHAPES, ids=str)
def test_grid_sample_edges(device, shape, mode):
    ops = _ops()
    Hi, Wi, Ho, Wo, C = shape
    blocks, grid, src, go, ref_out, ref_grad = _grid_ref(shape, mode)
    gd = grid.to(device).requires_grad_(True)
    out = ops.grid_sample(src.to(device), gd, mode)
    (out * go.to(device)).sum().backward()
    out, grad = out.detach().cpu(), gd.grad.cpu()
    assert out.shape == ref_out.shape and grad.shape == grid.shape
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    for b, name in enumerate(blocks):
        e_out = rel_err(out[b], ref_out[b]) if ref_out[b].any() else float(out[b].abs().max())
        if name == "random":
            bad = E.near_integer(grid[b][None], Hi, Wi)[0]
            assert float(bad.float().mean()) <= 0.01
            keep = ~bad
            e_grad = rel_err(grad[b][keep], ref_grad[b][keep])
        else:
            e_grad = rel_err(grad[b], ref_grad[b]) if ref_grad[b].any() else float(grad[b].abs().max())
        print(f"grid_sample {shape} {mode} {name}: out {e_out:.3g} grad {e_grad:.3g}")
        assert e_out < FWD_TOL, (name, e_out)
        assert e_grad < BWD_TOL, (name, e_grad)
        if mode == "border" and name in ("lattice", "rim"):
            # clip_coordinates_set_grad: no gradient along an axis whose coordinate is at or beyond the rim
            for k in (0, 1):
                at_rim = grid[b][..., k].abs() >= 1
                assert at_rim.any()
                assert not grad[b][..., k][at_rim].any(), (name, k)
                inside = ~at_rim & (ref_grad[b][..., k] != 0)
                assert (grad[b][..., k][inside] != 0).all(), (name, k)
        if mode == "zeros" and name == "far":
            assert not out[b].any() and not grad[b].any()
        if mode == "border" and name == "far":
            assert not grad[b].any()


# ---------------------------------------------------------------------------------------------
# smooth_loss
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.SMOOTH_SHAPES, ids=str)
def test_smooth_loss_edges(device, shape):
    """(3, 3, 96, 457) is 131 616 pixels: 544 past the 512 x 256 threads of one sweep of the forward's grid-stride loop."""
    ops = _ops()
    B, C, H, W = shape
    disp, img = E.smooth_cases(B, C, H, W, 300 + E.SMOOTH_SHAPES.index(shape))
    up = -2.5
    dr = disp.double().requires_grad_(True)
    ref = R.smooth_loss(dr, img.double())
    (ref * up).backward()
    dd = disp.to(device).requires_grad_(True)
    got = ops.smooth_loss(dd, img.to(device))
    (got * up).backward()
    grad = dd.grad.cpu()
    e_f, e_b = rel_err(got.detach().cpu().reshape(1), ref.detach().reshape(1)), rel_err(grad, dr.grad)
    print(f"smooth_loss {shape}: fwd {e_f:.3g} bwd {e_b:.3g}")
    assert e_f < FWD_TOL
    assert e_b < BWD_TOL
    flat = E.flat_pixels(disp)
    assert not grad[flat].any()                                 # sgn(0) == 0 on every side: exactly no gradient


# ---------------------------------------------------------------------------------------------
# loss_select
# ---------------------------------------------------------------------------------------------
def _select_reference(c, selec, noise):
    rp = c["reproj"]
    if selec:
        sel, fidx = R.select_reprojection(rp, c["warped_m1"], c["warped_p1"])
    else:
        sel, fidx = torch.min(rp, dim=1, keepdim=True)
    idm = c["identity"].min(1, keepdim=True)[0]
    aidx, _ = R.automask(sel, idm if noise is None else idm + noise)
    return sel, fidx, aidx, E.select_source_code(fidx, c["warped_m1"], c["warped_p1"], selec)


def _run_select(ops, device, c, selec, noise, grad_out=None):
    rd = c["reproj"].clone().to(device).requires_grad_(grad_out is not None)
    sel, src, fidx, aidx = ops.loss_select(rd, c["identity"].to(device), [c["warped_m1"].to(device), c["warped_p1"].to(device)],
                                           None if noise is None else noise.to(device), selec)
    if grad_out is not None:
        sel.backward(grad_out.to(device))
    return sel.detach().cpu(), src.cpu(), fidx.cpu(), aidx.cpu(), (rd.grad.cpu() if grad_out is not None else None)


@pytest.mark.parametrize("with_noise", [False, True], ids=["no_noise", "noise"])
@pytest.mark.parametrize("selec", [True, False], ids=["selec", "plain_min"])
@pytest.mark.parametrize("shape", E.SELECT_SHAPES, ids=str)
def test_loss_select_edges(device, shape, selec, with_noise):
    ops = _ops()
    B, C, H, W = shape
    c = E.select_cases(B, C, H, W, E.SELECT_SEEDS[shape])
    noise = c["noise"] if with_noise else None
    ref_sel, ref_fidx, ref_aidx, ref_src = _select_reference(c, selec, noise)
    go = torch.randn(B, 1, H, W, generator=_g(11))
    sel, src, fidx, aidx, d_reproj = _run_select(ops, device, c, selec, noise, go)
    assert torch.equal(sel, ref_sel)
    assert fidx.dtype == torch.int64 and torch.equal(fidx, ref_fidx)
    assert aidx.dtype == torch.int64 and torch.equal(aidx, ref_aidx)
    assert src.dtype == torch.uint8 and torch.equal(src, ref_src)
    # backward: autograd through the reference in fp64; every entry is the upstream value or 0, hence exact
    r64 = c["reproj"].detach().double().requires_grad_(True)
    if selec:
        s64, _ = R.select_reprojection(r64, c["warped_m1"], c["warped_p1"])
    else:
        s64, _ = torch.min(r64, dim=1, keepdim=True)
    s64.backward(go.double())
    assert torch.equal(d_reproj.double(), r64.grad)


def test_loss_select_nan_rule(device):
    """torch.min / torch.argmin: NaN propagates and the first NaN's index wins."""
    ops = _ops()
    shape = E.SELECT_SHAPES[-1]
    c = E.select_cases(*shape, E.SELECT_SEEDS[shape], nan_layer=True)
    for selec in (True, False):
        for noise in (None, c["noise"]):
            ref_sel, ref_fidx, ref_aidx, ref_src = _select_reference(c, selec, noise)
            sel, src, fidx, aidx, _ = _run_select(ops, device, c, selec, noise)
            assert torch.isnan(ref_sel).sum() >= 4
            assert torch.equal(fidx, ref_fidx)
            assert torch.equal(aidx, ref_aidx)
            assert torch.equal(torch.isnan(sel), torch.isnan(ref_sel))
            assert torch.equal(torch.nan_to_num(sel, nan=-1.0), torch.nan_to_num(ref_sel, nan=-1.0))
            assert torch.equal(src, ref_src)


# ---------------------------------------------------------------------------------------------
# loss_tail
# ---------------------------------------------------------------------------------------------
def _check_tail(ops, device, c, is_multi, use_cons=True, use_aug=True, all_masked=False):
    ref = E.tail_reference(c, is_multi, use_cons, use_aug)
    rd = c["reproj"].clone().to(device).requires_grad_(True)
    md = c["multi"].clone().to(device).requires_grad_(True)
    res = ops.loss_tail(rd, c["sel"].to(device), c["src"].to(device), None if is_multi else c["auto_idx"].to(device),
                        c["cons"].to(device) if (is_multi and use_cons) else None,
                        c["aug"].to(device) if (is_multi and use_aug) else None,
                        md if is_multi else None, c["mono"].to(device) if is_multi else None, is_multi)
    (res[0] * 0.7 + (res[1] * 1.3 if is_multi else 0)).backward()
    rl = res[0].detach().cpu().reshape(1)
    assert torch.equal(res[2].cpu().double(), ref["mask"])
    if all_masked:
        assert float(rl) == 0.0
        assert not rd.grad.cpu().any()
    else:
        e = rel_err(rl, ref["rl"].reshape(1))
        e_g = rel_err(rd.grad.cpu(), ref["d_reproj"]) if ref["d_reproj"].any() else float(rd.grad.abs().max())
        print(f"loss_tail {tuple(c['sel'].shape)} multi={is_multi} cons={use_cons} aug={use_aug}: rl {e:.3g} d_reproj {e_g:.3g}")
        assert e < TAIL_TOL
        assert e_g < TAIL_TOL
    if is_multi:
        e_c = rel_err(res[1].detach().cpu().reshape(1), ref["cl"].reshape(1)) if float(ref["cl"]) != 0 else abs(float(res[1].detach()))
        e_t = rel_err(res[3].cpu(), ref["target"])
        e_m = rel_err(md.grad.cpu(), ref["d_multi"]) if ref["d_multi"].any() else float(md.grad.abs().max())
        print(f"    consistency {e_c:.3g} target {e_t:.3g} d_multi {e_m:.3g}")
        assert e_c < TAIL_TOL
        assert e_t < TAIL_TOL
        assert e_m < TAIL_TOL


@pytest.mark.parametrize("is_multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("shape", E.TAIL_SHAPES, ids=str)
def test_loss_tail_edges(device, shape, is_multi):
    """(3, 3, 5): hw = 15, a thread's four pixels cross from one item (and its `aug`) into the next, 45 pixels in all;
    (2, 7, 73): 1022 pixels, the last thread stops after two; (2, 192, 684): 257 blocks, one more than the finalize
    kernel's 256 threads."""
    ops = _ops()
    B, H, W = shape
    c = E.tail_cases(B, H, W, 5, is_multi)
    _check_tail(ops, device, c, is_multi)
    if is_multi and B * H * W < 100000:
        _check_tail(ops, device, c, True, use_cons=False)
        _check_tail(ops, device, c, True, use_aug=False)
        _check_tail(ops, device, c, True, use_cons=False, use_aug=False)


@pytest.mark.parametrize("is_multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("shape", E.TAIL_SHAPES[:3], ids=str)
def test_loss_tail_all_masked(device, shape, is_multi):
    """sum(mask) == 0: rl = 0 / 1e-7 = 0 and no gradient reaches the reprojection loss; the consistency term then covers
    every pixel."""
    ops = _ops()
    B, H, W = shape
    _check_tail(ops, device, E.tail_cases(B, H, W, 5, is_multi, all_masked=True), is_multi, all_masked=True)


# ---------------------------------------------------------------------------------------------
# cost_volume_reduce
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.REDUCE_SHAPES, ids=str)
def test_cost_volume_reduce_edges(device, shape):
    ops = _ops()
    B, D, h, w = shape
    raw = E.reduce_cases(B, D, h, w)
    bins = R.depth_bins_log(0.37, 14.5, D)
    ref_masked, ref_conf, ref_idx, ref_low = E.reduce_reference(raw, bins, R)
    masked, conf, idx, low = ops.cost_volume_reduce(raw.to(device), bins.to(device))
    assert torch.equal(conf.cpu(), ref_conf)
    assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), ref_idx)
    assert torch.equal(masked.cpu(), ref_masked)                # v * 1 + mx * 0 and its mirror: exact in fp32
    e = rel_err(low.cpu(), ref_low)
    print(f"cost_volume_reduce {shape}: lowest {e:.3g}")
    assert e < FWD_TOL
