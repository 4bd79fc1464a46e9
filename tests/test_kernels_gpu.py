"""GPU parity: every HIP kernel, called through the C ABI (ppeadepth.ops -> libppea_depth.so),
against the CPU oracle (oracle/ref_ops.py) on the same seeded inputs and against the golden
vectors generated from the reference.

Tolerances (north_star): fp32 outputs within 1e-3 relative (we hold 2e-5 on forward values,
1e-4 on gradients); index tensors bit-exact.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5
BWD_TOL = 2e-4


def _ops():
    from ppeadepth import ops
    return ops


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H,W", [(31, 48, 160), (29, 24, 80), (27, 12, 40), (13, 6, 20),
                                   (31, 12, 20), (29, 24, 64), (27, 12, 32), (13, 6, 16),
                                   (31, 50, 37), (27, 33, 70), (13, 17, 9), (31, 1, 1)])
def test_dwconv_lk_fwd_bwd(device, K, H, W):
    ops = _ops()
    N, C = 2, 6
    x = torch.randn(N, C, H, W, generator=_g(K * 1000 + H))
    wb = torch.randn(C, 1, K, K, generator=_g(1)) / K
    ws = torch.randn(C, 1, 5, 5, generator=_g(2)) / 5
    xd = x.to(device).requires_grad_(True)
    yb, ys = ops.dwconv_lk(xd, wb.to(device), ws.to(device))
    assert rel_err(yb.cpu(), R.dwconv(x, wb)) < FWD_TOL
    assert rel_err(ys.cpu(), R.dwconv(x, ws)) < FWD_TOL
    gb = torch.randn(N, C, H, W, generator=_g(3))
    gs = torch.randn(N, C, H, W, generator=_g(4))
    (yb * gb.to(device) + ys * gs.to(device)).sum().backward()
    xr = x.clone().requires_grad_(True)
    (R.dwconv(xr, wb) * gb + R.dwconv(xr, ws) * gs).sum().backward()
    assert rel_err(xd.grad.cpu(), xr.grad) < BWD_TOL


@pytest.mark.parametrize("K", [7, 9, 21])
def test_dwconv_generic_sizes_and_wgrad(device, K):
    """Kernel sizes without a tuned instantiation (plug-in contract: any k > 5) + weight gradient."""
    ops = _ops()
    N, C, H, W = 2, 4, 11, 13
    x = torch.randn(N, C, H, W, generator=_g(K))
    w = (torch.randn(C, 1, K, K, generator=_g(K + 1)) / K)
    xd = x.to(device).requires_grad_(True)
    wd = w.to(device).requires_grad_(True)
    y, none = ops.dwconv_lk(xd, wd, None)
    assert none is None
    assert rel_err(y.cpu(), R.dwconv(x, w)) < FWD_TOL
    g = torch.randn(N, C, H, W, generator=_g(5))
    (y * g.to(device)).sum().backward()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (R.dwconv(xr, wr) * g).sum().backward()
    assert rel_err(xd.grad.cpu(), xr.grad) < BWD_TOL
    assert rel_err(wd.grad.cpu(), wr.grad) < BWD_TOL


def test_dwconv_golden_reference(device, golden):
    """Against the reference's own conv outputs (tests/golden/replk_blocks.npz)."""
    ops = _ops()
    g = golden("replk_blocks")
    for k in (31, 29, 27, 13):
        x = g[f"lk{k}:x"]
        wb = g[f"lk{k}:sd:lkb_origin.conv.weight"]
        ws = g[f"lk{k}:sd:small_conv.conv.weight"]
        yb, ys = ops.dwconv_lk(x.to(device), wb.to(device), ws.to(device))
        assert rel_err(yb.cpu(), g[f"lk{k}:y_big_conv"]) < FWD_TOL
        assert rel_err(ys.cpu(), g[f"lk{k}:y_small_conv"]) < FWD_TOL


@pytest.mark.parametrize("K,N,C,H,W", [(31, 3, 4, 48, 160), (29, 4, 4, 24, 80), (27, 5, 4, 12, 40), (13, 7, 4, 6, 20),
                                       (13, 2, 64, 2, 3), (27, 2, 32, 4, 6), (29, 2, 16, 8, 12), (31, 2, 8, 16, 24),
                                       (31, 2, 3, 48, 128), (29, 2, 3, 24, 64), (27, 3, 3, 12, 32), (13, 3, 3, 6, 16),
                                       (31, 2, 2, 70, 37), (27, 1, 2, 33, 90), (13, 2, 2, 17, 9), (31, 1, 1, 1, 1),
                                       (31, 2, 2, 128, 256),
                                       # the batch-major variant (12 x W / 6 x W planes): full and ragged image groups, an
                                       # odd channel count (idle wave), 1 / 2 / 3 column tiles, W % 8 == 4
                                       (27, 12, 6, 12, 40), (27, 17, 2, 12, 40), (27, 20, 3, 12, 8), (27, 1, 1, 12, 24),
                                       (13, 12, 8, 6, 20), (13, 18, 5, 6, 16), (13, 33, 2, 6, 44), (29, 12, 3, 24, 80), (29, 9, 2, 24, 64),
                                       # 48-row planes in column segments, interleaved rows (>= 12 of 16 MFMA rows filled)
                                       (31, 12, 3, 48, 160), (31, 16, 2, 48, 56), (31, 30, 1, 48, 24)])
def test_dwconv_bf16_mfma(device, K, N, C, H, W):
    """bf16 I/O on the matrix cores (banded-Toeplitz MFMA kernel): bf16 activations and bf16-rounded
    filters (what autocast feeds a conv), fp32 accumulation, one bf16 rounding of the output."""
    ops = _ops()
    # the arms the parameter list's comments claim, from the library's own plan (family 1 row-band, 2 batch-major)
    fwd, dgrad = (ops.dwconv_lk_plan(N, C, H, W, K, 5, mode) for mode in (0, 1))
    if (K, H) in ((27, 12), (13, 6), (29, 24)) and W % 4 == 0 and W <= 80:
        assert (fwd["family"], fwd["H"], dgrad["family"], dgrad["H"]) == (2, H, 2, H), (fwd, dgrad)
    if (K, H) == (31, 48) and N >= 12:
        assert (dgrad["family"], dgrad["H"], dgrad["NY"], dgrad["RS"]) == (2, 48, 12, 4) and fwd["family"] == 1, (fwd, dgrad)
    x = torch.randn(N, C, H, W, generator=_g(K + H)).bfloat16()
    wb = torch.randn(C, 1, K, K, generator=_g(8)) / K
    ws = torch.randn(C, 1, 5, 5, generator=_g(9)) / 5
    wbq, wsq = wb.bfloat16().float(), ws.bfloat16().float()

    def close(a, ref):
        a = a.float().cpu()
        return bool(((a - ref).abs() <= ref.abs() * 2 ** -7 + ref.abs().max() * 1e-3 + 1e-6).all())

    xd = x.to(device).requires_grad_(True)
    yb, ys = ops.dwconv_lk(xd, wb.to(device), ws.to(device))
    assert yb.dtype == torch.bfloat16
    assert close(yb, R.dwconv(x.float(), wbq))
    assert close(ys, R.dwconv(x.float(), wsq))
    y1, none = ops.dwconv_lk(x.to(device), wb.to(device), None)          # big branch alone
    assert none is None and close(y1, R.dwconv(x.float(), wbq))
    gb = torch.randn(N, C, H, W, generator=_g(3)).bfloat16()
    gs = torch.randn(N, C, H, W, generator=_g(4)).bfloat16()
    torch.autograd.backward([yb, ys], [gb.to(device), gs.to(device)])
    xr = x.float().clone().requires_grad_(True)
    (R.dwconv(xr, wbq) * gb.float() + R.dwconv(xr, wsq) * gs.float()).sum().backward()
    assert close(xd.grad, xr.grad)


def test_dwconv_linearity_full_size(device):
    """Size-independent property at the BASELINE config-2 shape [12,128,48,160], k=31:
    conv(a*x1 + x2) == a*conv(x1) + conv(x2), and a delta input reproduces the flipped filter."""
    ops = _ops()
    N, C, H, W, K = 12, 128, 48, 160, 31
    g = torch.Generator(device="cpu").manual_seed(11)
    wb = (torch.randn(C, 1, K, K, generator=g) / K).to(device)
    x1 = torch.randn(N, C, H, W, generator=g).to(device)
    x2 = torch.randn(N, C, H, W, generator=g).to(device)
    y1, _ = ops.dwconv_lk(x1, wb, None)
    y2, _ = ops.dwconv_lk(x2, wb, None)
    y12, _ = ops.dwconv_lk(1.5 * x1 + x2, wb, None)
    assert rel_err(y12, 1.5 * y1 + y2) < 1e-5
    delta = torch.zeros(1, C, H, W, device=device)
    delta[:, :, 24, 80] = 1.0
    yd, _ = ops.dwconv_lk(delta, wb, None)
    patch = yd[0, :, 24 - 15:24 + 16, 80 - 15:80 + 16]
    assert torch.equal(patch, wb[:, 0].flip(-1, -2))


@pytest.mark.parametrize("N,C,H,W,K", [(12, 128, 48, 160, 31),       # config 2: RepLKNet-31B stage 0, batch 12
                                       (8, 192, 48, 160, 31),        # config 4: RepLKNet-31L stage 0, batch 8
                                       (8, 384, 24, 80, 29),         # config 4: stage 1
                                       (2, 128, 128, 256, 31),       # config 5: 512x1024 frames, stage 0
                                       (12, 512, 12, 40, 27),        # config 2: stage 2 (batch-major variant)
                                       (8, 768, 12, 40, 27),         # config 4: stage 2
                                       (12, 1024, 6, 20, 13)])       # config 2: stage 3
def test_dwconv_bf16_mfma_full_size_vs_fp32_kernel(device, N, C, H, W, K):
    """The BENCHMARKED kernel at the benchmarked shapes of configs 2, 4 and 5: bf16 through `dwconv_mfma_kernel<K,5,*,*>`
    (forward and data gradient) against the fp32 vector kernel `dwconv_lk_kernel` on the same bf16-rounded values.
    Tolerance: both accumulate in fp32; the MFMA path rounds its result to bf16 once (2^-8 relative) and sums the
    K*K taps in a different order (a few 1e-4 of the output scale)."""
    ops = _ops()
    if H in (12, 6):                                     # "batch-major variant": so says the plan, in both directions
        assert [ops.dwconv_lk_plan(N, C, H, W, K, 5, mode)["family"] for mode in (0, 1)] == [2, 2]
    g = torch.Generator(device="cpu").manual_seed(21)
    wb = (torch.randn(C, 1, K, K, generator=g) / K).bfloat16().float().to(device)
    ws = (torch.randn(C, 1, 5, 5, generator=g) / 5).bfloat16().float().to(device)
    x = torch.randn(N, C, H, W, generator=g).bfloat16().to(device)
    gb = torch.randn(N, C, H, W, generator=g).bfloat16().to(device)
    gs = torch.randn(N, C, H, W, generator=g).bfloat16().to(device)

    def run(xin, gbin, gsin):
        xin = xin.clone().requires_grad_(True)
        yb, ys = ops.dwconv_lk(xin, wb, ws)
        torch.autograd.backward([yb, ys], [gbin, gsin])
        return yb, ys, xin.grad

    yb16, ys16, dx16 = run(x, gb, gs)
    assert yb16.dtype == torch.bfloat16 and dx16.dtype == torch.bfloat16
    yb32, ys32, dx32 = run(x.float(), gb.float(), gs.float())
    for a, b in ((yb16, yb32), (ys16, ys32), (dx16, dx32)):
        a = a.float()
        bad = (a - b).abs() > b.abs() * 2 ** -7 + b.abs().max() * 1e-3
        assert not bool(bad.any()), float((a - b).abs().max() / b.abs().max())


def test_dwconv_trainable_filter_is_repacked(device):
    """--fullft_reb: the flat Adam kernel updates filters through raw pointers (no `_version` bump).  A trainable
    filter must therefore never be served from the packed-image cache."""
    ops = _ops()
    C, K = 8, 13
    w = torch.nn.Parameter((torch.randn(C, 1, K, K, generator=_g(1)) / K).to(device))
    x = torch.randn(2, C, 6, 20, generator=_g(2)).bfloat16().to(device)
    y1, _ = ops.dwconv_lk(x, w, None)
    w.data.mul_(2.0)                               # `.data`: storage changes, version counter does not
    y2, _ = ops.dwconv_lk(x, w, None)
    assert rel_err(y2.float(), 2.0 * y1.float()) < 2 ** -7


# ---------------------------------------------------------------------------------------------
def test_backproject_project_golden(device, golden):
    ops = _ops()
    g = golden("layers_geometry")
    grid = ops.backproject_project(g["depth"].to(device), g["inv_K"].to(device), g["K"].to(device),
                                   g["T_inv"].to(device))
    assert (grid.cpu() - g["grid"]).abs().max() < 2e-5


@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (1, 5, 7), (3, 3, 300)])
def test_backproject_project_grad(device, B, H, W):
    ops = _ops()
    from oracle import synth
    depth = 0.5 + 5 * torch.rand(B, 1, H, W, generator=_g(1))
    K, inv_K = synth.kitti_K(H, W, 0)
    K, inv_K = K[None].repeat(B, 1, 1), inv_K[None].repeat(B, 1, 1)
    T = R.transformation_from_parameters(0.02 * torch.randn(B, 1, 3, generator=_g(2)),
                                         0.1 * torch.randn(B, 1, 3, generator=_g(3)), True)
    gg = torch.randn(B, H, W, 2, generator=_g(4))
    dr, Tr = depth.clone().requires_grad_(True), T.clone().requires_grad_(True)
    (R.project3d(R.backproject(dr, inv_K), K, Tr, H, W) * gg).sum().backward()
    dd, Td = depth.to(device).requires_grad_(True), T.to(device).requires_grad_(True)
    (ops.backproject_project(dd, inv_K.to(device), K.to(device), Td) * gg.to(device)).sum().backward()
    assert rel_err(dd.grad.cpu(), dr.grad) < BWD_TOL
    assert rel_err(Td.grad.cpu(), Tr.grad) < BWD_TOL


def test_backproject_project_pose_gradient_is_bitwise_reproducible(device):
    """dP sums 122 880 per-pixel terms per image.  Round 1 added the per-block sums with float atomics, so the pose
    gradient depended on the order in which the blocks finished (found in round 2: repeated runs of the same 10 steps
    diverged in the pose branch only).  Now: per-block partials in a workspace, summed in a fixed order -- 20 launches
    on the same data give the same bits (full-size frame, poisoned workspace and output)."""
    ops = _ops()
    from oracle import synth
    B, H, W = 4, 192, 640
    depth = (0.5 + 5 * torch.rand(B, 1, H, W, generator=_g(1))).to(device)
    K, inv_K = synth.kitti_K(H, W, 0)
    K, inv_K = K[None].repeat(B, 1, 1).to(device), inv_K[None].repeat(B, 1, 1).to(device)
    T = R.transformation_from_parameters(0.02 * torch.randn(B, 1, 3, generator=_g(2)),
                                         0.1 * torch.randn(B, 1, 3, generator=_g(3)), True).to(device)
    gg = torch.randn(B, H, W, 2, generator=_g(4)).to(device)
    first = None
    for rep in range(20):
        dd, Td = depth.clone().requires_grad_(True), T.clone().requires_grad_(True)
        junk = torch.full((1 << 20,), float("nan"), device=device)          # whatever the allocator hands out next
        del junk
        (ops.backproject_project(dd, inv_K, K, Td) * gg).sum().backward()
        got = (Td.grad.clone(), dd.grad.clone())
        if first is None:
            first = got
            assert torch.isfinite(got[0]).all()
        else:
            assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), rep


@pytest.mark.parametrize("mode", ["border", "zeros"])
def test_grid_sample(device, golden, mode):
    ops = _ops()
    g = golden("layers_geometry")
    key = "warped_wide" if mode == "border" else "warped_zeros"
    out = ops.grid_sample(g["src"].to(device), g["wide_grid"].to(device), mode)
    assert rel_err(out.cpu(), g[key]) < FWD_TOL
    if mode == "border":
        assert rel_err(ops.grid_sample(g["src"].to(device), g["grid"].to(device), mode).cpu(), g["warped"]) < FWD_TOL
    # gradient w.r.t. the grid vs the oracle (F.grid_sample autograd on CPU)
    grid = g["wide_grid"].clone()
    gr = grid.clone().requires_grad_(True)
    go = torch.randn(g["src"].shape[0], 3, *grid.shape[1:3], generator=_g(5))
    fn = R.grid_sample_border if mode == "border" else R.grid_sample_zeros
    (fn(g["src"], gr) * go).sum().backward()
    gd = grid.to(device).requires_grad_(True)
    (ops.grid_sample(g["src"].to(device), gd, mode) * go.to(device)).sum().backward()
    assert rel_err(gd.grad.cpu(), gr.grad) < BWD_TOL


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(24, 40), (17, 63), (192, 640), (2, 2), (2, 7), (4, 4), (3, 130)])
def test_ssim_l1(device, H, W):
    ops = _ops()
    B = 2
    pred = torch.rand(B, 3, H, W, generator=_g(1000 + H))
    tgt = torch.rand(B, 3, H, W, generator=_g(2000 + W))      # distinct seeds: pred == tgt is degenerate
    pr = pred.clone().requires_grad_(True)
    ref = R.reprojection_loss(pr, tgt)
    pd = pred.to(device).requires_grad_(True)
    out = ops.ssim_l1(pd, tgt.to(device))
    assert rel_err(out.cpu(), ref) < FWD_TOL
    go = torch.randn(B, 1, H, W, generator=_g(9))
    (ref * go).sum().backward()
    (out * go.to(device)).sum().backward()
    assert rel_err(pd.grad.cpu(), pr.grad) < BWD_TOL


def test_ssim_l1_golden(device, golden):
    ops = _ops()
    g = golden("losses")
    out = ops.ssim_l1(g["pred_m1"].to(device), g["tgt"].to(device))
    assert rel_err(out.cpu(), g["reproj_m1"]) < FWD_TOL
    # identical images -> SSIM loss 0, L1 0 (idempotence)
    z = ops.ssim_l1(g["tgt"].to(device), g["tgt"].to(device))
    assert float(z.abs().max()) < 1e-6


def test_smooth_loss(device, golden):
    ops = _ops()
    g = golden("layers_geometry")
    s = ops.smooth_loss(g["disp"].to(device), g["tgt"].to(device))
    assert rel_err(s.cpu(), g["smooth"]) < FWD_TOL
    dr = g["disp"].clone().requires_grad_(True)
    (R.smooth_loss(dr, g["tgt"]) * 3.0).backward()
    dd = g["disp"].to(device).requires_grad_(True)
    (ops.smooth_loss(dd, g["tgt"].to(device)) * 3.0).backward()
    assert rel_err(dd.grad.cpu(), dr.grad) < BWD_TOL


def test_loss_select_indices_bit_exact(device, golden):
    ops = _ops()
    g = golden("losses")
    tgt = g["tgt"]
    rp = torch.cat([R.reprojection_loss(g["pred_m1"], tgt), R.reprojection_loss(g["pred_p1"], tgt)], 1)
    idl = torch.cat([R.reprojection_loss(g["src_m1"], tgt), R.reprojection_loss(g["src_p1"], tgt)], 1)
    noise = g["mono:noise"] * 0.00001
    sel, src, fidx, aidx = ops.loss_select(rp.to(device), idl.to(device), [g["pred_m1"].to(device), g["pred_p1"].to(device)],
                                           noise.to(device), True)
    ref_sel, ref_fidx = R.select_reprojection(rp, g["pred_m1"], g["pred_p1"])
    assert torch.equal(sel.cpu(), ref_sel)
    assert fidx.dtype == torch.int64 and torch.equal(fidx.cpu(), ref_fidx)
    ref_idx, _ = R.automask(ref_sel, idl.min(1, keepdim=True)[0] + noise)
    assert aidx.dtype == torch.int64 and torch.equal(aidx.cpu(), ref_idx)
    # exact ties resolve to index 0 (first minimum), as torch.argmin does
    a, b = g["tie_a"], g["tie_b"]
    zeros = torch.ones_like(g["pred_m1"])
    _, _, _, tie = ops.loss_select(torch.cat([a, a], 1).to(device), torch.cat([b, b], 1).to(device),
                                   [zeros.to(device), zeros.to(device)], None, True)
    assert torch.equal((tie == 0).float().cpu(), g["tie_mask"])


# ---------------------------------------------------------------------------------------------
def test_cost_volume_golden(device, golden):
    ops = _ops()
    g = golden("cost_volume")
    bins = R.depth_bins_log(g["min_depth"], g["max_depth"], 96)
    cost = ops.cost_volume(g["cur"].to(device), g["lookup"][:, 0].to(device), g["poses"][:, 0].to(device),
                           g["K"].to(device), g["inv_K"].to(device), bins.to(device))
    masked, conf, idx, low = ops.cost_volume_reduce(cost, bins.to(device))
    # reference `cost` is after missing->max fill; compare the filled volume via masked/conf
    ref_conf = g["confidence"]
    assert torch.equal(conf.cpu(), ref_conf)
    assert rel_err(masked.cpu(), g["cost"] * ref_conf.unsqueeze(1)) < FWD_TOL
    assert idx.dtype == torch.int64
    assert torch.equal(idx.cpu(), g["argmin"])                      # bit-exact index tensor
    assert rel_err(low.cpu(), g["lowest_cost"]) < FWD_TOL
    assert float(cost[2].abs().max()) == 0.0                        # zeroed pose -> skipped item


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("two,act,res", [(False, 0, False), (False, 1, False), (True, 1, False), (False, 2, False),
                                         (False, 0, True)])
@pytest.mark.parametrize("shape", [(3, 8, 12, 40), (2, 5, 7, 9), (2, 4, 48, 160), (5, 64, 12, 40), (3, 130, 6, 20)])
def test_fused_bn_act(device, dtype, two, act, res, shape):
    """act(BN_a(z1) [+ BN_b(z2)]) * mask + r1 + s*r2 (training-mode batch statistics), forward, running
    statistics and all gradients against the oracle composite."""
    import torch.nn.functional as F
    from ppeadepth import ops
    N, C, H, W = shape
    g = _g(N * 100 + C + act)
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    z1 = (torch.randn(shape, generator=g) * 2 + 0.5).to(dt)
    z2 = (torch.randn(shape, generator=g) * 0.7 - 0.2).to(dt)
    g1, b1 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    g2, b2 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    mask = torch.tensor(([0.0] + [1.4] * N)[:N])
    r1 = torch.randn(shape, generator=g).to(dt)
    r2 = torch.randn(shape, generator=g).to(dt)
    go = torch.randn(shape, generator=g).to(dt)

    def ref():
        leaves = [t.float().clone().requires_grad_(True) for t in (z1, z2, g1, b1, g2, b2, r1, r2)]
        a, bb, w1, c1, w2, c2, q1, q2 = leaves
        rm, rv = torch.zeros(C), torch.ones(C)
        u = F.batch_norm(a, rm, rv, w1, c1, True, 0.1, 1e-5)
        if two:
            u = u + F.batch_norm(bb, torch.zeros(C), torch.ones(C), w2, c2, True, 0.1, 1e-5)
        u = F.relu(u) if act == 1 else (F.gelu(u) if act == 2 else u)
        if res:
            u = u * mask.view(-1, 1, 1, 1) + q1 + 0.5 * q2
        (u * go.float()).sum().backward()
        return u.detach(), leaves, rm, rv

    y_ref, leaves, rm_ref, rv_ref = ref()
    d = [t.to(device).requires_grad_(True) for t in (z1, z2, g1, b1, g2, b2, r1, r2)]
    rm, rv = torch.zeros(C, device=device), torch.ones(C, device=device)
    mean1, _, invstd1 = ops.bn_batch_stats(d[0].detach(), 1e-5, 0.1, rm, rv)
    kw = {}
    if two:
        mean2, _, invstd2 = ops.bn_batch_stats(d[1].detach(), 1e-5, 0.1, None, None)
        kw.update(z2=d[1], g2=d[4], b2=d[5], mean2=mean2, invstd2=invstd2)
    if res:
        kw.update(mask=mask.to(device), r1=d[6], r2=d[7], r2_scale=0.5)
    y = ops.bn_act_apply(d[0], d[2], d[3], mean1, invstd1, act=act, **kw)
    (y.float() * go.to(device).float()).sum().backward()
    tol_f, tol_b = (2e-5, 2e-4) if dtype == "f32" else (1e-2, 3e-2)
    assert rel_err(y.float().cpu(), y_ref) < tol_f
    assert rel_err(rm.cpu(), rm_ref) < 1e-5 and rel_err(rv.cpu(), rv_ref) < 1e-4
    used = [0, 2, 3] + ([1, 4, 5] if two else []) + ([6, 7] if res else [])
    for i in used:
        assert rel_err(d[i].grad.float().cpu(), leaves[i].grad) < tol_b, i


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 3, 6, 20), (1, 2, 3, 3), (2, 4, 24, 80), (1, 1, 3, 9)])
def test_reflect_pad1(device, dtype, shape):
    import torch.nn.functional as F
    from ppeadepth import ops
    x = torch.randn(shape, generator=_g(shape[2])).to(dtype)
    go = torch.randn(shape[0], shape[1], shape[2] + 2, shape[3] + 2, generator=_g(3)).to(dtype)
    xr = x.float().clone().requires_grad_(True)
    (F.pad(xr, (1, 1, 1, 1), mode="reflect") * go.float()).sum().backward()
    xd = x.to(device).requires_grad_(True)
    y = ops.reflect_pad1(xd)
    assert torch.equal(y.detach().cpu(), F.pad(x, (1, 1, 1, 1), mode="reflect"))
    (y.float() * go.to(device).float()).sum().backward()
    assert rel_err(xd.grad.float().cpu(), xr.grad) < (1e-6 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(2, 8, 24, 40), (1, 3, 7, 9), (2, 4, 1, 5), (2, 4, 16, 32), (1, 3, 6, 48), (2, 2, 2, 16)])
def test_dwconv3x3(device, dtype, stride, shape):
    import torch.nn.functional as F
    from ppeadepth import ops
    N, C, H, W = shape
    x = torch.randn(shape, generator=_g(H + stride)).to(dtype)
    w = torch.randn(C, 1, 3, 3, generator=_g(7)) / 3
    xr = x.float().clone().requires_grad_(True)
    ref = F.conv2d(xr, w, None, stride, 1, 1, C)
    go = torch.randn(ref.shape, generator=_g(8)).to(dtype)
    (ref * go.float()).sum().backward()
    xd = x.to(device).requires_grad_(True)
    y = ops.dwconv3x3(xd, w.to(device), stride)
    tol = 2e-5 if dtype == torch.float32 else 1e-2
    assert y.shape == ref.shape and rel_err(y.float().cpu(), ref) < tol
    (y.float() * go.to(device).float()).sum().backward()
    assert rel_err(xd.grad.float().cpu(), xr.grad) < tol


@pytest.mark.parametrize("B,M,K,H,W", [(2, 128, 128, 48, 160), (3, 512, 128, 12, 40), (2, 64, 256, 24, 80),
                                       (2, 32, 128, 6, 20), (1, 200, 96, 5, 8), (2, 1024, 256, 6, 20)])
def test_pwconv_mfma(device, B, M, K, H, W):
    """1x1 conv on MFMA (transposing LDS reads) vs fp32 matmul of the bf16-rounded operands, with bias;
    autograd wrapper: data gradient through the transposed matrix."""
    from ppeadepth import ops
    g = _g(M + K)
    x = torch.randn(B, K, H, W, generator=g).bfloat16()
    w = (torch.randn(M, K, 1, 1, generator=g) / K ** 0.5).bfloat16()
    bias = torch.randn(M, generator=g)
    ref = torch.einsum("mk,bkhw->bmhw", w.float().view(M, K), x.float()) + bias.view(1, -1, 1, 1)
    y = ops.pwconv_raw(w.view(M, K).contiguous().to(device), x.to(device), bias.to(device))
    assert y is not None
    assert (y.float().cpu() - ref).abs().max() <= ref.abs().max() * 2 ** -7
    xd = x.to(device).requires_grad_(True)
    wd = w.to(device)
    y2 = ops.pwconv_frozen(xd, wd)
    if M % 32:                                  # the data gradient contracts over M: not served, caller falls back
        assert y2 is None
        return
    go = torch.randn(B, M, H, W, generator=g).bfloat16()
    y2.backward(go.to(device))
    gref = torch.einsum("mk,bmhw->bkhw", w.float().view(M, K), go.float())
    assert (xd.grad.float().cpu() - gref).abs().max() <= gref.abs().max() * 2 ** -7


@pytest.mark.parametrize("N,K,M,H,W,act", [(12, 512, 2048, 12, 40, 2), (3, 128, 256, 6, 20, 1), (5, 64, 128, 12, 40, 0)])
def test_bn_channel_statistics_from_the_gemm_epilogue(device, N, K, M, H, W, act):
    """The one-launch channel BatchNorm with its statistics taken from the producing 1x1 conv's epilogue sums
    (`ppea_bn_fwd_channel_sums_*`: the FFN's BatchNorm + GELU at stages 2 / 3): saved / running statistics equal to the
    in-kernel reduction's to 1e-6 / 1e-5, outputs and gradients to bf16 rounding."""
    from ppeadepth import ops
    from ppeadepth.batchnorm import BatchNorm2d
    g = _g(N + K + M)
    x = torch.randn(N, K, H, W, generator=g).bfloat16().to(device)
    w = (torch.randn(M, K, 1, 1, generator=g) / K ** 0.5).to(device)
    go = torch.randn(N, M, H, W, generator=g).bfloat16().to(device)
    res = []
    for use_sums in (False, True):
        bn = BatchNorm2d(M).to(device)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(M, generator=_g(1)) + 0.5)
            bn.bias.copy_(torch.randn(M, generator=_g(2)) * 0.2)
        xl = x.clone().requires_grad_(True)
        z, sums = ops.pwconv_frozen(xl, w, want_sums=True)
        outs = ops.bn_act_channel(z, bn, act=act, sums=sums if use_sums else None)
        y, st = outs[0], outs[1]
        y.backward(go)
        res.append((y.detach(), st.clone(), bn.running_mean.clone(), bn.running_var.clone(), xl.grad, bn.weight.grad, bn.bias.grad))
    a, b = res
    assert rel_err(b[1][0], a[1][0]) < 1e-5 and rel_err(b[1][1], a[1][1]) < 1e-5
    assert rel_err(b[2], a[2]) < 1e-5 and rel_err(b[3], a[3]) < 1e-5
    assert rel_err(b[0].float(), a[0].float()) < 2 ** -6
    for k in (4, 5, 6):
        assert rel_err(b[k].float(), a[k].float()) < 2e-2, k


@pytest.mark.parametrize("B,C,Ch,H,W,taps", [(12, 512, 128, 12, 40, 1), (3, 128, 32, 48, 160, 1), (2, 256, 64, 24, 80, 9),
                                              (2, 200, 160, 8, 12, 1), (2, 64, 32, 6, 20, 1)])
def test_pwgrad_pair_equals_two_launches(device, B, C, Ch, H, W, taps):
    """An adapter's two weight gradients (D_fc2: dy x h, D_fc1: g x x, the latter tap-major for the 3x3 form) in ONE GEMM
    launch + ONE reduce launch against the two-launch form: same sums to fp32 summation order (the split count differs),
    bias gradients included; shapes whose planes are not a multiple of 32 pixels fall back to the two launches."""
    from ppeadepth import ops
    g = _g(B + C + Ch)
    dy = torch.randn(B, C, H, W, generator=g).bfloat16().to(device)
    h = torch.randn(B, Ch, H, W, generator=g).bfloat16().to(device)
    gg = torch.randn(B, taps * Ch, H, W, generator=g).bfloat16().to(device)
    x = torch.randn(B, C, H, W, generator=g).bfloat16().to(device)
    w1_shape = (Ch, C, 3, 3) if taps == 9 else (Ch, C)
    a = (dy, h, (C, Ch), torch.float32, 1, (0, C), torch.float32)
    b = (gg, x, w1_shape, torch.bfloat16, taps, ((4 * Ch, Ch) if taps == 9 else (0, Ch)), torch.bfloat16)
    (dw2, db2), (dw1, db1) = ops.pwgrad_into_pair(a, b)
    r2, r1 = ops.pwgrad_into(*a), ops.pwgrad_into(*b)
    assert rel_err(dw2, r2[0]) < 1e-5 and rel_err(db2, r2[1]) < 1e-5
    assert rel_err(dw1.float(), r1[0].float()) < 2 ** -7 and rel_err(db1.float(), r1[1].float()) < 2 ** -7
    ref = torch.einsum("bmp,bnp->mn", dy.float().flatten(2), h.float().flatten(2))
    assert rel_err(dw2, ref) < 1e-4


@pytest.mark.parametrize("epi", ["none", "dgelu"])
@pytest.mark.parametrize("B,M,K,H,W", [(12, 128, 512, 12, 40), (3, 512, 128, 12, 40), (2, 160, 128, 24, 80), (2, 72, 96, 6, 20),
                                       (1, 1024, 256, 5, 8), (2, 128, 1152, 12, 40)])
def test_pwconv_transposed_matrix_on_the_lds_dma_ring(device, monkeypatch, epi, B, M, K, H, W):
    """The transposed-A mode (At [K][M]: the adapters' and the frozen convs' data gradients use the forward matrix as is)
    on the v2 kernel, whose A tile then has the X tile's layout and comes out of the same transposing LDS read: equal to
    v1's transposed mode to bf16 rounding, and both to the fp32 product of the bf16 operands; ragged M (160, 72) and M
    tiles past the matrix included."""
    from ppeadepth import ops
    g = _g(M + K + H)
    x = torch.randn(B, K, H, W, generator=g).bfloat16().to(device)
    at = (torch.randn(K, M, generator=g) / K ** 0.5).bfloat16().to(device)
    aux = torch.randn(B, M, H, W, generator=g).bfloat16().to(device)
    kw = dict(epi=ops.EPI_DGELU, aux=aux) if epi == "dgelu" else {}
    ref = torch.einsum("km,bkhw->bmhw", at.float(), x.float())
    if epi == "dgelu":
        a = aux.float()
        ref = ref * (0.5 * (1 + torch.erf(a / 2 ** 0.5)) + a * torch.exp(-0.5 * a * a) / (2 * torch.pi) ** 0.5)
    monkeypatch.setenv("PPEA_PW_V2", "0")
    y1 = ops.pwconv_ex(at, x, transposed=True, **kw)
    monkeypatch.delenv("PPEA_PW_V2")
    y2 = ops.pwconv_ex(at, x, transposed=True, **kw)
    y1, y2 = (y1[0] if isinstance(y1, tuple) else y1), (y2[0] if isinstance(y2, tuple) else y2)
    tol = ref.abs().max() * 2 ** -7
    assert (y1.float() - ref).abs().max() <= tol and (y2.float() - ref).abs().max() <= tol


@pytest.mark.parametrize("tile", ["128,64", "128,32", "64,64", "64,32", "32,64"])
@pytest.mark.parametrize("B,M,K,H,W", [(2, 256, 128, 48, 160), (3, 512, 256, 12, 40), (2, 200, 192, 24, 80),
                                       (3, 96, 512, 6, 20), (1, 1024, 1024, 5, 8), (5, 64, 64, 13, 8)])
def test_pwconv_v2_lds_dma_ring_every_tile(device, monkeypatch, tile, B, M, K, H, W):
    """pwconv v2 (three-stage LDS ring filled by LDS-DMA, counted vmcnt, XCD-aware tile order, 16-byte epilogue stores),
    every tile shape forced in turn: plain / bias, the GELU epilogue (pre-activation + activation), the GELU' epilogue and
    the BatchNorm-statistics epilogue against the fp32 product of the bf16-rounded operands and against v1 (identical
    rounding points: equal to the last bf16 bit up to fp32 summation order); ragged channel tiles (M % BM != 0), planes
    that are not a multiple of the 128-pixel tile, K of 1-16 steps."""
    import os
    from ppeadepth import _abi, ops
    bk = int(tile.split(",")[1])
    if K % bk:
        pytest.skip("tile needs K % BK == 0 (the dispatch then takes another tile)")
    g = _g(M + K + H)
    x = torch.randn(B, K, H, W, generator=g).bfloat16().to(device)
    a = (torch.randn(M, K, generator=g) / K ** 0.5).bfloat16().to(device)
    bias = torch.randn(M, generator=g).to(device)
    aux = torch.randn(B, M, H, W, generator=g).bfloat16().to(device)
    ref = torch.einsum("mk,bkhw->bmhw", a.float(), x.float())
    ptr, sp = _abi.ptr, _abi.stream_ptr

    def run():
        y0 = ops.pwconv_raw(a, x, bias)
        pre, act = ops.pwconv_ex(a, x, bias, ops.EPI_GELU)
        dg = ops.pwconv_ex(a, x, None, ops.EPI_DGELU, aux)
        P = _abi.lib.ppea_pwconv_stats_partials(B, M, K, H * W)
        ys = torch.empty(B, M, H, W, device=device, dtype=torch.bfloat16)
        sums = torch.full((M, P, 2), float("nan"), device=device)
        _abi.call("ppea_pwconv_stats_bf16", ptr(a), ptr(x), None, ptr(ys), ptr(sums), B, M, K, H * W, sp())
        return y0, pre, act, dg, ys, sums

    monkeypatch.setenv("PPEA_PW_V2", tile)
    y0, pre, act, dg, ys, sums = run()
    monkeypatch.setenv("PPEA_PW_V2", "0")
    v1 = run()
    monkeypatch.delenv("PPEA_PW_V2")
    tol = 2 ** -7
    refb = ref + bias.view(1, -1, 1, 1)
    assert (y0.float() - refb).abs().max() <= refb.abs().max() * tol
    assert torch.equal(pre, y0)
    assert (act.float() - torch.nn.functional.gelu(pre.float())).abs().max() <= 2 ** -7 * act.float().abs().max()
    xa = aux.float()
    dgelu = 0.5 * (1 + torch.erf(xa / 2 ** 0.5)) + xa * torch.exp(-0.5 * xa * xa) / (2 * torch.pi) ** 0.5
    assert (dg.float() - ref * dgelu).abs().max() <= (ref * dgelu).abs().max() * tol
    assert (ys.float() - ref).abs().max() <= ref.abs().max() * tol
    tot = sums.double().sum(1)
    assert torch.isfinite(tot).all()
    assert rel_err(tot[:, 0].float(), ys.float().sum((0, 2, 3))) < 1e-5
    assert rel_err(tot[:, 1].float(), (ys.float() ** 2).sum((0, 2, 3))) < 1e-5
    for mine, old in zip((y0, act, dg, ys), (v1[0], v1[2], v1[3], v1[4])):
        # same operands, same rounding points; only the fp32 summation order inside a K step may differ
        assert (mine.float() - old.float()).abs().max() <= old.float().abs().max() * 2 ** -7
        assert (mine != old).float().mean() < 0.02


@pytest.mark.parametrize("v2", ["1", "0"])
@pytest.mark.parametrize("B,M,N,H,W", [(2, 128, 128, 12, 40), (3, 288, 128, 48, 160), (2, 100, 36, 6, 20),
                                       (12, 1152, 512, 12, 40), (1, 32, 256, 3, 8), (2, 130, 34, 8, 32),
                                       (12, 288, 128, 48, 160), (5, 64, 514, 4, 8)])
def test_pwgrad_mfma(device, monkeypatch, v2, B, M, N, H, W):
    """Pixel-contraction GEMM (weight gradients) + row sums vs fp32 einsum of the bf16 operands: v2 (three-stage LDS ring
    filled by LDS-DMA, planes that are a multiple of the 32-pixel step) and v1 (any plane with HW % 8 == 0); ragged row /
    column tiles, result widths that are not a multiple of 4, 1 .. 11 splits."""
    from ppeadepth import ops
    monkeypatch.setenv("PPEA_PWGRAD_V2", v2)
    g = _g(M + N)
    p = torch.randn(B, M, H, W, generator=g).bfloat16()
    q = torch.randn(B, N, H, W, generator=g).bfloat16()
    ref = torch.einsum("bmhw,bnhw->mn", p.double(), q.double()).float()
    rs_ref = p.double().sum((0, 2, 3)).float()
    c, rs = ops.pwgrad(p.to(device), q.to(device))
    assert (c.cpu() - ref).abs().max() <= 1e-4 * (B * H * W) ** 0.5 + 1e-5 * ref.abs().max()
    assert (rs.cpu() - rs_ref).abs().max() <= 1e-4 * (B * H * W) ** 0.5
    c2, none = ops.pwgrad(p.to(device), q.to(device), want_rowsum=False)
    assert none is None and torch.equal(c2, c)                     # deterministic


def _adapter_ref(kind, x, w1, b1, w2, b2):
    import torch.nn.functional as F
    if kind == "conv":
        h = F.gelu(F.conv2d(x, w1, b1, padding=1))
    else:
        h = F.gelu(torch.einsum("mk,bkhw->bmhw", w1, x) + b1.view(1, -1, 1, 1))
    return torch.einsum("cm,bmhw->bchw", w2, h) + b2.view(1, -1, 1, 1)


@pytest.mark.parametrize("kind", ["conv", "mlp"])
@pytest.mark.parametrize("B,C,H,W", [(2, 128, 12, 40), (2, 256, 6, 20), (1, 128, 48, 160), (3, 512, 4, 8)])
def test_adapters_mfma(device, kind, B, C, H, W):
    """Adapter / B_Adapter forward + all gradients on the MFMA kernels vs an fp32 autograd reference
    evaluated on the same bf16-rounded inputs and parameters."""
    from ppeadepth import ops
    Ch = C // 4
    g = _g(C + H)
    x = torch.randn(B, C, H, W, generator=g).bfloat16()
    w1 = (torch.randn(*((Ch, C, 3, 3) if kind == "conv" else (Ch, C)), generator=g) /
          (C * (9 if kind == "conv" else 1)) ** 0.5).bfloat16()
    b1 = (0.1 * torch.randn(Ch, generator=g)).bfloat16()
    w2 = (torch.randn(C, Ch, generator=g) / Ch ** 0.5).bfloat16()
    b2 = (0.1 * torch.randn(C, generator=g)).bfloat16()
    go = torch.randn(B, C, H, W, generator=g).bfloat16()
    leaves = [t.float().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    ref = _adapter_ref(kind, *leaves)
    ref.backward(go.float())
    dl = [t.to(device).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    assert ops.adapter_supported(dl[0], Ch)
    y = (ops.conv_adapter if kind == "conv" else ops.mlp_adapter)(*dl)
    y.backward(go.to(device))
    tol = 2 ** -6
    assert (y.float().cpu() - ref).abs().max() <= tol * ref.abs().max()
    for name, a, r in zip(("dx", "dw1", "db1", "dw2", "db2"), dl, leaves):
        assert a.grad.dtype == a.dtype
        err = (a.grad.float().cpu() - r.grad).abs().max()
        assert err <= tol * r.grad.abs().max(), (name, float(err), float(r.grad.abs().max()))


def test_adam_flat_matches_torch_adam(device):
    """One-launch Adam over a flat buffer == torch.optim.Adam (reference defaults) step for step -- parameters and both
    moments; the bf16 working copy of the head of the buffer is the rounded master.  The two fp32 evaluations carry their
    own states, so the moments' differences add up over the steps: each evaluation adds at most the a-priori one-step error
    of tests/test_adam_cpu.py -- 2 u (|m_prev| + |g|) to m (earlier differences shrink by b1), 6 u relative to v (all terms
    positive: relative differences add).  On top of that the two do not use the same 1 - b: the C ABI carries b as fp32 and
    the kernel forms 1 - fp32(b) (exact), torch rounds the double 1 - b to fp32; fp32(b)'s error u b, seen from 1 - b, is
    u b / (1 - b): 9 u for b1, 999 u = 6e-5 for b2 (1.3e-5 in fact).  It scales every g^2 term of v alike, so it does not add
    up over the steps, and it drops out of the update, whose bias correction uses the same fp32(b2) ("Optimizer
    phase").  (tests/test_adam_gpu.py holds the kernel to float64 one step at a time.)"""
    from ppeadepth._abi import call, ptr, stream_ptr
    g = _g(5)
    n, n_lo = 10007, 4099
    p0 = torch.randn(n, generator=g)
    ref = p0.clone().to(device).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    P = p0.clone().to(device)
    M, V = torch.zeros_like(P), torch.zeros_like(P)
    W16 = torch.empty(n_lo, device=device, dtype=torch.bfloat16)
    state = torch.tensor([0.0, 1e-3], device=device)
    u, m_tol = 2.0 ** -24, 0.0
    for step in range(4):
        grad = (torch.randn(n, generator=g) * (10.0 ** (step - 2))).to(device)
        ref.grad = grad.clone()
        opt.step()
        state[0] += 1
        m_tol += (2 * 2 + 0.1 * 9) * u * float(M.abs().max() + grad.abs().max())
        call("ppea_adam_flat_f32", ptr(P), ptr(grad), ptr(M), ptr(V), ptr(W16), n, n_lo, ptr(state), 0.9, 0.999, 1e-8,
             stream_ptr())
        assert (P - ref.detach()).abs().max() <= 2e-7 * ref.detach().abs().max() + 1e-9, step
        st = opt.state[ref]
        assert float((M - st["exp_avg"]).abs().max()) <= m_tol, step
        assert bool(((V - st["exp_avg_sq"]).abs() <= ((step + 1) * 2 * 6 + 999) * u * st["exp_avg_sq"]).all()), step
    assert torch.equal(W16, P[:n_lo].bfloat16())


@pytest.mark.parametrize("invert", [False, True])
def test_pose_matrix_kernel_equals_the_composite(device, invert):
    """A15 `transformation_from_parameters` (layers.py:26-42, 61-100) as one launch per direction: the matrix and the
    gradients of axis-angle and translation against the element-wise composite in fp32 (the backward's Jacobian comes from
    the same arithmetic on dual numbers), incl. small and zero rotation angles."""
    from ppeadepth import layers
    g = _g(3 + int(invert))
    aa = (torch.randn(12, 1, 3, generator=g) * torch.tensor([1e-3, 1e-2, 0.1, 1.0] * 3).view(12, 1, 1))
    aa[5] = 0.0
    tr = torch.randn(12, 1, 3, generator=g)
    go = torch.randn(12, 4, 4, generator=g)
    res = []
    for kernel in (False, True):
        layers.POSE_MATRIX_KERNEL = kernel
        try:
            a = aa.clone().to(device).requires_grad_(True)
            t = tr.clone().to(device).requires_grad_(True)
            T = layers.transformation_from_parameters(a, t, invert)
            (T * go.to(device)).sum().backward()
            res.append((T.detach().cpu(), a.grad.cpu(), t.grad.cpu()))
        finally:
            layers.POSE_MATRIX_KERNEL = True
    ok = [i for i in range(12) if i != 5]                    # (the composite's own gradient at a zero angle is NaN / 0-0)
    assert (res[1][0] - res[0][0]).abs().max() < 2e-6
    assert rel_err(res[1][1][ok], res[0][1][ok]) < 1e-4 and rel_err(res[1][2], res[0][2]) < 1e-5
    assert torch.isfinite(res[1][1]).all()


@pytest.mark.parametrize("invert", [False, True])
def test_pose_matrix_kernel_vs_reference_golden_and_oracle_autograd(device, golden, invert):
    """A15 against the REFERENCE, not against this repo's own composite: (1) the kernel's matrices on
    the golden's axis-angle / translation equal `layers_geometry.npz:T_fwd / T_inv` -- outputs of the reference's own
    `transformation_from_parameters` (layers.py:26-58); (2) matrices and both input gradients equal the CPU oracle
    (oracle/ref_ops.py, pinned to the same golden by tests/test_oracle_golden.py) under its autograd, on draws that cover
    angles from 1e-3 to ~2 rad and a batch of 12."""
    from oracle import ref_ops as R
    from ppeadepth import layers
    g = golden("layers_geometry")
    aa, tt = g["axisangle"], g["translation"]
    T = layers.transformation_from_parameters(aa.to(device), tt.to(device), invert)
    assert rel_err(T.cpu(), g["T_inv" if invert else "T_fwd"]) < 2e-6
    gen = _g(13 + int(invert))
    aa = (torch.randn(12, 1, 3, generator=gen) * torch.tensor([1e-3, 1e-2, 0.1, 1.0] * 3).view(12, 1, 1))
    tr = torch.randn(12, 1, 3, generator=gen)
    go = torch.randn(12, 4, 4, generator=gen)
    # (the oracle in fp64: at angles of 1e-3 rad the fp32 composite itself loses 3-4 digits of the axis-angle gradient
    # to the cancellations in Rodrigues' formula, so two fp32 evaluations agree only to ~3e-4)
    a0, t0 = aa.double().requires_grad_(True), tr.double().requires_grad_(True)
    T0 = R.transformation_from_parameters(a0, t0, invert)
    (T0 * go.double()).sum().backward()
    a1, t1 = aa.clone().to(device).requires_grad_(True), tr.clone().to(device).requires_grad_(True)
    assert layers.POSE_MATRIX_KERNEL
    T1 = layers.transformation_from_parameters(a1, t1, invert)
    (T1 * go.to(device)).sum().backward()
    assert (T1.detach().cpu().double() - T0.detach()).abs().max() < 2e-6
    assert rel_err(a1.grad.cpu(), a0.grad) < 5e-4 and rel_err(t1.grad.cpu(), t0.grad) < 1e-5


def test_adam_flat_scaled_divides_rank_summed_gradients(device):
    """Several ranks: the exchange leaves the SUM of the gradients over the ranks in the flat buffer and the Adam kernel
    multiplies by 1 / world as it reads them -- bit-identical to a separate scaling pass followed by the plain kernel."""
    from ppeadepth._abi import call, ptr, stream_ptr
    g = _g(6)
    n, n_lo, world = 5003, 1024, 8
    p0 = torch.randn(n, generator=g).to(device)
    res = []
    for fused in (False, True):
        P, M, V = p0.clone(), torch.zeros(n, device=device), torch.zeros(n, device=device)
        W16 = torch.empty(n_lo, device=device, dtype=torch.bfloat16)
        state = torch.tensor([0.0, 1e-3], device=device)
        gg = _g(7)
        for step in range(3):
            gsum = (torch.randn(n, generator=gg) * 3.0).to(device)
            state[0] += 1
            if fused:
                call("ppea_adam_flat_scaled_f32", ptr(P), ptr(gsum), ptr(M), ptr(V), ptr(W16), n, n_lo, ptr(state), 0.9, 0.999,
                     1e-8, 1.0 / world, stream_ptr())
            else:
                call("ppea_adam_flat_f32", ptr(P), ptr(gsum * (1.0 / world)), ptr(M), ptr(V), ptr(W16), n, n_lo, ptr(state), 0.9,
                     0.999, 1e-8, stream_ptr())
        res.append((P, M, V, W16))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (3, 16, 24, 80), (1, 4, 192, 640)])
def test_bias_elu(device, dtype, shape):
    """elu(z + b) in one pass; backward = dz and the bias gradient (per-plane partial sums)."""
    import torch.nn.functional as F
    from ppeadepth import ops
    g = _g(shape[1])
    z = torch.randn(shape, generator=g).to(dtype)
    b = torch.randn(shape[1], generator=g)
    go = torch.randn(shape, generator=g).to(dtype)
    zr, br = z.float().clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.elu(zr + br.view(1, -1, 1, 1))
    (ref * go.float()).sum().backward()
    zd, bd = z.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    y = ops.bias_elu(zd, bd)
    (y.float() * go.to(device).float()).sum().backward()
    tol = 2e-6 if dtype == torch.float32 else 1e-2
    assert rel_err(y.float().cpu(), ref.detach()) < tol
    assert rel_err(zd.grad.float().cpu(), zr.grad) < max(tol, 1e-5)
    assert rel_err(bd.grad.cpu(), br.grad) < (1e-4 if dtype == torch.float32 else 2e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("groups,act,res", [(1, 1, False), (2, 1, True), (2, 0, False), (1, 1, True)])
@pytest.mark.parametrize("shape", [(4, 64, 12, 20), (2, 256, 3, 5), (6, 16, 7, 9)])
def test_nhwc_bn_act(device, dtype, groups, act, res, shape):
    """Pose-trunk BatchNorm on channels_last data: per-sub-batch statistics, ReLU and residual-before-activation in
    the same pass, running statistics updated once per sub-batch in order; all gradients."""
    import torch.nn.functional as F
    from ppeadepth import ops
    N, C, H, W = shape
    g = _g(C + groups)
    x = (torch.randn(shape, generator=g) * 1.5 + 0.3).to(dtype)
    r = torch.randn(shape, generator=g).to(dtype)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    go = torch.randn(shape, generator=g).to(dtype)
    xr, rr = x.float().clone().requires_grad_(True), r.float().clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rm, rv = torch.zeros(C), torch.ones(C)
    outs = []
    for xc, rc in zip(xr.chunk(groups, 0), rr.chunk(groups, 0)):
        u = F.batch_norm(xc, rm, rv, wr, br, True, 0.1, 1e-5)
        if res:
            u = u + rc
        outs.append(F.relu(u) if act == 1 else u)
    ref = torch.cat(outs, 0)
    (ref * go.float()).sum().backward()
    cl = torch.channels_last
    xd = x.to(device).contiguous(memory_format=cl).requires_grad_(True)
    rd = r.to(device).contiguous(memory_format=cl).requires_grad_(True)
    wd, bd = w.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    rmd, rvd = torch.zeros(C, device=device), torch.ones(C, device=device)
    assert ops.nhwc_bn_supported(xd, groups)
    y, stats = ops.nhwc_bn_act(xd, wd, bd, rmd, rvd, rd if res else None, act, groups, 1e-5, 0.1)
    assert y.is_contiguous(memory_format=cl)
    (y.float() * go.to(device).float()).sum().backward()
    tf, tb = (3e-5, 3e-4) if dtype == torch.float32 else (1e-2, 3e-2)
    assert rel_err(y.float().cpu(), ref.detach()) < tf
    assert rel_err(rmd.cpu(), rm) < 1e-5 and rel_err(rvd.cpu(), rv) < 1e-4
    assert rel_err(xd.grad.float().cpu(), xr.grad) < tb
    assert rel_err(wd.grad.cpu(), wr.grad) < tb and rel_err(bd.grad.cpu(), br.grad) < tb
    if res:
        assert rel_err(rd.grad.float().cpu(), rr.grad) < tb


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 32, 7, 9), (1, 8, 3, 3), (2, 64, 24, 80), (1, 16, 3, 11)])
def test_decoder_passes_channels_last(device, dtype, shape):
    """ReflectionPad2d(1) and bias + ELU on channels_last tensors (decoder in NHWC): values, format and gradients."""
    import torch.nn.functional as F
    from ppeadepth import ops
    g = _g(shape[1] + shape[2])
    cl = torch.channels_last
    x = torch.randn(shape, generator=g).to(dtype)
    b = torch.randn(shape[1], generator=g)
    xr, br = x.float().clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.elu(F.pad(xr, (1, 1, 1, 1), mode="reflect") + br.view(1, -1, 1, 1))
    go = torch.randn(ref.shape, generator=g).to(dtype)
    (ref * go.float()).sum().backward()
    xd = x.to(device).contiguous(memory_format=cl).requires_grad_(True)
    bd = b.to(device).requires_grad_(True)
    p = ops.reflect_pad1(xd)
    assert p.is_contiguous(memory_format=cl) and p.shape == ref.shape
    y = ops.bias_elu(p, bd)
    assert y.is_contiguous(memory_format=cl)
    (y.float() * go.to(device).contiguous(memory_format=cl).float()).sum().backward()
    tol = 3e-6 if dtype == torch.float32 else 1e-2
    assert rel_err(y.float().cpu(), ref.detach()) < tol
    assert rel_err(xd.grad.float().cpu(), xr.grad) < max(tol, 2e-5)
    assert rel_err(bd.grad.cpu(), br.grad) < (1e-4 if dtype == torch.float32 else 2e-2)


# ---------------------------------------------------------------------------------------------
# A3-A6 in isolation: the product MODULES (not only their kernels) against the reference's own module outputs
# ---------------------------------------------------------------------------------------------
def _sub(g, prefix):
    return {n[len(prefix):]: v.clone() for n, v in g.items() if n.startswith(prefix)}


def test_replk_modules_vs_reference_golden(device, golden):
    """`RepLKBlock`, `ConvFFN`, `B_Adapter`, `Adapter` of this build, loaded with the reference modules' state_dicts,
    against the reference's outputs (tests/golden/replk_blocks.npz: blk:y, ffn:y, badpt:y, adpt:y) and the BN
    running statistics after one training forward (rka.py:283-289, 315-326)."""
    from ppeadepth.networks import replknet_adapter as rka
    g = golden("replk_blocks")
    x = g["badpt:x"].to(device)
    C = x.shape[1]
    ba = rka.B_Adapter(C, adpt_test=4, mlp_ratio=0.25)
    ba.load_state_dict(_sub(g, "badpt:sd:"))
    assert rel_err(ba.to(device)(x).cpu(), g["badpt:y"]) < 1e-4
    ad = rka.Adapter(C, adpt_test=4, mlp_ratio=0.25)
    ad.load_state_dict(_sub(g, "adpt:sd:"))
    assert rel_err(ad.to(device)(x).cpu(), g["adpt:y"]) < 1e-4
    blk = rka.RepLKBlock(C, C, 13, 5, drop_path=0.0, adpt_test=4, ratio=0.25)
    blk.load_state_dict(_sub(g, "blk:sd:"))
    blk.to(device).train()
    assert rel_err(blk(x).cpu(), g["blk:y"]) < 1e-4
    sd = blk.state_dict()
    for n, v in _sub(g, "blk:after:").items():
        assert rel_err(sd[n].cpu(), v) < 1e-4, n
    ffn = rka.ConvFFN(C, 4 * C, C, drop_path=0.0, adpt_test=4)
    ffn.load_state_dict(_sub(g, "ffn:sd:"))
    ffn.to(device).train()
    assert rel_err(ffn(x).cpu(), g["ffn:y"]) < 1e-4


def _l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("kind,C,K,H,W", [("blk", 64, 13, 6, 20), ("blk", 128, 31, 24, 40), ("ffn", 64, 0, 12, 40),
                                           ("ffn", 128, 0, 6, 20)])
def test_replk_modules_bf16_vs_oracle(device, kind, C, K, H, W):
    """The bf16 execution of a whole block (pwconv / dwconv_mfma / tapsum / pwgrad / fused BN kernels, adapter on a
    forked stream) against the fp32 CPU oracle on the same weights: output, input gradient, adapter weight gradients.

    Tolerances: the forward output sees ~6 chained bf16 roundings of O(1) activations -> 3e-2 of the tensor's max
    (measured 7e-3).  `ConvFFN` is smooth (GELU), so its gradients hold the same bound.  `RepLKBlock` has two ReLU
    gates: a pre-activation within 2^-9 of zero flips its gate under ANY bf16 execution and moves that gradient entry
    by 100 % (one such flip even separates two fp32 implementations: 0.2 in max-norm, 2e-2 in L2 at C=64, 6x20 --
    tools/debug_misc.py), so its gradients are compared in L2 and bounded by 1.5x the L2 error of torch's own bf16
    autocast of the same module (+ floor)."""
    import types
    from oracle import ref_model as RM, synth
    from ppeadepth import ops
    from ppeadepth.networks import replknet_adapter as rka
    B = 3

    def make():
        if kind == "blk":
            m = rka.RepLKBlock(C, C, K, 5, drop_path=0.0, adpt_test=4, ratio=0.25)
        else:
            m = rka.ConvFFN(C, 4 * C, C, drop_path=0.0, adpt_test=4)
        synth.fill_state_dict(m)
        return m
    m = make()
    sd = {"m." + k: v.clone() for k, v in m.state_dict().items()}
    names = [n for n, _ in m.named_parameters() if "adapter" in n]
    for n in names:
        sd["m." + n].requires_grad_(True)
    x = torch.randn(B, C, H, W, generator=_g(C + H))
    go = torch.randn(B, C, H, W, generator=_g(7))
    opt = types.SimpleNamespace(rep_size="b", g_blk=1.0, g_ffn=1.0, use_checkpoint=False)
    ref = RM.RefRepDepth(sd, opt)
    xr = x.clone().requires_grad_(True)
    yr = ref._replk_block(xr, "m", K, 0.0) if kind == "blk" else ref._conv_ffn(xr, "m", 0.0)
    yr.backward(go)

    def run():
        mod = make().to(device).train()
        for n, p in mod.named_parameters():
            p.requires_grad = "adapter" in n or ".bn" in n or "_bn" in n        # the Stage-1 freeze rule
        xd = x.to(device).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(xd.bfloat16())
        y.backward(go.to(device).bfloat16())
        params = dict(mod.named_parameters())
        return y, xd.grad, {n: params[n].grad for n in names}

    y, dx, dw = run()
    assert y.dtype == torch.bfloat16
    assert rel_err(y.float().cpu(), yr.detach()) < 3e-2
    if kind == "ffn":
        assert rel_err(dx.cpu(), xr.grad) < 3e-2
        for n in names:
            assert rel_err(dw[n].float().cpu(), sd["m." + n].grad) < 3e-2, n
        return
    saved = (rka.FUSE_BN, rka.PW_MFMA, rka.ADAPTER_MFMA, ops._MFMA_K)
    try:
        rka.FUSE_BN = rka.PW_MFMA = rka.ADAPTER_MFMA = False
        ops._MFMA_K = ()
        _, dx_t, dw_t = run()
    finally:
        rka.FUSE_BN, rka.PW_MFMA, rka.ADAPTER_MFMA, ops._MFMA_K = saved
    e, et = _l2(dx.cpu(), xr.grad), _l2(dx_t.cpu(), xr.grad)
    assert e < 1.5 * et + 1e-2 and e < 0.3, ("dx", e, et)
    for n in names:
        e, et = _l2(dw[n].float().cpu(), sd["m." + n].grad), _l2(dw_t[n].float().cpu(), sd["m." + n].grad)
        assert e < 1.5 * et + 1e-2 and e < 0.3, (n, e, et)


def test_structural_reparam_and_deep_fuse_bn_equivalence(device):
    """SURVEY 8(f)-4, the reference's own check (replknet.py:400-413): eval forward of a RepLKNet-adapter backbone before
    and after `structural_reparam()` (merged 31/29/27/13 convs with bias on the `dwconv_lk` kernel) and after
    `deep_fuse_BN()` (rka.py:563-580) gives the same four feature maps."""
    from oracle import synth
    from ppeadepth.networks import replknet_adapter as rka
    net = rka.RepLKNetAdapter([31, 29, 27, 13], [1, 1, 2, 1], [32, 64, 96, 128], 0.3, 5, num_classes=None,
                              out_indices=(0, 1, 2, 3), use_checkpoint=False, use_sync_bn=False, adpt_test=4)
    synth.fill_state_dict(net)
    net.to(device).eval()
    x = torch.rand(2, 3, 64, 96, generator=_g(3)).to(device)
    with torch.no_grad():
        base = [f.clone() for f in net(x)]
        net.structural_reparam()
        merged = [m for m in net.modules() if isinstance(m, rka.ReparamLargeKernelConv)]
        assert merged and all(type(m.lkb_reparam).__name__ == "LargeKernelDW" and m.lkb_reparam.bias is not None
                              for m in merged)
        after = net(x)
        for a, b in zip(after, base):
            assert rel_err(a, b) < 1e-4
        net.deep_fuse_BN()
        assert not any(isinstance(m[1], rka.BatchNorm2d) for m in net.modules()
                       if isinstance(m, torch.nn.Sequential) and len(m) in (2, 3) and hasattr(m[0], "kernel_size"))
        fused = net(x)
        for a, b in zip(fused, base):
            assert rel_err(a, b) < 1e-4


# ---------------------------------------------------------------------------------------------
# A12 / A14: dense convolutions on the implicit-GEMM MFMA kernels (conv_nhwc.hip / conv_wgrad.hip)
# ---------------------------------------------------------------------------------------------
CONV_CASES = [
    # name,            N, Cin, H,  W,  Cout, k, stride, pad, reflect, act,       bias,  nchw
    ("dec_32_32",      2, 32,  24, 40, 32,   3, 1,      1,   True,    "elu",     True,  False),
    ("dec_64_32_odd",  1, 64,  13, 21, 32,   3, 1,      1,   True,    "elu",     True,  False),
    ("dec_1024_512",   2, 1024, 6, 20, 512,  3, 1,      1,   True,    "elu",     True,  False),
    ("dec_256_128",    2, 256, 24, 16, 128,  3, 1,      1,   True,    "elu",     True,  False),
    ("disp_32_1",      2, 32,  16, 24, 1,    3, 1,      1,   True,    "sigmoid", True,  False),
    ("reduce_224_128", 2, 224, 12, 40, 128,  3, 1,      1,   False,   "relu",    True,  True),
    ("res_64_64",      3, 64,  12, 20, 64,   3, 1,      1,   False,   "none",    False, False),
    ("res_64_128_s2",  3, 64,  12, 20, 128,  3, 2,      1,   False,   "none",    False, False),
    ("res_64_128_s2o", 2, 64,  13, 19, 128,  3, 2,      1,   False,   "none",    False, False),
    ("down_64_128_s2", 3, 64,  12, 20, 128,  1, 2,      0,   False,   "none",    False, False),
    ("conv1_7x7_s2",   2, 8,   32, 48, 64,   7, 2,      3,   False,   "none",    False, False),
    ("stem_3x3_s2",    2, 8,   32, 48, 128,  3, 2,      1,   False,   "none",    False, True),
    ("squeeze_1x1",    4, 512, 6,  20, 256,  1, 1,      0,   False,   "relu",    True,  False),
    ("posehead_12",    4, 256, 6,  20, 12,   1, 1,      0,   False,   "none",    True,  False),
    # >= 2048 tiles of 8x16 pixels, <= 64 channels: the persistent kernel with the weights resident in LDS (forward and,
    # with the flipped weights / the zero-padded full correlation of the reflection case, the data gradient)
    ("big_32_32_ragged", 3, 32, 190, 630, 32, 3, 1,     1,   True,    "elu",     True,  False),
    ("big_32_1",       3, 32,  192, 640, 1,  3, 1,      1,   True,    "sigmoid", True,  False),
    ("big_64_48",      3, 64,  190, 630, 48, 3, 1,      1,   False,   "none",    False, False),
    ("big_40_16",      3, 40,  192, 640, 16, 3, 1,      1,   False,   "relu",    True,  False),
    # the two decoder layers whose weight-gradient plan takes the "fill" splits beyond the 32 MB workspace cap (9-16 slabs,
    # flat slab reduction; conv_wgrad.hip plan()), at the benchmarked batch and map size
    ("wgrad_512_256_fill", 12, 512, 24, 80, 256, 3, 1,  1,   True,    "elu",     True,  False),
    ("wgrad_256_128_fill", 12, 256, 48, 160, 128, 3, 1, 1,   True,    "elu",     True,  False),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv2d_nhwc_mfma(device, case):
    """Forward, data gradient, weight gradient and bias gradient of the implicit-GEMM convolution kernels against a
    plain fp32 PyTorch reference of the same op on the same bf16-rounded operands (reflection / zero padding, stride
    1 / 2, 1x1 / 3x3 / 7x7, fused bias + ReLU / ELU / sigmoid, channels_last and NCHW outputs, ragged sizes) at the layer
    shapes of the step, one max-norm figure per tensor.  The per-element bound, the float64 reference and a row for every
    instantiation and plan outcome of these kernels are in tests/test_conv_arms_gpu.py (tables: oracle/conv_inputs.py)."""
    import torch.nn.functional as F
    from ppeadepth import ops
    name, N, Cin, H, W, Cout, k, stride, pad, reflect, act, has_bias, nchw = case
    g = _g(len(name) * 7 + Cin)
    x = torch.randn(N, Cin, H, W, generator=g).bfloat16()
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).bfloat16()
    b = (0.2 * torch.randn(Cout, generator=g)).bfloat16() if has_bias else None

    def ref(xr, wr, br):
        xp = F.pad(xr, (pad,) * 4, mode="reflect") if reflect else xr
        z = F.conv2d(xp, wr, br, stride, 0 if reflect else pad)
        return {"none": z, "relu": F.relu(z), "elu": F.elu(z), "sigmoid": torch.sigmoid(z)}[act]
    leaves = [t.float().clone().requires_grad_(True) if t is not None else None for t in (x, w, b)]
    yr = ref(*leaves)
    go = torch.randn(yr.shape, generator=g).bfloat16()
    yr.backward(go.float())

    xd = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = w.to(device).requires_grad_(True)
    bd = b.to(device).requires_grad_(True) if has_bias else None
    assert ops.conv_supported(xd, wd)
    y = ops.conv2d_nhwc(xd, wd, bd, stride, pad, reflect, act, nchw)
    assert y.shape == yr.shape and y.dtype == torch.bfloat16
    assert y.is_contiguous() if nchw else (Cout % 8 != 0 or y.is_contiguous(memory_format=torch.channels_last))
    y.backward(go.to(device))
    tol = 2 ** -7
    assert rel_err(y.float().cpu(), yr.detach()) < tol
    if Cin != 8:                                    # the image-fed layers (stem, pose conv1) need no data gradient
        assert rel_err(xd.grad.float().cpu(), leaves[0].grad) < tol
    assert rel_err(wd.grad.float().cpu(), leaves[1].grad) < tol
    if has_bias:
        assert rel_err(bd.grad.float().cpu(), leaves[2].grad) < tol


def test_image_to_nhwc_and_conv_full_size(device):
    """The two image-fed layers at full size: the fp32 NCHW frames are normalised, padded to 8 channels and laid out
    channels_last by one kernel (resnet_encoder.py:399 `(x - 0.45) / 0.225`), then convolved."""
    import torch.nn.functional as F
    from ppeadepth import ops
    g = _g(5)
    img = torch.rand(2, 6, 192, 640, generator=g)
    w = (torch.randn(64, 6, 7, 7, generator=g) / 17).bfloat16()
    xn = ops.image_to_nhwc(img.to(device), 8, 0.45, 0.225)
    want = ((img - 0.45) / 0.225).bfloat16()
    assert torch.equal(xn[:, :6].cpu().float(), want.float()) and float(xn[:, 6:].abs().max()) == 0.0
    w8 = torch.cat([w, torch.zeros(64, 2, 7, 7, dtype=torch.bfloat16)], 1).to(device)
    y = ops.conv2d_nhwc(xn, w8, None, 2, 3)
    yr = F.conv2d(want.float(), w.float(), None, 2, 3)
    assert rel_err(y.float().cpu(), yr) < 2 ** -7


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("two,act,res", [(False, 0, False), (False, 1, False), (True, 1, False), (False, 2, False),
                                         (False, 0, True), (True, 1, True)])
@pytest.mark.parametrize("shape", [(12, 64, 12, 40), (3, 128, 6, 24), (5, 64, 6, 20), (12, 96, 4, 8)])
def test_bn_channel_one_launch(device, dtype, two, act, res, shape):
    """Small channels: statistics + running-statistics update + apply in ONE launch (and reduce + apply in one launch
    backward) -- forward, saved statistics, running statistics and every gradient against the fp32 oracle composite
    (the same reference as test_fused_bn_act)."""
    import torch.nn.functional as F
    from ppeadepth import ops
    from ppeadepth.batchnorm import BatchNorm2d
    N, C, H, W = shape
    g = _g(N * 100 + C + act)
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    z1 = (torch.randn(shape, generator=g) * 2 + 0.5).to(dt)
    z2 = (torch.randn(shape, generator=g) * 0.7 - 0.2).to(dt)
    g1, b1 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    g2, b2 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    mask = torch.tensor(([0.0] + [1.4] * N)[:N])
    r1 = torch.randn(shape, generator=g).to(dt)
    r2 = torch.randn(shape, generator=g).to(dt)
    go = torch.randn(shape, generator=g).to(dt)
    leaves = [t.float().clone().requires_grad_(True) for t in (z1, z2, g1, b1, g2, b2, r1, r2)]
    a, bb, w1, c1, w2, c2, q1, q2 = leaves
    rm_ref, rv_ref, rm2_ref, rv2_ref = torch.zeros(C), torch.ones(C), torch.zeros(C), torch.ones(C)
    u = F.batch_norm(a, rm_ref, rv_ref, w1, c1, True, 0.1, 1e-5)
    if two:
        u = u + F.batch_norm(bb, rm2_ref, rv2_ref, w2, c2, True, 0.1, 1e-5)
    u = F.relu(u) if act == 1 else (F.gelu(u) if act == 2 else u)
    if res:
        u = u * mask.view(-1, 1, 1, 1) + q1 + 0.5 * q2
    (u * go.float()).sum().backward()

    bn1, bn2 = BatchNorm2d(C).to(device), BatchNorm2d(C).to(device)
    with torch.no_grad():
        bn1.weight.copy_(g1); bn1.bias.copy_(b1); bn2.weight.copy_(g2); bn2.bias.copy_(b2)
    d = [t.to(device).requires_grad_(True) for t in (z1, z2, r1, r2)]
    assert ops.bn_channel_ok(d[0])
    kw = dict(z2=d[1], bn2=bn2) if two else {}
    if res:
        kw.update(mask=mask.to(device), r1=d[2], r2=d[3], r2_scale=0.5)
    y, st = ops.bn_act_channel(d[0], bn1, act=act, **kw)
    (y.float() * go.to(device).float()).sum().backward()
    tol_f, tol_b = (2e-5, 2e-4) if dtype == "f32" else (1e-2, 3e-2)
    assert rel_err(y.float().cpu(), u.detach()) < tol_f
    assert rel_err(bn1.running_mean.cpu(), rm_ref) < 1e-5 and rel_err(bn1.running_var.cpu(), rv_ref) < 1e-4
    zf = z1.float()
    assert rel_err(st[0].cpu(), zf.mean((0, 2, 3))) < 1e-5
    assert rel_err(st[1].cpu(), (zf.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()) < 1e-5
    assert rel_err(d[0].grad.float().cpu(), a.grad) < tol_b
    assert rel_err(bn1.weight.grad.cpu(), w1.grad) < tol_b and rel_err(bn1.bias.grad.cpu(), c1.grad) < tol_b
    if two:
        assert rel_err(bn2.running_var.cpu(), rv2_ref) < 1e-4
        assert rel_err(d[1].grad.float().cpu(), bb.grad) < tol_b
        assert rel_err(bn2.weight.grad.cpu(), w2.grad) < tol_b and rel_err(bn2.bias.grad.cpu(), c2.grad) < tol_b
    if res:
        assert rel_err(d[2].grad.float().cpu(), q1.grad) < tol_b and rel_err(d[3].grad.float().cpu(), q2.grad) < tol_b


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bn_channel_skip_gradient_is_added_in_the_backward_launch(device, dtype):
    """A block's input feeds its pre-BN AND its residual connection (rka.py:283-289, 315-326).  With `skip=True` the
    BN returns the input once more for the residual use and adds that use's gradient inside its one backward launch:
    bit-identical to autograd's separate element-wise add (the BN gradient is rounded to the storage type first, as
    a stored dz would be), and the autograd graph holds no add node for x."""
    from ppeadepth import ops
    from ppeadepth.batchnorm import BatchNorm2d, fused_bn_act
    shape = (12, 64, 12, 40)
    g = _g(77)
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    x0 = (torch.randn(shape, generator=g) * 2 + 0.5).to(dt).to(device)
    go = torch.randn(shape, generator=g).to(dt).to(device)
    gs = torch.randn(shape, generator=g).to(dt).to(device)
    grads = []
    for skip in (False, True):
        bn = BatchNorm2d(64).to(device)
        leaf = x0.clone().requires_grad_(True)
        x = leaf * 1                                           # a non-leaf input, like a block's
        if skip:
            y, xs = fused_bn_act(x, bn, skip=True)
            assert xs.grad_fn is y.grad_fn and xs.data_ptr() == x.data_ptr()
        else:
            y, xs = fused_bn_act(x, bn), x
        ((y * go).sum() + (xs * gs).sum()).backward()
        grads.append((leaf.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 6, 10, 24), (3, 64, 12, 40, 0), (2, 8, 3, 5, 8)])
def test_upsample2x_cat_one_pass(device, dtype, shape):
    """Decoder glue (depth_decoder_v2.py:231-236): nearest 2x upsampling + skip concatenation in one launch, and the
    split + 2x2 block sum backward in one launch -- exact against F.interpolate / torch.cat and their autograd
    (copies forward; backward sums four values in fp32 and rounds once, like upsample_nearest2d_backward)."""
    import torch.nn.functional as F
    from ppeadepth import ops
    from ppeadepth.layers import upsample_cat
    N, C1, h, w, C2 = shape
    g = _g(N * 1000 + C1 + C2)
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    a0 = torch.randn(N, C1, h, w, generator=g).to(dt).to(device).contiguous(memory_format=torch.channels_last)
    b0 = None if C2 == 0 else torch.randn(N, C2, 2 * h, 2 * w, generator=g).to(dt).to(device).contiguous(
        memory_format=torch.channels_last)
    go = torch.randn(N, C1 + C2, 2 * h, 2 * w, generator=g).to(dt).to(device).contiguous(memory_format=torch.channels_last)
    res = []
    for fused in (False, True):
        a = a0.clone().requires_grad_(True)
        b = None if b0 is None else b0.clone().requires_grad_(True)
        if fused:
            assert ops.up2cat_supported(a, b)
            y = upsample_cat(a, b)
            assert y.is_contiguous(memory_format=torch.channels_last)
        else:
            y = F.interpolate(a, scale_factor=2, mode="nearest")
            y = y if b is None else torch.cat([y, b], 1)
        (y * go).sum().backward()
        res.append((y.detach(), a.grad, None if b is None else b.grad))
    assert torch.equal(res[0][0], res[1][0])
    if dtype == "f32":
        assert rel_err(res[1][1], res[0][1]) < 1e-6          # summation order inside the 2x2 block
    else:
        assert rel_err(res[1][1].float(), res[0][1].float()) < 2 ** -8
    if C2:
        assert torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("shape", [(12, 128, 48, 160, 512), (3, 256, 24, 88, 96), (2, 64, 40, 72, 32), (12, 512, 48, 160, 128)])
def test_pwconv_epilogue_sums_give_the_batchnorm_statistics(device, shape):
    """BatchNorm statistics from the producing 1x1 conv's epilogue (conv_bn / conv_bn_relu, rka.py:182-197): same output
    bytes as the plain launch; per-channel (sum, sum of squares) partials whose fp64 totals give mean / biased variance /
    invstd of the STORED bf16 tensor to 1e-6 relative, and the running statistics F.batch_norm would leave (ragged last
    pixel tile, channel counts that do not fill a workgroup tile, all three tile configurations)."""
    import torch.nn.functional as F
    from ppeadepth import ops
    B, K, H, W, M = shape
    g = _g(B * 10 + M)
    x = torch.randn(B, K, H, W, generator=g).bfloat16().to(device)
    w = (torch.randn(M, K, 1, 1, generator=g) / K ** 0.5 + 0.02).bfloat16().to(device)
    y0 = ops.pwconv_frozen(x, w)
    y, sums = ops.pwconv_frozen(x, w, want_sums=True)
    assert torch.equal(y, y0) and sums.shape[0] == M and sums.shape[2] == 2 and torch.isfinite(sums).all()
    rm, rv = torch.zeros(M, device=device), torch.ones(M, device=device)
    mean, var, invstd = ops.bn_batch_stats_from_sums(sums, B * H * W, 1e-5, 0.1, rm, rv)
    yf = y.float()
    rm_ref, rv_ref = torch.zeros(M, device=device), torch.ones(M, device=device)
    F.batch_norm(yf, rm_ref, rv_ref, None, None, True, 0.1, 1e-5)
    want_mean, want_var = yf.double().mean((0, 2, 3)), yf.double().var((0, 2, 3), unbiased=False)
    assert rel_err(mean.cpu(), want_mean.cpu()) < 1e-6 and rel_err(var.cpu(), want_var.cpu()) < 1e-5
    assert rel_err(invstd.cpu(), (want_var + 1e-5).rsqrt().cpu()) < 1e-5
    assert rel_err(rm.cpu(), rm_ref.cpu()) < 1e-5 and rel_err(rv.cpu(), rv_ref.cpu()) < 1e-5


@pytest.mark.parametrize("shape", [(12, 128, 48, 160, 31), (12, 256, 24, 80, 29), (3, 64, 20, 36, 13), (12, 512, 12, 40, 27),
                                   (20, 6, 6, 20, 13)])
def test_dwconv_epilogue_sums_give_both_batchnorm_statistics(device, shape):
    """The large-kernel depthwise conv's epilogue returns per-channel partial sums of BOTH outputs (k x k and 5 x 5 branch,
    rka.py:232-239): same output bytes as the plain launch, and statistics of the stored bf16 tensors to 1e-6 / 1e-5."""
    from ppeadepth import ops
    N, C, H, W, K = shape
    g = _g(N + C + K)
    x = torch.randn(N, C, H, W, generator=g).bfloat16().to(device)
    wb = (torch.randn(C, 1, K, K, generator=g) / K).to(device)
    ws = (torch.randn(C, 1, 5, 5, generator=g) / 5).to(device)
    yb0, ys0 = ops.dwconv_lk(x, wb, ws)
    yb, ys, sums = ops.dwconv_lk(x, wb, ws, want_sums=True)
    assert sums is not None and torch.equal(yb, yb0) and torch.equal(ys, ys0)
    for y, s in ((yb, sums[0]), (ys, sums[1])):
        mean, var, invstd = ops.bn_batch_stats_from_sums(s.contiguous(), N * H * W, 1e-5, 0.1, None, None)
        yf = y.double()
        assert rel_err(mean.cpu(), yf.mean((0, 2, 3)).cpu()) < 1e-6
        assert rel_err(var.cpu(), yf.var((0, 2, 3), unbiased=False).cpu()) < 1e-5


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_bn_channel_next_kernels_are_bit_identical_to_two_launches(device, dtype):
    """Kernel level, both dtypes: y, y2 = bn_act_channel_next(z, A, B, mask, r1, r2) against bn_act_channel(z, A, ...)
    followed by fused_bn_act(y, B, skip=True) -- outputs, every gradient (z, r1, r2, both BNs' affine parameters) and the
    running statistics must agree BITWISE, with and without a gradient arriving at y through another consumer."""
    from ppeadepth import ops
    from ppeadepth.batchnorm import BatchNorm2d, fused_bn_act
    shape = (5, 64, 6, 20)
    g = _g(123)
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    z0 = (torch.randn(shape, generator=g) * 2 + 0.5).to(dt).to(device)
    r10, r20 = torch.randn(shape, generator=g).to(dt).to(device), torch.randn(shape, generator=g).to(dt).to(device)
    go2, goy = torch.randn(shape, generator=g).to(dt).to(device), torch.randn(shape, generator=g).to(dt).to(device)
    mask = torch.tensor([0.0, 1.25, 1.25, 0.0, 1.25], device=device)
    res = []
    for merged in (False, True):
        bnA, bnB = BatchNorm2d(64).to(device), BatchNorm2d(64).to(device)
        with torch.no_grad():
            bnA.weight.copy_(torch.rand(64, generator=_g(1)) + 0.5); bnA.bias.copy_(torch.randn(64, generator=_g(2)) * 0.2)
            bnB.weight.copy_(torch.rand(64, generator=_g(3)) + 0.5); bnB.bias.copy_(torch.randn(64, generator=_g(4)) * 0.2)
        z, r1, r2 = (t.clone().requires_grad_(True) for t in (z0, r10, r20))
        if merged:
            y, y2, _ = ops.bn_act_channel_next(z, bnA, bnB, mask=mask, r1=r1, r2=r2, r2_scale=0.5)
            ys = y
        else:
            y, _ = ops.bn_act_channel(z, bnA, mask=mask, r1=r1, r2=r2, r2_scale=0.5)
            y2, ys = fused_bn_act(y, bnB, skip=True)
        ((y2 * go2).sum() + (ys * goy).sum()).backward()
        res.append([y.detach(), y2.detach(), z.grad, r1.grad, r2.grad, bnA.weight.grad, bnA.bias.grad, bnB.weight.grad,
                    bnB.bias.grad, bnA.running_mean, bnA.running_var, bnB.running_mean, bnB.running_var])
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), i


def test_block_chain_last_bn_plus_next_pre_bn_is_bit_identical(device, dtype="bf16"):
    """fused_bn_act_next: a block's last BatchNorm (+ DropPath + residual + adapter) and the next block's first BatchNorm
    as ONE launch per direction.  A whole stage (2 RepLK + 2 ConvFFN blocks, DropPath on, adapters on) run with and
    without the chaining must agree BITWISE: output, input gradient, every parameter gradient, every running statistic."""
    from oracle import synth
    from ppeadepth import batchnorm, rng
    from ppeadepth.networks import replknet_adapter as rka
    C, K, H, W, B = 128, 13, 12, 20, 3          # hidden = 32: the adapters run on the MFMA kernels (deterministic), not the library

    def run(chain):
        saved = batchnorm.BN_CHAIN
        batchnorm.BN_CHAIN = chain
        try:
            st = rka.RepLKNetStage(C, 2, K, [0.1, 0.2], 5, adpt_test=4, ratio=0.25)
            synth.fill_state_dict(st)
            st = st.to(device).train()
            for n, p in st.named_parameters():
                p.requires_grad = "adapter" in n or ".bn" in n or "_bn" in n
            g = _g(5)
            x = torch.randn(B, C, H, W, generator=g).to(device).requires_grad_(True)
            go = torch.randn(B, C, H, W, generator=g).to(device)
            rng.set_mode("reference")
            torch.manual_seed(11)
            if dtype == "bf16":
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = st(x.bfloat16())
                y.backward(go.bfloat16())
            else:
                y = st(x)
                y.backward(go)
            torch.cuda.synchronize()
            grads = {n: p.grad for n, p in st.named_parameters() if p.grad is not None}
            return y.detach(), x.grad, grads, {n: b.clone() for n, b in st.named_buffers()}
        finally:
            batchnorm.BN_CHAIN = saved
            rng.set_mode("device")

    a, b = run(False), run(True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) > 20
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n
    for n in a[3]:
        assert torch.equal(a[3][n], b[3][n]), n


@pytest.mark.parametrize("dtype,shape", [("bf16", (128, 13, 12, 20, 3)), ("f32", (128, 13, 12, 20, 3)), ("f32", (64, 27, 12, 40, 5)),
                                         ("bf16", (64, 27, 12, 40, 12))])
@pytest.mark.parametrize("chain", [True, False])
def test_bn_second_consumer_gradient_added_in_the_backward_launch_is_bit_identical(device, chain, dtype, shape):
    """A block's first BatchNorm output feeds its first 1x1 conv and its adapter.  With BN_DUP the adapter reads an alias whose
    gradient reaches the BatchNorm's backward launch separately and is added there (round(dy + dyb), then the usual
    arithmetic) instead of by autograd's own element-wise kernel: a whole stage must agree BITWISE with and without it --
    output, input gradient, every parameter gradient, every running statistic -- and launch fewer add kernels."""
    from oracle import synth
    from torch.profiler import ProfilerActivity, profile
    from ppeadepth import batchnorm, rng
    from ppeadepth.networks import replknet_adapter as rka
    C, K, H, W, B = shape

    def run(dup):
        saved = (batchnorm.BN_DUP, batchnorm.BN_CHAIN, rka.ADAPTER_STREAMS)
        batchnorm.BN_DUP, batchnorm.BN_CHAIN = dup, chain
        rka.ADAPTER_STREAMS = False            # the alias is handed to adapters that run in line (the teacher's), see rka.ConvFFN.forward
        try:
            st = rka.RepLKNetStage(C, 2, K, [0.1, 0.2], 5, adpt_test=4, ratio=0.25)
            synth.fill_state_dict(st)
            st = st.to(device).train()
            for n, p in st.named_parameters():
                p.requires_grad = "adapter" in n or ".bn" in n or "_bn" in n
            g = _g(5)
            x = torch.randn(B, C, H, W, generator=g).to(device).requires_grad_(True)
            go = torch.randn(B, C, H, W, generator=g).to(device)
            rng.set_mode("reference")
            torch.manual_seed(11)
            with profile(activities=[ProfilerActivity.CPU]) as prof:
                if dtype == "bf16":
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        y = st(x.bfloat16())
                    y.backward(go.bfloat16())
                else:
                    y = st(x)
                    y.backward(go)
            torch.cuda.synchronize()
            adds = sum(1 for e in prof.events() if e.name in ("aten::add_", "aten::add"))
            grads = {n: p.grad for n, p in st.named_parameters() if p.grad is not None}
            return y.detach(), x.grad, grads, {n: b.clone() for n, b in st.named_buffers()}, adds
        finally:
            batchnorm.BN_DUP, batchnorm.BN_CHAIN, rka.ADAPTER_STREAMS = saved
            rng.set_mode("device")

    a, b = run(False), run(True)
    # fp32: the adapters' convolutions run in the library, whose weight-gradient kernels do not sum in a fixed order
    same = torch.equal if dtype == "bf16" else (lambda u, v: rel_err(u, v) < 1e-5)
    assert same(a[0], b[0]) and same(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) > 20
    for n in a[2]:
        assert same(a[2][n], b[2][n]), n
    for n in a[3]:
        assert same(a[3][n], b[3][n]), n
    assert b[4] <= a[4] - 3, (a[4], b[4])              # 4 blocks: at least 3 element-wise adds gone


# bf16 large-kernel arm (statistics from the 1x1 conv's epilogue sums of bf16-stored values): twice the error measured
# against the fp64 composite before the bookkeeping was unified (running mean, running variance)
LK_BOOK_MEASURED = (2.547e-3, 2.891e-4)
LK_BOOK_TOL = tuple(2 * e for e in LK_BOOK_MEASURED)


@pytest.mark.parametrize("grad", [True, False])
@pytest.mark.parametrize("arm", ["channel", "channel_pair", "general_one_launch", "general_partials", "next", "large_kernel"])
def test_bn_front_end_books_the_checkpoint_replay(device, arm, grad):
    """Every arm of the BatchNorm front end with a deferred book active and replay_update set, then flush(): the
    reference's reentrant checkpoint runs a block twice on the same batch, so num_batches_tracked == 2 and the running
    statistics are those of torch.nn.BatchNorm2d (fp64, CPU) after two passes.  Under no_grad (the lookup frames) the call
    is counted once."""
    from ppeadepth import ops
    from ppeadepth.batchnorm import BatchNorm2d, DeferredStats, fused_bn_act, fused_bn_act_next, set_deferred
    from ppeadepth.networks import replknet_adapter as rka
    g = _g(41)

    def mk_bn(C):
        bn = BatchNorm2d(C).to(device).train()
        bn.replay_update = True
        with torch.no_grad():
            bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(C, generator=g) * 0.2)
        return bn

    def draw(shape):
        return torch.randn(shape, generator=g) * 2 + 0.5

    def ref_twice(bn, z64):
        ref = torch.nn.BatchNorm2d(bn.num_features).double().train()
        with torch.no_grad():
            ref.weight.copy_(bn.weight.detach().cpu())
            ref.bias.copy_(bn.bias.detach().cpu())
            y = ref(z64)
            ref(z64)
        return ref, y

    shape = {"general_one_launch": (2, 5, 7, 9), "general_partials": (2, 4, 48, 160), "large_kernel": (3, 64, 20, 36)}.get(
        arm, (2, 64, 4, 8))
    C = shape[1]
    tol = (1e-5, 1e-4)
    counted = []                                   # further BatchNorms whose calls are only counted here
    book = DeferredStats()
    set_deferred(book)
    try:
        with torch.set_grad_enabled(grad):
            if arm == "large_kernel":
                blk = rka.RepLKBlock(C, C, 13, 5, 0.0, adpt_test=-1).to(device).train()
                x = torch.randn(shape, generator=g).bfloat16()
                w = torch.randn(C, C, 1, 1, generator=g) / C ** 0.5
                with torch.no_grad():
                    blk.pw1.conv.weight.copy_(w)
                    blk.pw1.bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
                for p in blk.parameters():
                    p.requires_grad = p.dim() == 1
                for m in blk.modules():
                    if isinstance(m, BatchNorm2d):
                        m.replay_update = True
                assert blk._pw1_large_kernel_fused(x.to(device)) is not None
                pairs = [(blk.pw1.bn, F.conv2d(x.double(), w.double()))]
                counted = [blk.large_kernel.lkb_origin.bn, blk.large_kernel.small_conv.bn]
                tol = LK_BOOK_TOL
            elif arm == "next":
                z, bnA, bnB = draw(shape), mk_bn(C), mk_bn(C)
                assert fused_bn_act_next(z.to(device), bnA, bnB) is not None
                pairs = [(bnA, z.double())]
                pairs.append((bnB, ref_twice(bnA, z.double())[1]))
            elif arm == "channel_pair":
                z1, z2, bn1, bn2 = draw(shape), draw(shape), mk_bn(C), mk_bn(C)
                assert ops.bn_channel_ok(z1.to(device))
                fused_bn_act(z1.to(device), bn1, z2.to(device), bn2, act=ops.ACT_RELU)
                pairs = [(bn1, z1.double()), (bn2, z2.double())]
            else:
                z, bn = draw(shape), mk_bn(C)
                assert ops.bn_channel_ok(z.to(device)) == (arm == "channel")
                fused_bn_act(z.to(device), bn, act=ops.ACT_RELU)
                pairs = [(bn, z.double())]
    finally:
        set_deferred(None)
    for bn in [p[0] for p in pairs] + counted:
        assert int(bn.num_batches_tracked) == 0            # deferred: nothing counted before the flush
    book.flush()
    for bn in [p[0] for p in pairs] + counted:
        assert int(bn.num_batches_tracked) == (2 if grad else 1)
    if not grad:
        return
    for k, (bn, z64) in enumerate(pairs):
        ref, _ = ref_twice(bn, z64)
        em, ev = rel_err(bn.running_mean.cpu(), ref.running_mean), rel_err(bn.running_var.cpu(), ref.running_var)
        print(f"bn book {arm}[{k}]: running mean {em:.3e} running var {ev:.3e}")
        assert int(ref.num_batches_tracked) == 2
        assert em < tol[0] and ev < tol[1], (arm, k, em, ev)


# ---- round 3: the remaining library holes ---------------------------------------------------------------
@pytest.mark.parametrize("kind,C,hidden", [("mlp", 192, 48), ("conv", 192, 48), ("mlp", 128, 148), ("conv", 64, 20)])
def test_adapters_with_ragged_hidden_width_run_on_the_mfma_kernels(device, kind, C, hidden):
    """Hidden widths that are not a multiple of 32 (RepLKNet-31L stage 0: 48; the Stage-2 decoder adapter: 148) are
    zero-padded to the next multiple: same function and gradients as the fp32 composite of the bf16-rounded operands."""
    import torch.nn.functional as F
    from ppeadepth import ops
    B, H, W = 2, 12, 40
    g = _g(C + hidden)
    x = torch.randn(B, C, H, W, generator=g).bfloat16()
    w1 = (torch.randn((hidden, C, 3, 3) if kind == "conv" else (hidden, C), generator=g) / (C * (9 if kind == "conv" else 1)) ** 0.5).bfloat16()
    b1 = (torch.randn(hidden, generator=g) * 0.1).bfloat16()
    w2 = (torch.randn(C, hidden, generator=g) / hidden ** 0.5).bfloat16()
    b2 = (torch.randn(C, generator=g) * 0.1).bfloat16()
    go = torch.randn(B, C, H, W, generator=g).bfloat16()
    ref_leaves = [t.float().clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    xr, w1r, b1r, w2r, b2r = ref_leaves
    pre = F.conv2d(xr, w1r, b1r, padding=1) if kind == "conv" else torch.einsum("mk,bkhw->bmhw", w1r, xr) + b1r.view(1, -1, 1, 1)
    yr = torch.einsum("mk,bkhw->bmhw", w2r, F.gelu(pre)) + b2r.view(1, -1, 1, 1)
    (yr * go.float()).sum().backward()
    leaves = [t.to(device).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    assert ops.adapter_supported(leaves[0], hidden)
    y = (ops.conv_adapter if kind == "conv" else ops.mlp_adapter)(*leaves)
    (y.float() * go.to(device).float()).sum().backward()
    assert (y.float().cpu() - yr.detach()).abs().max() <= yr.abs().max() * 2 ** -6
    for mine, ref in zip(leaves, ref_leaves):
        assert mine.grad.shape == ref.grad.shape
        assert (mine.grad.float().cpu() - ref.grad).abs().max() <= ref.grad.abs().max() * 2 ** -5, mine.shape


def test_pw_linear_trainable_forward_and_gradients(device):
    from ppeadepth import ops
    B, K, M, H, W = 3, 128, 160, 12, 40
    g = _g(7)
    x = torch.randn(B, K, H, W, generator=g).bfloat16()
    w = (torch.randn(M, K, generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(M, generator=g).bfloat16()
    go = torch.randn(B, M, H, W, generator=g).bfloat16()
    xr, wr, br = (t.float().clone().requires_grad_(True) for t in (x, w, b))
    yr = torch.einsum("mk,bkhw->bmhw", wr, xr) + br.view(1, -1, 1, 1)
    (yr * go.float()).sum().backward()
    xd, wd, bd = (t.to(device).requires_grad_(True) for t in (x, w, b))
    assert ops.pw_linear_supported(xd, M)
    y = ops.pw_linear(xd, wd, bd)
    (y.float() * go.to(device).float()).sum().backward()
    assert (y.float().cpu() - yr.detach()).abs().max() <= yr.abs().max() * 2 ** -7
    for mine, ref in ((xd, xr), (wd, wr), (bd, br)):
        assert (mine.grad.float().cpu() - ref.grad).abs().max() <= ref.grad.abs().max() * 2 ** -6


@pytest.mark.parametrize("N,C,H,W", [(2, 32, 48, 160), (1, 32, 5, 7), (2, 64, 12, 16)])
def test_conv_transpose_on_the_implicit_gemm_kernels(device, N, C, H, W):
    """ConvTranspose2d(C, C, 3, stride 2, padding 1, output_padding 1) (depth_decoder_v2.py:137-139): forward = the data
    gradient kernel of a stride-2 conv, data gradient = that conv's forward, weight gradient = its weight gradient with
    the activations exchanged; against torch's fp32 ConvTranspose2d on the bf16-rounded operands."""
    import torch.nn as nn
    from ppeadepth import ops
    g = _g(N * 100 + C + H)
    m = nn.ConvTranspose2d(C, C, 3, 2, 1, output_padding=1)
    with torch.no_grad():
        m.weight.copy_((torch.randn(m.weight.shape, generator=g) / (9 * C) ** 0.5).bfloat16().float())
        m.bias.copy_((torch.randn(C, generator=g) * 0.1).bfloat16().float())
    x = torch.randn(N, C, H, W, generator=g).bfloat16()
    go = torch.randn(N, C, 2 * H, 2 * W, generator=g).bfloat16()
    xr = x.float().clone().requires_grad_(True)
    yr = m(xr)
    (yr * go.float()).sum().backward()
    ref = (yr.detach(), xr.grad.clone(), m.weight.grad.clone(), m.bias.grad.clone())
    md = nn.ConvTranspose2d(C, C, 3, 2, 1, output_padding=1).to(device)
    md.load_state_dict(m.state_dict())
    md = md.bfloat16()
    xd = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.conv_transpose_module(md, xd)
    assert y is not None and tuple(y.shape) == (N, C, 2 * H, 2 * W)
    (y.float() * go.to(device).float()).sum().backward()
    got = (y.float().cpu(), xd.grad.float().cpu(), md.weight.grad.float().cpu(), md.bias.grad.float().cpu())
    for a, b in zip(got, ref):
        assert a.shape == b.shape and (a - b).abs().max() <= b.abs().max() * 2 ** -6


def test_decoder_adapter_split_equals_the_concatenated_form(device):
    """Adapter(cat([f0, up8(f3)])) == W1a f0 + up8(W1b f3) (+ GELU, D_fc2): the bf16 HIP form against the module's fp32
    forward on the same (bf16-rounded) parameters, values and all parameter / input gradients."""
    import torch.nn.functional as F
    from ppeadepth.networks.depth_decoder_v2 import Adapter
    B, Cf, Cc, h, w = 2, 128, 1024, 6, 16
    g = _g(3)
    ad = Adapter(Cf + Cc, 32)
    with torch.no_grad():
        for p in ad.parameters():
            p.copy_((torch.randn(p.shape, generator=g) / max(p.shape[-1], 8) ** 0.5).bfloat16().float())
    f0 = torch.randn(B, Cf, 8 * h, 8 * w, generator=g).bfloat16()
    f3 = torch.randn(B, Cc, h, w, generator=g).bfloat16()
    go = torch.randn(B, 32, 8 * h, 8 * w, generator=g).bfloat16()
    a, b = f0.float().clone().requires_grad_(True), f3.float().clone().requires_grad_(True)
    yr = ad(torch.cat([a, F.interpolate(b, scale_factor=8, mode="nearest")], 1))
    (yr * go.float()).sum().backward()
    ref = [yr.detach(), a.grad, b.grad] + [p.grad.clone() for p in ad.parameters()]
    import copy
    adg = copy.deepcopy(ad).to(device).bfloat16()
    for p in adg.parameters():
        p.grad = None
    ad_, bd_ = f0.to(device).requires_grad_(True), f3.to(device).requires_grad_(True)
    y = adg.forward_split(ad_, bd_, 8)
    assert y is not None
    (y.float() * go.to(device).float()).sum().backward()
    got = [y.float().cpu(), ad_.grad.float().cpu(), bd_.grad.float().cpu()] + [p.grad.float().cpu() for p in adg.parameters()]
    for u, v in zip(got, ref):
        assert u.shape == v.shape and (u - v).abs().max() <= v.abs().max() * 2 ** -5


@pytest.mark.parametrize("N,C,H,W,K", [(12, 128, 48, 160, 31), (12, 256, 24, 80, 29), (12, 512, 12, 40, 27),
                                       (6, 1024, 6, 20, 13), (3, 64, 20, 36, 13), (2, 64, 50, 37, 31), (17, 64, 12, 32, 27)])
def test_dwconv_fused_input_batchnorm_relu_equals_the_separate_launches(device, N, C, H, W, K):
    """RepLKBlock forward (rka.py:305-308): pw1's BatchNorm + ReLU applied inside the depthwise kernel's staging pass
    (statistics finalised per wave from the 1x1 conv's epilogue sums) against the separate launches -- statistics from the
    same sums, flat apply, then the depthwise conv: forward outputs, saved statistics and running statistics BIT-IDENTICAL
    (same arithmetic, same rounding points; zero padding of the ACTIVATED tensor, incl. planes whose width is not a
    multiple of 8), gradients to rounding."""
    from ppeadepth import ops
    from ppeadepth.batchnorm import BatchNorm2d
    g = _g(N + C + K)
    Kin = 64
    x = torch.randn(N, Kin, H, W, generator=g).bfloat16().to(device)
    wpw = (torch.randn(C, Kin, 1, 1, generator=g) / Kin ** 0.5).to(device)
    wb = (torch.randn(C, 1, K, K, generator=g) / K).to(device)
    ws = (torch.randn(C, 1, 5, 5, generator=g) / 5).to(device)
    gb, gs = (torch.randn(N, C, H, W, generator=g).bfloat16().to(device) for _ in range(2))
    if (H * W) % 8:
        pytest.skip("the 1x1 conv's MFMA path (and its statistics epilogue) needs HW % 8 == 0")
    assert ops.dwconv_lk_bn_supported((N, C, H, W), K, 5)
    res = []
    for fused in (False, True):
        bn = BatchNorm2d(C).to(device)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(C, generator=_g(1)) + 0.5)
            bn.bias.copy_(torch.randn(C, generator=_g(2)) * 0.2)
        xl = x.clone().requires_grad_(True)
        z, sums = ops.pwconv_frozen(xl, wpw, want_sums=True)
        if fused:
            yb, ys, st = ops.dwconv_lk_bn(z, sums, bn, wb, ws)
            mean, invstd = st[0], st[1]
        else:
            mean, _var, invstd = ops.bn_batch_stats_from_sums(sums, N * H * W, bn.eps, bn.momentum, bn.running_mean,
                                                              bn.running_var)
            t = ops.bn_act_apply(z, bn.weight, bn.bias, mean, invstd, act=ops.ACT_RELU)
            yb, ys = ops.dwconv_lk(t, wb, ws)
        torch.autograd.backward([yb, ys], [gb, gs])
        res.append((yb, ys, mean.clone(), invstd.clone(), bn.running_mean.clone(), bn.running_var.clone(), xl.grad,
                    bn.weight.grad, bn.bias.grad))
    a, b = res
    for k in range(6):
        assert torch.equal(a[k], b[k]), k
    for k in (6, 7, 8):
        assert rel_err(b[k].float(), a[k].float()) < 2e-2, k


# ---- fp32 dense convolutions / linear layers on the fp32 matrix cores (csrc/conv_f32.hip) ----------------------------------
CONV_F32_CASES = [  # N, Cin, H, W, Cout, K, stride, pad, channels_last
    (2, 128, 16, 24, 128, 1, 1, 0, False),      # RepLKBlock pw1 / pw2 (rka.py:292-326)
    (2, 128, 16, 24, 32, 3, 1, 1, False),       # B_Adapter D_fc1 (rka.py:49-109)
    (3, 6, 33, 47, 64, 7, 2, 3, True),          # pose conv1 (resnet_encoder.py:376-388), ragged map, 6 input channels
    (2, 3, 32, 48, 128, 3, 2, 1, False),        # RepLKNet stem[0]
    (2, 64, 17, 23, 128, 3, 2, 1, True),        # ResNet layer2 conv1 (stride 2), channels_last, odd sizes
    (2, 64, 16, 24, 128, 1, 2, 0, True),        # ResNet downsample 1x1 stride 2
    (1, 70, 9, 13, 37, 3, 1, 0, False),         # decoder conv after the reflection pad (pad 0), ragged channels
    (2, 224, 12, 20, 128, 3, 1, 1, False),      # reduce_conv (rkm.py:127-131)
    (4, 256, 2, 3, 12, 1, 1, 0, True),          # PoseDecoder pose.2
]


@pytest.mark.parametrize("case", CONV_F32_CASES)
def test_conv2d_f32_mfma_vs_torch(device, case):
    """Forward, data gradient, weight gradient and bias gradient of csrc/conv_f32.hip against F.conv2d on the CPU in fp64
    (the oracle's arithmetic: plain PyTorch), NCHW and channels_last operands, 1e-5 relative."""
    from ppeadepth import ops
    N, Cin, H, W, Cout, K, stride, pad, cl = case
    g = _g(sum(case[:8]))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) / (Cin * K * K) ** 0.5
    b = torch.randn(Cout, generator=g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.conv2d(xr, wr, br, stride, pad)
    go = torch.randn(yr.shape, generator=g)
    yr.backward(go.double())
    xd = x.to(device)
    if cl:
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd.requires_grad_(True)
    wd, bd = w.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    assert ops.conv2d_f32_ok(xd, wd, (stride, stride), (pad, pad))
    y = ops.conv2d_f32(xd, wd, bd, stride, pad)
    assert y.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    y.backward(go.to(device))
    assert rel_err(y.detach().cpu(), yr.detach()) < 1e-5
    assert rel_err(xd.grad.cpu(), xr.grad) < 1e-5
    assert rel_err(wd.grad.cpu(), wr.grad) < 1e-5
    assert rel_err(bd.grad.cpu(), br.grad) < 1e-5


def test_conv2d_f32_module_linear_and_transposed_conv(device):
    """The module-level entry points of the fp32 family: `ops.Conv2d` (what nn.Conv2d.forward falls through to), nn.Linear
    over the channel axis, and ConvTranspose2d(32, 32, 3, 2, 1, 1) of the Stage-2 decoder adapter (dec.py:137-139) as the
    data gradient of a stride-2 conv -- outputs and every gradient against torch on the CPU in fp64."""
    from ppeadepth import ops
    from ppeadepth.networks.replknet_adapter import channel_linear
    g = _g(77)
    x = torch.randn(2, 32, 12, 16, generator=g)
    conv = ops.Conv2d(32, 48, 3, 1, 1)
    lin = torch.nn.Linear(48, 40)
    dec = torch.nn.ConvTranspose2d(40, 24, 3, 2, 1, output_padding=1)
    ref = [m.__class__(*a).double() for m, a in ((conv, (32, 48, 3, 1, 1)), (lin, (48, 40)))]
    ref.append(torch.nn.ConvTranspose2d(40, 24, 3, 2, 1, output_padding=1).double())
    for m, r in zip((conv, lin, dec), ref):
        r.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    xr = x.double().requires_grad_(True)
    h = ref[0](xr)
    h = F.linear(h.permute(0, 2, 3, 1), ref[1].weight, ref[1].bias).permute(0, 3, 1, 2)
    yr = ref[2](torch.nn.functional.gelu(h))
    go = torch.randn(yr.shape, generator=g)
    yr.backward(go.double())
    for m in (conv, lin, dec):
        m.to(device)
    xd = x.to(device).requires_grad_(True)
    h = channel_linear(conv(xd), lin)
    y = ops.conv_transpose_f32_module(dec, torch.nn.functional.gelu(h))
    assert y is not None and tuple(y.shape) == (2, 24, 24, 32)
    y.backward(go.to(device))
    assert rel_err(y.detach().cpu(), yr.detach()) < 1e-5
    assert rel_err(xd.grad.cpu(), xr.grad) < 1e-5
    for m, r in zip((conv, lin, dec), ref):
        for (k, p), (_, q) in zip(m.named_parameters(), r.named_parameters()):
            assert rel_err(p.grad.cpu(), q.grad) < 2e-5, (type(m).__name__, k)


def test_bn_statistics_from_epilogue_sums_with_a_large_mean(device):
    """the BatchNorm kernels that take their statistics from the producing GEMM's epilogue sums form
    var = E[x^2] - mean^2 (fp32 per-tile partials, fp64 combination).  Pinned against F.batch_norm in fp64 on channels with
    |mean| / std from 1 to 100: the relative variance error stays below 3e-7 * (1 + (mean / std)^2) (outputs: 1e-3 of the
    tensor's max at ratio 100, 2^-7 bf16 rounding below that), running statistics included."""
    from ppeadepth import batchnorm, ops
    from ppeadepth.networks import replknet_adapter as rka
    g = _g(41)
    B, K, M, H, W = 12, 64, 128, 12, 40
    conv = rka.PointwiseConv(K, M, 1, 1, 0, 1, 1, False)
    ratio = torch.tensor([1.0, 10.0, 30.0, 100.0]).repeat(M // 4)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(M, K, 1, 1, generator=g) / K ** 0.5)
    conv.weight.requires_grad_(False)
    conv = conv.to(device)
    conv.weight.data = conv.weight.data.bfloat16()
    bn = batchnorm.BatchNorm2d(M).to(device).train()
    x = torch.randn(B, K, H, W, generator=g)
    # a constant input channel with a large weight row sum shifts output channel m by ratio[m] standard deviations
    x[:, 0] = 1.0
    with torch.no_grad():
        conv.weight[:, 0, 0, 0] = ratio.to(device).bfloat16()
    xd = x.to(device).bfloat16()
    z, sums = conv.forward_sums(xd, always=True)
    assert sums is not None
    y = batchnorm.fused_bn_act(z, bn, sums=sums)
    zr = z.detach().double().cpu()
    mean, var = zr.mean((0, 2, 3)), zr.var((0, 2, 3), unbiased=False)
    assert float((mean.abs() / var.sqrt()).max()) > 60
    yr = F.batch_norm(zr, None, None, bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), True, 0.1, bn.eps)
    assert rel_err(y.detach().float().cpu(), yr) < 2 ** -7 + 1e-3
    n = B * H * W
    got_var = (bn.running_var.double().cpu() - 0.9) / 0.1 * (n - 1) / n
    rel = ((got_var - var).abs() / var)
    bound = 3e-7 * (1 + (mean / var.sqrt()) ** 2) + 1e-6
    assert bool((rel <= bound).all()), (rel / bound).max()
    assert rel_err(bn.running_mean.double().cpu() / 0.1, mean) < 1e-6


def test_cost_volume_bf16_packed_pairs_is_bit_identical_to_the_fp32_kernel(device):
    """The bf16 step's cost volume (channel pairs packed into dwords: half the bytes through the L1) against the fp32 kernel
    on the same features widened to fp32: same arithmetic in the same order -> identical bits, incl. a skipped item (zeroed
    pose), the 2-pixel border mask and footprints that leave the map; C = 30 (odd pair count), ragged map."""
    from oracle import synth
    from ppeadepth import ops
    g = _g(23)
    B, C, h, w, D = 3, 30, 21, 37, 13
    cur = torch.randn(B, C, h, w, generator=g).bfloat16().to(device)
    look = torch.randn(B, C, h, w, generator=g).bfloat16().to(device)
    K, inv_K = synth.kitti_K(4 * h, 4 * w, 2)
    K, inv_K = K[None].repeat(B, 1, 1).to(device), inv_K[None].repeat(B, 1, 1).to(device)
    T = torch.eye(4)[None].repeat(B, 1, 1)
    T[:, 2, 3], T[:, 0, 3] = 0.8, 0.3
    T[1] = 0.0                                                    # skipped item (repdepth.py:561-575)
    T = T.to(device)
    bins = torch.exp(torch.linspace(-2.3, 2.3, D)).to(device)
    a = ops.cost_volume(cur, look, T, K, inv_K, bins)
    saved, ops.CV_BF16 = ops.CV_BF16, False
    try:
        b = ops.cost_volume(cur, look, T, K, inv_K, bins)
    finally:
        ops.CV_BF16 = saved
    assert torch.equal(a, b)
    assert float((a[0] != 0).float().mean()) > 0.2 and float(a[1].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 64, 24, 40), (2, 16, 13, 19), (24, 64, 96, 320)])
def test_maxpool3x3s2_nhwc_equals_torch(device, dtype, shape):
    """MaxPool2d(3, 2, 1) of the pose trunk on channels_last tensors (csrc/nhwc_pool.hip) against F.max_pool2d: outputs and
    the input gradient EXACTLY (post-ReLU input: about half the entries are exact zeros, so the tie rule -- first maximum
    in scan order -- decides most windows), odd map sizes, the benchmarked [24,64,96,320]."""
    from ppeadepth import ops
    g = _g(sum(shape))
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    x = torch.relu(torch.randn(*shape, generator=g)).to(dt)
    xr = x.clone().to(device).requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    go = torch.randn(yr.shape, generator=g).to(dt).to(device)
    yr.backward(go)
    xd = x.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.maxpool3x3s2(xd)
    assert y is not None and y.is_contiguous(memory_format=torch.channels_last)
    y.backward(go)
    assert torch.equal(y.detach(), yr.detach())
    if dtype == "f32":
        assert torch.equal(xd.grad, xr.grad)
    else:       # torch accumulates the (up to four) bf16 contributions of a pixel in its own order; here: fp32 sum, one rounding
        assert rel_err(xd.grad.float().cpu(), xr.grad.float().cpu()) < 2 ** -7
        assert float((xd.grad != xr.grad).float().mean()) < 0.02


@pytest.mark.parametrize("is_multi", [False, True])
def test_loss_tail_equals_the_elementwise_composite(device, is_multi):
    """ops.loss_tail (mask, masked mean of the selected reprojection loss, consistency term and target: trainer.py:1092-1139
    in one pass per direction) against the reference's element-wise formulation in fp64 under autograd: both scalars, the
    mask, the target, d reproj (routed by the selection's source index incl. the forced-zero code 2) and d multi_depth."""
    from ppeadepth import ops
    g = _g(5 + int(is_multi))
    B, H, W = 3, 20, 36
    reproj = torch.rand(B, 2, H, W, generator=g)
    src = torch.randint(0, 3, (B, 1, H, W), generator=g).to(torch.uint8)
    sel = torch.where(src == 0, reproj[:, :1], torch.where(src == 1, reproj[:, 1:], torch.zeros(B, 1, H, W)))
    auto_idx = torch.randint(0, 2, (B, 1, H, W), generator=g)
    cons = (torch.rand(B, H, W, generator=g) > 0.4).float()
    aug = torch.tensor([0.0, 1.0, 0.0]).view(B, 1, 1, 1)
    multi = 1 + torch.rand(B, 1, H, W, generator=g)
    mono = 1 + torch.rand(B, 1, H, W, generator=g)
    multi[0, 0, 0, :5] = mono[0, 0, 0, :5]                      # |.| at 0: gradient 0
    # reference (fp64)
    r = reproj.double().requires_grad_(True)
    m64 = multi.double().requires_grad_(True)
    selr = torch.where(src == 0, r[:, :1], torch.where(src == 1, r[:, 1:], torch.zeros(B, 1, H, W, dtype=torch.float64)))
    if is_multi:
        mask = cons.double().unsqueeze(1) * (1 - aug.double())
    else:
        mask = (auto_idx == 0).double()
    rl_ref = (selr * mask).sum() / (mask.sum() + 1e-7)
    cm = 1 - mask
    cl_ref = (torch.abs(m64 - mono.double()) * cm).mean() if is_multi else None
    tgt_ref = 1 / (mono.double() * cm + m64.detach() * (1 - cm)) if is_multi else None
    (rl_ref * 0.7 + (cl_ref * 1.3 if is_multi else 0)).backward()
    # kernels
    rd = reproj.to(device).requires_grad_(True)
    md = multi.to(device).requires_grad_(True)
    res = ops.loss_tail(rd, sel.to(device), src.to(device), None if is_multi else auto_idx.to(device),
                        cons.to(device) if is_multi else None, aug.to(device) if is_multi else None,
                        md if is_multi else None, mono.to(device) if is_multi else None, is_multi)
    (res[0] * 0.7 + (res[1] * 1.3 if is_multi else 0)).backward()
    assert rel_err(res[0].detach().cpu().reshape(1), rl_ref.detach().reshape(1)) < 1e-6
    assert torch.equal(res[2].cpu().double(), mask)
    assert rel_err(rd.grad.cpu(), r.grad) < 1e-6
    if is_multi:
        assert rel_err(res[1].detach().cpu().reshape(1), cl_ref.detach().reshape(1)) < 1e-6
        assert rel_err(res[3].cpu(), tgt_ref) < 1e-6
        assert rel_err(md.grad.cpu(), m64.grad) < 1e-6
