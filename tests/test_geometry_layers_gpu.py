"""`layers.BackprojectDepth` / `layers.Project3D` on the HIP kernels of csrc/geometry.hip (backproject_*, project3d_*):
the reference's goldens through the class API, bit identity with the fused `ops.backproject_project`, gradients against
the reference's class bodies evaluated in fp64 on the host, determinism, fp32 arithmetic under autocast, the launch
census of the class chain, and the boundaries (ops refuse host tensors, Trainer attributes, plug-in package name).

Shapes: 5x67 = 335 pixels (two blocks, ragged tail, odd width); 96x192 = 72 blocks per image (the 64-lane second-stage
reduction loops twice); 2x2 (W - 1 = H - 1 = 1).  Every batch item has its own depth, K, inv_K and T.
"""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 67), (3, 96, 192), (1, 2, 2)]
BWD_TOL = 2e-4              # tests/test_kernels_gpu.py:18, applied as rel_err(...) < BWD_TOL at :215-216


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _mods():
    from ppeadepth import layers, ops
    return layers, ops


# ---- the parent commit's class bodies (reference layers.py:163-168, 184-199), dtype-agnostic: the fp64 host reference ----
def _backproject_ref(depth, inv_K, H, W):
    B = depth.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=depth.dtype), torch.arange(W, dtype=depth.dtype), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=depth.dtype)], 0)[None].repeat(B, 1, 1)
    cam_points = torch.matmul(inv_K[:, :3, :3], pix)
    cam_points = depth.view(B, 1, -1) * cam_points
    return torch.cat([cam_points, torch.ones(B, 1, H * W, dtype=depth.dtype)], 1)


def _project3d_ref(points, K, T, H, W, eps=1e-7):
    B = points.shape[0]
    P = torch.matmul(K, T)[:, :3, :]
    cam_points = torch.matmul(P, points)
    pix = cam_points[:, :2, :] / (cam_points[:, 2, :].unsqueeze(1) + eps)
    pix = pix.view(B, 2, H, W).permute(0, 2, 3, 1)
    pix = (pix / pix.new_tensor([W - 1, H - 1]) - 0.5) * 2
    return pix, cam_points[:, 2, :].unsqueeze(1).view(B, 1, H, W)


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """Seeded fp32 host inputs of one shape (never modified) and the fp64 reference gradients, computed once per shape."""
    from oracle import synth
    seed = 1000 * B + H
    depth = 0.5 + 5 * torch.rand(B, 1, H, W, generator=_g(seed))
    K0, _ = synth.kitti_K(H, W, 0)
    K = K0[None].repeat(B, 1, 1)
    K[:, 0, 0] *= 1 + 0.05 * torch.arange(B)                    # a focal length per item
    K[:, 1, 2] *= 1 + 0.03 * torch.arange(B)
    inv_K = torch.linalg.pinv(K)
    # all nine entries of inv_K[:3,:3] in play (an exact inverse has four zeros); the x / y columns scaled so that the
    # ray's z stays near 1 across the image
    inv_K[:, :3, :3] += 0.02 * torch.randn(B, 3, 3, generator=_g(seed + 1)) * torch.tensor([1.0 / W, 1.0 / H, 1.0])
    T = R.transformation_from_parameters(0.02 * torch.randn(B, 1, 3, generator=_g(seed + 2)),
                                         0.1 * torch.randn(B, 1, 3, generator=_g(seed + 3)), True)
    # Project3D on its own: a point cloud whose row 3 is NOT all ones
    points = torch.cat([2 * torch.randn(B, 1, H * W, generator=_g(seed + 4)), torch.randn(B, 1, H * W, generator=_g(seed + 5)),
                        0.5 + 5 * torch.rand(B, 1, H * W, generator=_g(seed + 6)),
                        1 + 0.2 * torch.rand(B, 1, H * W, generator=_g(seed + 7))], 1)
    g_points = torch.randn(B, 4, H * W, generator=_g(seed + 8))
    g_grid = torch.randn(B, H, W, 2, generator=_g(seed + 9))
    g_z = torch.randn(B, 1, H, W, generator=_g(seed + 10))
    c = dict(depth=depth, K=K, inv_K=inv_K, T=T, points=points, g_points=g_points, g_grid=g_grid, g_z=g_z)
    d = {k: v.double() for k, v in c.items()}
    dd, di = d["depth"].requires_grad_(True), d["inv_K"].requires_grad_(True)
    (_backproject_ref(dd, di, H, W) * d["g_points"]).sum().backward()
    c["ref_bp"] = (dd.grad, di.grad)
    for dc in (False, True):
        pp, kk, tt = (d[k].detach().clone().requires_grad_(True) for k in ("points", "K", "T"))
        pix, z = _project3d_ref(pp, kk, tt, H, W)
        ((pix * d["g_grid"]).sum() + ((z * d["g_z"]).sum() if dc else 0.0)).backward()
        c["ref_p3", dc] = (pp.grad, kk.grad, tt.grad)
    return c


def _dev(c, device, *names, grad=()):
    return [c[n].to(device).requires_grad_(n in grad) for n in names]


# ---- 1. the reference's own outputs through the class API ---------------------------------------------------------------
def test_classes_match_reference_golden(device, golden):
    """Bounds of tests/test_oracle_golden.py::test_backproject_project_warp for the same arrays: rel 1e-5 (points),
    abs 1e-5 (grid)."""
    layers, _ = _mods()
    g = golden("layers_geometry")
    B, _, H, W = g["depth"].shape
    pts = layers.BackprojectDepth(B, H, W).to(device)(g["depth"].to(device), g["inv_K"].to(device))
    assert pts.shape == g["points"].shape and pts.dtype == torch.float32
    assert rel_err(pts.cpu(), g["points"]) < 1e-5
    grid = layers.Project3D(B, H, W).to(device)(g["points"].to(device), g["K"].to(device), g["T_inv"].to(device))
    assert grid.shape == g["grid"].shape
    assert (grid.cpu() - g["grid"]).abs().max() < 1e-5


# ---- 2. the same arithmetic, split at the point cloud ---------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_chain_is_bit_identical_to_fused_kernel(device, B, H, W):
    layers, ops = _mods()
    c = _case(B, H, W)
    bp, pr = layers.BackprojectDepth(B, H, W).to(device), layers.Project3D(B, H, W).to(device)
    d1, inv_K, K, T1 = _dev(c, device, "depth", "inv_K", "K", "T", grad=("depth", "T"))
    d2, T2 = _dev(c, device, "depth", "T", grad=("depth", "T"))
    gg = c["g_grid"].to(device)
    pts = bp(d1, inv_K)
    assert pts.shape == (B, 4, H * W) and bool((pts[:, 3] == 1).all())
    grid = pr(pts, K, T1)
    fused = ops.backproject_project(d2, inv_K, K, T2)
    assert torch.equal(grid, fused)
    grid.backward(gg)
    fused.backward(gg)
    assert torch.equal(d1.grad, d2.grad)                       # the chained d_depth carries the fused kernel's bits
    assert torch.equal(T1.grad, T2.grad)                       # ... and so does the pose gradient (same fixed-order dP)


# ---- 3. gradients against the fp64 host composite -------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_backproject_gradients(device, B, H, W):
    layers, _ = _mods()
    c = _case(B, H, W)
    depth, inv_K = _dev(c, device, "depth", "inv_K", grad=("depth", "inv_K"))
    pts = layers.BackprojectDepth(B, H, W).to(device)(depth, inv_K)
    assert rel_err(pts.cpu(), _backproject_ref(c["depth"].double(), c["inv_K"].double(), H, W)) < 1e-5
    pts.backward(c["g_points"].to(device))
    ref_depth, ref_inv_K = c["ref_bp"]
    print("d_depth", rel_err(depth.grad.cpu(), ref_depth), "d_inv_K", rel_err(inv_K.grad.cpu(), ref_inv_K))
    assert rel_err(depth.grad.cpu(), ref_depth) < BWD_TOL
    assert rel_err(inv_K.grad.cpu(), ref_inv_K) < BWD_TOL
    assert bool((inv_K.grad[:, 3, :] == 0).all()) and bool((inv_K.grad[:, :, 3] == 0).all())
    # inv_K without a gradient: the sums are skipped, d_depth is the same
    d2, k2 = _dev(c, device, "depth", "inv_K", grad=("depth",))
    layers.BackprojectDepth(B, H, W).to(device)(d2, k2).backward(c["g_points"].to(device))
    assert torch.equal(d2.grad, depth.grad) and k2.grad is None


@pytest.mark.parametrize("dc", [False, True])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_project3d_gradients(device, B, H, W, dc):
    layers, _ = _mods()
    c = _case(B, H, W)
    points, K, T = _dev(c, device, "points", "K", "T", grad=("points", "K", "T"))
    out = layers.Project3D(B, H, W, dc=dc).to(device)(points, K, T)
    ref_pix, ref_z = _project3d_ref(c["points"].double(), c["K"].double(), c["T"].double(), H, W)
    if dc:
        pix, z = out
        assert z.shape == (B, 1, H, W) and rel_err(z.cpu(), ref_z) < 1e-5
        torch.autograd.backward([pix, z], [c["g_grid"].to(device), c["g_z"].to(device)])
    else:
        pix = out
        pix.backward(c["g_grid"].to(device))
    assert pix.shape == (B, H, W, 2) and rel_err(pix.cpu(), ref_pix) < 1e-5
    for name, got, ref in zip(("d_points", "dK", "dT"), (points.grad, K.grad, T.grad), c["ref_p3", dc]):
        print(name, rel_err(got.cpu(), ref))
        assert rel_err(got.cpu(), ref) < BWD_TOL, name


def test_project3d_depth_output_alone_carries_a_gradient(device):
    """`dc=True` with only the projected depth used downstream: d cam[2] / d points = P[2]."""
    layers, _ = _mods()
    B, H, W = SHAPES[0]
    c = _case(B, H, W)
    points, K, T = _dev(c, device, "points", "K", "T", grad=("points",))
    _, z = layers.Project3D(B, H, W, dc=True).to(device)(points, K, T)
    z.backward(c["g_z"].to(device))
    P2 = torch.matmul(c["K"].double(), c["T"].double())[:, 2, :]
    ref = P2[:, :, None] * c["g_z"].double().view(B, 1, -1)
    assert rel_err(points.grad.cpu(), ref) < BWD_TOL


def test_one_camera_for_all_items(device):
    """The matching encoders' use (reference networks/resnet_encoder.py:187-201): `batch_size` = number of depth planes D,
    depth [D,h,w] without a channel axis, and ONE camera and pose, inv_K / K / T of shape [1,4,4], for all D items.  The
    composite broadcasts them in its matmuls; the device path has to give the same points, grid, projected depth and
    gradients (d inv_K, dK, dT are sums over the D items).  Reference: the class bodies in fp64 on the host, bounds as in
    the per-item tests above."""
    layers, _ = _mods()
    D, H, W = 5, 5, 67
    c = _case(2, H, W)
    host = dict(depth=0.5 + 5 * torch.rand(D, H, W, generator=_g(77)), inv_K=c["inv_K"][1:2], K=c["K"][1:2], T=c["T"][1:2],
                points=torch.cat([c["points"], c["points"].flip(2), c["points"][:1] * 1.1], 0),
                g_points=torch.randn(D, 4, H * W, generator=_g(78)), g_grid=torch.randn(D, H, W, 2, generator=_g(79)),
                g_z=torch.randn(D, 1, H, W, generator=_g(80)))
    d = {k: v.double() for k, v in host.items()}
    bp, pr = layers.BackprojectDepth(D, H, W).to(device), layers.Project3D(D, H, W, dc=True).to(device)

    depth, inv_K = _dev(host, device, "depth", "inv_K", grad=("depth", "inv_K"))
    pts = bp(depth, inv_K)
    dd, di = d["depth"].clone().requires_grad_(True), d["inv_K"].clone().requires_grad_(True)
    ref_pts = _backproject_ref(dd, di, H, W)
    assert pts.shape == (D, 4, H * W) and rel_err(pts.detach().cpu(), ref_pts.detach()) < 1e-5
    pts.backward(host["g_points"].to(device))
    (ref_pts * d["g_points"]).sum().backward()
    assert depth.grad.shape == (D, H, W) and inv_K.grad.shape == (1, 4, 4)
    for name, got, ref in (("d_depth", depth.grad, dd.grad), ("d_inv_K", inv_K.grad, di.grad)):
        print(name, rel_err(got.cpu(), ref))
        assert rel_err(got.cpu(), ref) < BWD_TOL, name
    # depth without a gradient: d_depth is neither allocated nor written, d_inv_K is the same
    d2, k2 = _dev(host, device, "depth", "inv_K", grad=("inv_K",))
    bp(d2, k2).backward(host["g_points"].to(device))
    assert d2.grad is None and torch.equal(k2.grad, inv_K.grad)

    points, K, T = _dev(host, device, "points", "K", "T", grad=("points", "K", "T"))
    pix, z = pr(points, K, T)
    pp, kk, tt = (d[k].clone().requires_grad_(True) for k in ("points", "K", "T"))
    ref_pix, ref_z = _project3d_ref(pp, kk, tt, H, W)
    assert pix.shape == (D, H, W, 2) and rel_err(pix.detach().cpu(), ref_pix.detach()) < 1e-5
    assert z.shape == (D, 1, H, W) and rel_err(z.detach().cpu(), ref_z.detach()) < 1e-5
    torch.autograd.backward([pix, z], [host["g_grid"].to(device), host["g_z"].to(device)])
    ((ref_pix * d["g_grid"]).sum() + (ref_z * d["g_z"]).sum()).backward()
    assert K.grad.shape == T.grad.shape == (1, 4, 4)
    for name, got, ref in (("d_points", points.grad, pp.grad), ("dK", K.grad, kk.grad), ("dT", T.grad, tt.grad)):
        print(name, rel_err(got.cpu(), ref))
        assert rel_err(got.cpu(), ref) < BWD_TOL, name
    # a camera per item with one pose for all: the remaining broadcast the composite's K @ T accepts
    K5, T1 = host["K"].repeat(D, 1, 1).to(device), host["T"].to(device)
    assert torch.equal(pr(points.detach(), K5, T1)[0], pix)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------
def test_backward_is_bitwise_reproducible(device):
    layers, _ = _mods()
    B, H, W = 3, 96, 192
    c = _case(B, H, W)
    bp, pr = layers.BackprojectDepth(B, H, W).to(device), layers.Project3D(B, H, W, dc=True).to(device)
    runs = []
    for rep in range(2):
        depth, inv_K, K, T = _dev(c, device, "depth", "inv_K", "K", "T", grad=("depth", "inv_K", "K", "T"))
        junk = torch.full((1 << 18,), float("nan"), device=device)      # whatever the allocator hands out next
        del junk
        pix, z = pr(bp(depth, inv_K), K, T)
        torch.autograd.backward([pix, z], [c["g_grid"].to(device), c["g_z"].to(device)])
        runs.append([t.grad.clone() for t in (depth, inv_K, K, T)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 5. fp32 under autocast ----------------------------------------------------------------------------------------------
def test_autocast_keeps_fp32_bits(device):
    layers, _ = _mods()
    B, H, W = SHAPES[0]
    c = _case(B, H, W)
    bp, pr = layers.BackprojectDepth(B, H, W).to(device), layers.Project3D(B, H, W, dc=True).to(device)
    depth, inv_K, K, T = _dev(c, device, "depth", "inv_K", "K", "T")
    pts = bp(depth, inv_K)
    pix, z = pr(pts, K, T)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pts_a = bp(depth, inv_K)
        pix_a, z_a = pr(pts_a, K, T)
    for a, b in ((pts_a, pts), (pix_a, pix), (z_a, z)):
        assert a.dtype == torch.float32 and torch.equal(a, b)


# ---- 6. launch census ----------------------------------------------------------------------------------------------------
def test_class_chain_launch_census(device):
    """One forward + backward of BackprojectDepth -> Project3D at B=3, 96x192 with every input asking for its gradient
    (profiler pattern of tests/test_e2e_gpu.py::test_fp32_step_launches_no_library_convolution_or_gemm).  Library kernels:
    the 4x4 product K @ T and its two gradient products, nothing else.  Device launches: forward backproject_fwd, K @ T,
    project3d_fwd = 3; backward project3d_bwd + its reduction, the product's two gradients, backproject_bwd + its
    reduction = 6."""
    from torch.profiler import ProfilerActivity, profile
    layers, _ = _mods()
    B, H, W = 3, 96, 192
    c = _case(B, H, W)
    bp, pr = layers.BackprojectDepth(B, H, W).to(device), layers.Project3D(B, H, W).to(device)
    gg = c["g_grid"].to(device)

    def run():
        depth, inv_K, K, T = _dev(c, device, "depth", "inv_K", "K", "T", grad=("depth", "inv_K", "K", "T"))
        torch.cuda.synchronize()
        return (depth, inv_K, K, T), (lambda: pr(bp(depth, inv_K), K, T).backward(gg))

    run()[1]()                                               # warm-up (code objects, rocBLAS solution lookup)
    torch.cuda.synchronize()
    leaves, step = run()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        step()
        torch.cuda.synchronize()
    assert all(t.grad is not None for t in leaves)
    names = {}
    for ev in prof.events():
        if str(ev.device_type).endswith("CUDA") and ev.name:
            names[ev.name] = names.get(ev.name, 0) + 1
    print(names)
    ours = sum(n for k, n in names.items() if re.search(r"backproject_(fwd|bwd)|project3d_(fwd|bwd)|bp_reduce_4x4", k))
    assert ours == 6, names
    lib = re.compile(r"Cijk_|igemm|ck::|ck_tile|miopen|MIOpen|naive_conv|SubTensorOp|gemm_|Gemm|wmma|batched_transpose")
    hits = {n: k for n, k in names.items() if lib.search(n)}
    assert not {n: k for n, k in hits.items() if "Cijk_" not in n}, hits
    assert sum(hits.values()) <= 3, hits                      # K @ T and its two gradient products
    assert sum(names.values()) <= 9, names


# ---- 7. boundary ---------------------------------------------------------------------------------------------------------
def test_device_instances_hold_no_pixel_buffers(device):
    layers, _ = _mods()
    B, H, W = SHAPES[0]
    c = _case(B, H, W)
    bp = layers.BackprojectDepth(B, H, W).to(device)
    bp(*_dev(c, device, "depth", "inv_K"))
    held = [v for v in list(bp.buffers()) + list(bp.parameters()) + list(vars(bp).values()) if torch.is_tensor(v)]
    assert not held and bp._host is None


def test_reference_style_generate_images_pred(device):
    """A `generate_images_pred` written against the reference's Trainer attributes (reference trainer.py:898-914) gives
    the sampling grids of this build's fused `Trainer.generate_images_pred`, bit for bit, and the same warped frames."""
    from oracle import synth
    from ppeadepth import options
    from ppeadepth.layers import disp_to_depth, transformation_from_parameters
    from ppeadepth.trainer import Trainer
    B, H, W = 2, 64, 96
    opt = options.default_options(height=H, width=W, batch_size=B)
    tr = Trainer(opt, None, device)
    assert sorted(tr.backproject_depth) == sorted(tr.project_3d) == list(range(opt.sclm + 1))
    assert type(tr.backproject_depth[0]).__name__ == "BackprojectDepth" and type(tr.project_3d[0]).__name__ == "Project3D"
    assert (tr.backproject_depth[0].batch_size, tr.backproject_depth[0].height, tr.backproject_depth[0].width) == (B, H, W)
    assert (tr.project_3d[0].batch_size, tr.project_3d[0].height, tr.project_3d[0].width) == (B, H, W)
    inputs = {k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W).items()}

    def outputs():
        o = {("disp", 0): (0.02 + 0.9 * torch.rand(B, 1, H, W, generator=_g(5))).to(device)}
        for i, f in enumerate(opt.frame_ids[1:]):
            o[("cam_T_cam", 0, f)] = transformation_from_parameters(
                (0.02 * torch.randn(B, 1, 3, generator=_g(6 + i))).to(device),
                (0.1 * torch.randn(B, 1, 3, generator=_g(8 + i))).to(device), invert=(f < 0))
        return o

    ours = outputs()
    tr.generate_images_pred(inputs, ours)
    ref = outputs()
    for scale in range(opt.sclm + 1):
        _, depth = disp_to_depth(ref[("disp", scale)], opt.min_depth, opt.max_depth)
        ref[("depth", 0, scale)] = depth
        for frame_id in opt.frame_ids[1:]:
            T = ref[("cam_T_cam", 0, frame_id)]
            cam_points = tr.backproject_depth[0](ref[("depth", 0, scale)], inputs[("inv_K", 0)])
            pix_coords = tr.project_3d[0](cam_points, inputs[("K", 0)], T)
            ref[("sample", frame_id, scale)] = pix_coords
            ref[("color", frame_id, scale)] = F.grid_sample(inputs[("color", frame_id, 0)], pix_coords,
                                                            padding_mode="border", align_corners=True)
    for f in opt.frame_ids[1:]:
        assert torch.equal(ref[("sample", f, 0)], ours[("sample", f, 0)])
        assert rel_err(ref[("color", f, 0)], ours[("color", f, 0)]) < 2e-5


def test_classes_under_the_plugin_package_name():
    """`ppea_kernels.layers` in a process whose `ppeadepth` is foreign (tests/test_plugin.py): both classes run on the
    kernels there and agree with their own host composite."""
    from test_plugin import _child
    out = _child("""
        sys.path.append(os.environ['LARGE_KERNEL_CONV_IMPL'])         # INTEGRATION.md section 2
        import ppea_kernels
        L = ppea_kernels.layers
        assert L.__name__ == "_ppea_depth_amd_kernels.layers" and sys.modules["ppeadepth"] is foreign
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(3)
        B, H, W = 2, 5, 67
        depth = 0.5 + 5 * torch.rand(B, 1, H, W, generator=g)
        K = torch.tensor([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]])[None].repeat(B, 1, 1)
        T = torch.eye(4)[None].repeat(B, 1, 1)
        T[:, :3, 3] = 0.1 * torch.randn(B, 3, generator=g)
        bp, pr = L.BackprojectDepth(B, H, W), L.Project3D(B, H, W, dc=True)
        pts = bp(depth, torch.linalg.inv(K))
        pix, z = pr(pts, K, T)
        bp, pr = bp.to(dev), pr.to(dev)
        pts_d = bp(depth.to(dev), torch.linalg.inv(K).to(dev))
        pix_d, z_d = pr(pts_d, K.to(dev), T.to(dev))
        def rel(a, b):
            return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))
        assert rel(pts_d.cpu(), pts) < 1e-5 and rel(z_d.cpu(), z) < 1e-5 and (pix_d.cpu() - pix).abs().max() < 1e-5
        try:
            ppea_kernels.ops.backproject(depth, torch.linalg.inv(K))
        except Exception as e:
            assert type(e).__name__ == "PpeaKernelError", repr(e)
        else:
            raise AssertionError("CPU tensor was accepted")
        print("ok")
    """)
    assert out.strip().endswith("ok")
