"""Writes tests/golden/geometry_bits.npz: the raw bits of every output of the csrc/geometry.hip kernels, through their
`ops`-level functions, on seeded inputs.

    python tools/gen_geometry_bits_golden.py [--out tests/golden/geometry_bits.npz]          (needs the GPU)

The fixture pins the ARITHMETIC of the file -- association, order of the k sums, division against reciprocal-multiply, the
fixed order of the block reductions -- across changes that are meant to leave it alone: tests/test_geometry_bits_gpu.py
calls `compute()` again and asserts `torch.equal` against what was recorded.  Record it at the commit BEFORE such a change.
Inputs are not stored: `compute()` draws them from seeded host generators.

Contents (`compute()` is the list):
  backproject_project   grid, d_depth, K and T gradients (dP through the 4x4 product)
  backproject           points, d_depth, d_inv_K
  project3d             without / with the projected depth: grid, z, d_points, K and T gradients
  grid_sample           forward and grid gradient, zeros and border padding
  pose_matrix           forward and backward, invert False / True
  pose_chain            F = 1..4 on batch-strided views, one mid-chain frame of item 1 masked off; F = 3 on fp64 copies
  pose_chain_ring       F = 1..4 with a new pair, one item with seen < F; F = 3 from the ring alone
Shapes (B, H, W): (2, 5, 67) odd sizes and a ragged last block; (1, 2, 2) the minimum; (1, 72, 232) = 66 blocks of 256
pixels, so the 64-lane second reduction stage loops twice -- for that one only the reduced outputs are kept.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ppea-depth_amd")]

SHAPES = [(2, 5, 67), (1, 2, 2), (1, 72, 232)]
REDUCED_ONLY = {(1, 72, 232)}
POSE_B = 3


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _camera(B, H, W, seed, device):
    """Seeded per-item depth, K, inv_K (all nine entries of its 3x3 in play) and T (a perturbed identity)."""
    depth = 0.5 + 5 * torch.rand(B, 1, H, W, generator=_g(seed))
    K = torch.eye(4)[None].repeat(B, 1, 1)
    K[:, 0, 0], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2] = 0.58 * W, 0.5 * W, 1.92 * H, 0.5 * H
    K[:, 0, 0] *= 1 + 0.05 * torch.arange(B)
    K[:, 1, 2] *= 1 + 0.03 * torch.arange(B)
    inv_K = torch.linalg.inv(K)
    inv_K[:, :3, :3] += 0.02 * torch.randn(B, 3, 3, generator=_g(seed + 1)) * torch.tensor([1.0 / W, 1.0 / H, 1.0])
    T = torch.eye(4)[None].repeat(B, 1, 1)
    T[:, :3, :3] += 0.02 * torch.randn(B, 3, 3, generator=_g(seed + 2))
    T[:, :3, 3] = 0.1 * torch.randn(B, 3, generator=_g(seed + 3))
    return [t.to(device) for t in (depth, K, inv_K, T)]


def _leaf(t):
    return t.clone().requires_grad_(True)


def _geometry(ops, out, B, H, W, device):
    tag = f"{B}x{H}x{W}"
    full = (B, H, W) not in REDUCED_ONLY
    seed = 7000 + 100 * B + H
    depth, K, inv_K, T = _camera(B, H, W, seed, device)
    d_grid = torch.randn(B, H, W, 2, generator=_g(seed + 4)).to(device)
    d_z = torch.randn(B, 1, H, W, generator=_g(seed + 5)).to(device)
    d_points = torch.randn(B, 4, H * W, generator=_g(seed + 6)).to(device)
    points = torch.randn(B, 4, H * W, generator=_g(seed + 7)).to(device)
    points[:, 2] = points[:, 2].abs() + 1.0                    # in front of the camera
    points[:, 3] = 1.0 + 0.1 * points[:, 3]                    # row 3 is NOT all ones

    d, k, t = _leaf(depth), _leaf(K), _leaf(T)
    grid = ops.backproject_project(d, inv_K, k, t)
    grid.backward(d_grid)
    out[f"bpp/{tag}/K.grad"], out[f"bpp/{tag}/T.grad"] = k.grad, t.grad
    if full:
        out[f"bpp/{tag}/grid"], out[f"bpp/{tag}/d_depth"] = grid, d.grad

    d, ik = _leaf(depth), _leaf(inv_K)
    pts = ops.backproject(d, ik)
    pts.backward(d_points)
    out[f"bp/{tag}/d_inv_K"] = ik.grad
    if full:
        out[f"bp/{tag}/points"], out[f"bp/{tag}/d_depth"] = pts, d.grad

    for with_depth in (False, True):
        name = f"p3d{'z' if with_depth else ''}/{tag}"
        p, k, t = _leaf(points), _leaf(K), _leaf(T)
        res = ops.project3d(p, k, t, H, W, with_depth=with_depth)
        if with_depth:
            torch.autograd.backward(list(res), [d_grid, d_z])
            grid, z = res
        else:
            res.backward(d_grid)
            grid, z = res, None
        out[f"{name}/K.grad"], out[f"{name}/T.grad"] = k.grad, t.grad
        if full:
            out[f"{name}/grid"], out[f"{name}/d_points"] = grid, p.grad
            if z is not None:
                out[f"{name}/z"] = z

    if full:
        src = torch.rand(B, 3, H + 1, W + 2, generator=_g(seed + 8)).to(device)
        g = (2.6 * torch.rand(B, H, W, 2, generator=_g(seed + 9)) - 1.3)          # a tenth of the samples beyond each rim
        g[0, 0, 0, 0], g[0, 0, 1, 1], g[0, -1, -1, 0] = -1.0, 1.0, 50.0          # on the rims, and far outside
        d_out = torch.randn(B, 3, H, W, generator=_g(seed + 10)).to(device)
        for mode in ("zeros", "border"):
            gl = _leaf(g.to(device))
            o = ops.grid_sample(src, gl, mode)
            o.backward(d_out)
            out[f"gs/{tag}/{mode}/out"], out[f"gs/{tag}/{mode}/d_grid"] = o, gl.grad


def _pose(ops, out, device):
    B = POSE_B
    raw = torch.randn(4, B, 2, 1, 3, generator=_g(9001))          # four pose-network outputs; [:, :, 0] the axis-angle
    raw[:, :, 0] *= 0.05
    raw[:, :, 1] *= 0.3
    raw[0, 0, 0] = 0.0                                             # item 0 of pair 0: the zero rotation (angle = 0)
    dT = torch.randn(B, 4, 4, generator=_g(9002)).to(device)
    for invert in (False, True):
        aa, tr = _leaf(raw[1, :, 0].to(device)), _leaf(raw[1, :, 1].to(device))
        T = ops.pose_matrix(aa, tr, invert)
        T.backward(dT)
        out[f"pose/{int(invert)}/T"], out[f"pose/{int(invert)}/d_aa"], out[f"pose/{int(invert)}/d_tr"] = T, aa.grad, tr.grad

    dev = raw.to(device)
    for Fr in range(1, 5):
        pairs = [(dev[p, :, 0], dev[p, :, 1]) for p in range(Fr)]            # [B,1,3] views, batch stride 6
        chain = [(f, f % 2 == 0, f - 1) for f in range(Fr)]
        keep = torch.ones(B, Fr)
        keep[1, (Fr - 1) // 2] = 0.0
        out[f"chain/{Fr}/T"] = ops.pose_chain(pairs, chain, keep.to(device))
        out[f"chain/{Fr}/T_all"] = ops.pose_chain(pairs, chain)
    pairs = [(dev[p, :, 0].double(), dev[p, :, 1].double()) for p in range(3)]
    out["chain/3/T_copied"] = ops.pose_chain(pairs, [(2, True, -1), (0, False, 0), (1, True, 0)])

    for Fr in range(1, 5):
        ring = (0.2 * torch.randn(Fr, B, 2, 3, generator=_g(9100 + Fr))).to(device)
        state = torch.tensor([Fr + 1, Fr, Fr - 1, Fr + 2], dtype=torch.int32, device=device)    # head, seen[0..2]
        T, present = ops.pose_chain_ring(ring, state, (dev[3, :, 0], dev[3, :, 1]))
        out[f"ring/{Fr}/T"], out[f"ring/{Fr}/present"], out[f"ring/{Fr}/ring"] = T, present, ring
    ring = (0.2 * torch.randn(3, B, 2, 3, generator=_g(9200))).to(device)
    state = torch.tensor([-2, 3, 1, 2], dtype=torch.int32, device=device)
    T, present = ops.pose_chain_ring(ring, state)
    out["ring/3/T_stored"], out["ring/3/present_stored"] = T, present


def compute(device):
    """-> {name: host tensor}, every output listed in the module docstring."""
    from ppeadepth import ops
    out = {}
    for B, H, W in SHAPES:
        _geometry(ops, out, B, H, W, device)
    _pose(ops, out, device)
    return {k: v.detach().cpu() for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "geometry_bits.npz"))
    args = ap.parse_args()
    out = {k: v.numpy() for k, v in compute(torch.device("cuda:0")).items()}
    for k, v in out.items():
        assert np.isfinite(v.astype(np.float64)).all(), k
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    assert size < 512 * 1024, size
    print(f"wrote {args.out}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
