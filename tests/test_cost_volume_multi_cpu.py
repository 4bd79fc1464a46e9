"""Several lookup frames without a GPU: the CPU composite of the fused cost volume against the reference's own loop over the
lookups (tests/golden/cost_volume_multi.npz, written by tools/gen_golden_multi.py), its single-frame form against the
function it replaced, the declarations of the two new entry points, and a CPU predictor with two matching frames."""
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_err

from oracle import synth

FWD_TOL = 2e-5      # the project's fp32 forward bound against the reference (tests/test_kernels_gpu.py)
FOLD_TOL = 1e-4     # fp32 torch on the same machine (tests/test_inference_cpu.py)
B, H, W = 2, 64, 96


def test_cpu_composite_reproduces_the_reference_on_three_lookup_frames(golden):
    """Measured: masked cost 1.4e-06, lowest_cost 0; confidence, missing mask and argmin (outside the 1 near-tie pixel) equal."""
    from ppeadepth.inference import cost_volume_cpu, cost_volume_reduce_cpu
    g = golden("cost_volume_multi")
    raw = cost_volume_cpu(g["cur"], g["lookup"], g["poses"], g["K"], g["inv_K"], g["bins"])
    masked, conf, idx, low = cost_volume_reduce_cpu(raw, g["bins"])
    keep = ~g["near_tie"]
    assert float(g["near_tie"].float().mean()) <= 5e-3
    assert torch.equal(conf, g["confidence"])
    assert torch.equal((raw == 0), g["missing"].bool())
    e_cost = rel_err(masked, g["cost"] * g["confidence"].unsqueeze(1))
    e_low = rel_err(low[keep], g["lowest_cost"][keep])
    print(f"cpu composite vs reference, F = 3: masked cost {e_cost:.3e} lowest_cost {e_low:.3e}")
    assert e_cost < FWD_TOL and e_low < FWD_TOL
    assert idx.dtype == torch.int64 and torch.equal(idx[keep], g["argmin"][keep])
    assert float(raw[2].abs().max()) == 0.0                          # every frame skipped
    # item 1 (frame 1 zeroed) is the two remaining frames
    two = cost_volume_cpu(g["cur"][1:2], g["lookup"][1:2, [0, 2]], g["poses"][1:2, [0, 2]], g["K"][1:2], g["inv_K"][1:2],
                          g["bins"])
    assert torch.equal(raw[1:2], two)


def _single_frame_before(cur, look, poses, K, inv_K, bins, eps=1e-7):
    """`inference.cost_volume_cpu` as it was when it served one lookup frame."""
    Bn, C, h, w = cur.shape
    D = bins.shape[0]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w)], 0)
    inner = torch.zeros(h, w)
    inner[2:-2, 2:-2] = 1.0
    out = []
    for b in range(Bn):
        if float(poses[b].sum()) == 0.0:
            out.append(torch.zeros(D, h, w))
            continue
        rays = inv_K[b, :3, :3] @ pix
        pts = torch.cat([bins.view(D, 1, 1) * rays[None], torch.ones(D, 1, h * w)], 1)
        cam = (K[b] @ poses[b])[:3][None] @ pts
        xy = cam[:, :2] / (cam[:, 2:3] + eps)
        gx = ((xy[:, 0] / (w - 1)) - 0.5) * 2
        gy = ((xy[:, 1] / (h - 1)) - 0.5) * 2
        grid = torch.stack([gx, gy], -1).reshape(D, h, w, 2)
        warped = F.grid_sample(look[b][None].expand(D, C, h, w), grid, mode="bilinear", padding_mode="zeros",
                               align_corners=True)
        xv, yv = (grid[..., 0] / 2 + 0.5) * (w - 1), (grid[..., 1] / 2 + 0.5) * (h - 1)
        edge = ((xv >= 2.0) & (xv <= w - 2) & (yv >= 2.0) & (yv <= h - 2)).float()
        diff = (warped - cur[b:b + 1]).abs().mean(1) * (edge * inner)
        out.append(diff / ((diff > 0).float() + 1e-7))
    return torch.stack(out)


def test_cpu_composite_with_one_frame_is_bitwise_the_single_frame_function(golden):
    from ppeadepth.inference import cost_volume_cpu
    g = golden("cost_volume")
    args = (g["K"], g["inv_K"], g["bins"])
    before = _single_frame_before(g["cur"], g["lookup"][:, 0], g["poses"][:, 0], *args)
    assert float((before[0] != 0).float().mean()) > 0.2
    assert torch.equal(cost_volume_cpu(g["cur"], g["lookup"][:, 0], g["poses"][:, 0], *args), before)
    assert torch.equal(cost_volume_cpu(g["cur"], g["lookup"], g["poses"], *args), before)          # [B,1,...] form


def test_multi_frame_entry_points_are_declared_and_bound():
    from ppeadepth import _abi
    header = open(os.path.join(ROOT, "include", "ppea_depth.h")).read()
    for name, nargs in (("ppea_cost_volume_multi_fwd_f32", 15), ("ppea_cost_volume_multi_fwd_bf16", 16)):
        assert re.search(r"\bint %s\(" % name, header)
        assert len(_abi.SIGNATURES[name]) == nargs and hasattr(_abi.lib, name)


def _build(**extra):
    from ppeadepth import networks, options
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, **extra)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model, conditioned=True)
    return model.train(), opt


@pytest.fixture(scope="module")
def two_frames():
    return _build(num_matching_frames=2)


def test_cpu_predictor_with_two_matching_frames_chains_the_poses(two_frames):
    """Measured: pose[:, 1] against pose_pair(-2, -1) @ pose[:, 0] computed pair by pair: 0 (equal)."""
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.layers import transformation_from_parameters
    model, opt = two_frames
    assert model.matching_ids == [0, -1, -2]
    data = synth.make_rendered_inputs(B, H, W, frame_ids=(0, -1, 1, -2))
    p = DepthPredictor(model, opt, device="cpu")
    looks = torch.stack([data[("color", -1, 0)], data[("color", -2, 0)]], 1)
    r = p.predict(data[("color", 0, 0)], looks, data[("K", 2)], data[("inv_K", 2)], 0.1, 10.0)
    assert r["disp"].shape == (B, 1, H, W) and r["lowest_cost"].shape == (B, H // 4, W // 4) and r["pose"].shape == (B, 2, 4, 4)
    assert bool(torch.isfinite(r["disp"]).all()) and model.training
    with torch.no_grad():
        aa, tt = model.pose([[p._pose_features(torch.cat([data[("color", -2, 0)], data[("color", -1, 0)]], 1))]])
        pair = transformation_from_parameters(aa[:, 0], tt[:, 0], invert=True)
    e = rel_err(r["pose"][:, 1], torch.matmul(pair, r["pose"][:, 0]))
    print(f"chained pose 0 -> -2: {e:.3e}")
    assert e <= FOLD_TOL
    # the second frame is used: another frame -2 moves the prediction, and a [B,3,H,W] call is refused
    other = looks.clone()
    other[:, 1] = data[("color", 1, 0)]
    r2 = p.predict(data[("color", 0, 0)], other, data[("K", 2)], data[("inv_K", 2)], 0.1, 10.0)
    assert not torch.equal(r2["disp"], r["disp"])
    from ppeadepth import _abi
    with pytest.raises(_abi.PpeaKernelError):
        p.predict(data[("color", 0, 0)], data[("color", -1, 0)], data[("K", 2)], data[("inv_K", 2)], 0.1, 10.0)


def test_predictor_refuses_an_opt_that_disagrees_with_the_model(two_frames):
    from ppeadepth import _abi
    from ppeadepth.inference import DepthPredictor
    model, opt = two_frames
    for bad in (types.SimpleNamespace(num_matching_frames=1), types.SimpleNamespace(num_matching_frames=3),
                types.SimpleNamespace(num_matching_frames=2, use_future_frame=True)):
        with pytest.raises(_abi.PpeaKernelError):
            DepthPredictor(model, bad, device="cpu")
    assert DepthPredictor(model, opt, device="cpu").lookup_ids == [-1, -2]
