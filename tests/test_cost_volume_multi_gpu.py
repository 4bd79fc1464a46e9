"""`ops.cost_volume_multi`: F lookup frames in one fused launch, against the reference's own loop over the lookups
(tests/golden/cost_volume_multi.npz), the recorded bits of the former single-frame kernels for F = 1, the bf16 packed
form and the CPU composite."""
import pytest
import torch

from conftest import rel_err

from oracle import synth

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5      # tests/test_kernels_gpu.py: the bound of test_cost_volume_golden


def test_cost_volume_multi_golden(device, golden):
    """Measured: masked cost 2.8e-06, lowest_cost 0, argmin equal at every pixel (the near-tie pixel included)."""
    from ppeadepth import ops
    g = {k: v.to(device) for k, v in golden("cost_volume_multi").items()}
    args = (g["K"], g["inv_K"], g["bins"])
    cost = ops.cost_volume_multi(g["cur"], g["lookup"], g["poses"], *args)
    masked, conf, idx, low = ops.cost_volume_reduce(cost, g["bins"])
    keep = ~g["near_tie"]
    assert float(g["near_tie"].float().mean()) <= 5e-3
    assert torch.equal(conf, g["confidence"])
    e_cost = rel_err(masked, g["cost"] * g["confidence"].unsqueeze(1))
    e_low = rel_err(low[keep], g["lowest_cost"][keep])
    print(f"fused F = 3 vs reference: masked cost {e_cost:.3e} lowest_cost {e_low:.3e}, argmin differs at "
          f"{int((idx != g['argmin']).sum())} pixels (near ties: {int(g['near_tie'].sum())})")
    assert e_cost < FWD_TOL
    assert idx.dtype == torch.int64 and torch.equal(idx[keep], g["argmin"][keep])
    assert e_low < FWD_TOL
    assert float(cost[2].abs().max()) == 0.0                          # every frame zeroed -> skipped item
    # item 1 has frame 1 zeroed: the same bits as the kernel run on the two frames that are left
    two = ops.cost_volume_multi(g["cur"][1:2], g["lookup"][1:2, [0, 2]].contiguous(), g["poses"][1:2, [0, 2]].contiguous(),
                                g["K"][1:2], g["inv_K"][1:2], g["bins"])
    assert float((two != 0).float().mean()) > 0.2 and torch.equal(cost[1:2], two)


def _ragged(F, device, dtype=torch.bfloat16):
    """The shape of test_cost_volume_bf16_packed_pairs_is_bit_identical_to_the_fp32_kernel with F frames: C = 30 (odd pair
    count), ragged map, more than one block; a distinct pose per frame, item 1 with frame 0 zeroed."""
    g = torch.Generator().manual_seed(23 + F)
    B, C, h, w, D = 3, 30, 21, 37, 13
    cur = torch.randn(B, C, h, w, generator=g).to(dtype).to(device)
    look = torch.randn(B, F, C, h, w, generator=g).to(dtype).to(device)
    K, inv_K = synth.kitti_K(4 * h, 4 * w, 2)
    K, inv_K = K[None].repeat(B, 1, 1).to(device), inv_K[None].repeat(B, 1, 1).to(device)
    T = torch.eye(4)[None, None].repeat(B, F, 1, 1)
    for f in range(F):
        T[:, f, 2, 3], T[:, f, 0, 3] = 0.8 - 0.5 * f, 0.3 - 0.25 * f
    T[1, 0] = 0.0
    bins = torch.exp(torch.linspace(-2.3, 2.3, D)).to(device)
    return cur, look, T.to(device), K, inv_K, bins


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_lookup_frame_is_the_single_frame_kernel(device, golden, dtype):
    """F = 1 of the one sweep kernel gives the bits of the dedicated single-frame kernels it replaced, recorded at the last
    commit that had them (tests/golden/cost_volume_f1_bits.npz, tools/gen_golden_cost_volume_f1.py)."""
    from ppeadepth import ops
    cur, look, T, K, inv_K, bins = _ragged(1, device, dtype)
    want = golden("cost_volume_f1_bits")["f32" if dtype == torch.float32 else "bf16"].to(device)
    a = ops.cost_volume_multi(cur, look, T, K, inv_K, bins)
    b = ops.cost_volume(cur, look[:, 0], T[:, 0], K, inv_K, bins)
    assert float((a[0] != 0).float().mean()) > 0.2 and float(a[1].abs().max()) == 0.0          # item 1 is skipped
    assert torch.equal(a, want) and torch.equal(b, want)


@pytest.mark.parametrize("F", [2, 3, 4])
def test_frame_order_skip_and_bf16_pairs(device, F):
    """Measured, fp32 kernel vs CPU composite: F = 2 1.5e-07, F = 3 1.4e-06, F = 4 1.2e-06; non-zero share of item 0 0.72."""
    from ppeadepth import ops
    from ppeadepth.inference import cost_volume_cpu
    cur, look, T, K, inv_K, bins = _ragged(F, device)
    a = ops.cost_volume_multi(cur, look, T, K, inv_K, bins)                       # packed channel pairs
    b = ops.cost_volume_multi(cur.float(), look.float(), T, K, inv_K, bins)       # fp32 kernel on the widened features
    assert torch.equal(a, b)
    ref = cost_volume_cpu(cur.float().cpu(), look.float().cpu(), T.cpu(), K.cpu(), inv_K.cpu(), bins.cpu())
    e = rel_err(b.cpu(), ref)
    share = float((b[0] != 0).float().mean())
    print(f"F = {F}: fp32 kernel vs CPU composite {e:.3e}, non-zero share of item 0 {share:.2f}")
    assert e < FWD_TOL
    assert share > 0.2
    # item 1's first frame is skipped: the other frames alone give the same bits (F = 2: the F = 1 instantiation)
    rest = ops.cost_volume_multi(cur[1:2].float(), look[1:2, 1:].float().contiguous(), T[1:2, 1:].contiguous(), K[1:2],
                                 inv_K[1:2], bins)
    assert torch.equal(b[1:2], rest)


def test_more_than_four_lookup_frames_are_refused(device):
    from ppeadepth import _abi, ops
    cur, look, T, K, inv_K, bins = _ragged(5, device)
    with pytest.raises(_abi.PpeaKernelError):
        ops.cost_volume_multi(cur, look, T, K, inv_K, bins)
    with pytest.raises(_abi.PpeaKernelError):
        ops.cost_volume_multi(cur.float(), look.float(), T, K, inv_K, bins)
