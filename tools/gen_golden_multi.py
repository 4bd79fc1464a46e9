"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/cost_volume_multi.npz from the REFERENCE itself.

    python tools/gen_golden_multi.py

The reference's unmodified `RepLKMatchingAdapter.match_features` (the loop over the lookup frames, rkm.py:289-326),
`compute_confidence_mask`, the argmin block of `forward` (:449-453) and `indices_to_disparity` on three lookup frames,
loaded the way `oracle/gen_golden.py::gen_cost_volume` loads them and with its construction and scales: B = 3, F = 3,
C = 16, 16 x 24, 96 log bins 0.37 .. 14.5, fp32; a distinct pose per frame.  Item 1 has frame 1 zeroed (a partial skip),
item 2 all frames (the whole item skipped).  The fixture is data only.

Two properties are asserted here, on the reference's results alone:
  (a) both branches of the average are exercised: at >= 10 % of item 0's (bin, pixel) entries two or more frames
      contribute, and at >= 5 % exactly one does;
  (b) `near_tie` marks the pixels whose best and second-best `viz` cost differ by less than 1e-5 relative -- there the
      winning bin is decided by the last bits of an fp32 mean over channels, so a kernel that sums in another order may
      pick the neighbour.  Their share is <= TIE_CAP = 0.5 % (tests/test_inference_gpu.py).  A pixel without any matching
      cost (all 96 bins at the fill value 100: the 2-pixel border, a skipped item) is an exact tie that every
      implementation resolves to bin 0, and is not marked.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as rh  # noqa: E402
from oracle import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "cost_volume_multi.npz")
TIE_REL, TIE_CAP = 1e-5, 5e-3


def rnd(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@torch.no_grad()
def main():
    assert rh.reference_available(), "the reference checkout is needed to regenerate this fixture"
    rh.install_stubs()
    from ppeadepth.networks.replk_matching_adapter import RepLKMatchingAdapter as RMA
    from ppeadepth import layers as L
    B, F, C, h, w, D = 3, 3, 16, 16, 24, 96
    me = types.SimpleNamespace(num_depth_bins=D, matching_height=h, matching_width=w, depth_binning="log",
                               device=torch.device("cpu"), set_missing_to_max=True,
                               backprojector=L.BackprojectDepth(D, h, w), projector=L.Project3D(D, h, w))
    RMA.compute_depth_bins(me, torch.Tensor([0.37]), torch.Tensor([14.5]))
    cur = rnd(B, C, h, w, seed=131).relu()
    look = rnd(B, F, C, h, w, seed=132).relu()
    poses = torch.stack([L.transformation_from_parameters(rnd(B, 1, 3, seed=133 + 2 * f, scale=0.02),
                                                          rnd(B, 1, 3, seed=134 + 2 * f, scale=0.3), invert=True)
                         for f in range(F)], 1)
    poses[1, 1] *= 0          # item 1: frame 1 missing (rkm.py:294)
    poses[2] *= 0             # item 2: every frame missing
    K, inv_K = synth.kitti_K(4 * h, 4 * w, 2)
    K, inv_K = K[None].repeat(B, 1, 1), inv_K[None].repeat(B, 1, 1)
    cost, miss = RMA.match_features(me, cur, look, poses, K, inv_K)
    conf = RMA.compute_confidence_mask(me, cost * (1 - miss))
    viz = cost.clone()
    viz[viz == 0] = 100
    _mins, argmin = torch.min(viz, 1)
    lowest = RMA.indices_to_disparity(me, argmin)

    # (a) frames contributing per entry of item 0: a frame contributes where its own single-frame volume is not missing
    count = sum(1 - RMA.match_features(me, cur[:1], look[:1, f:f + 1], poses[:1, f:f + 1], K[:1], inv_K[:1])[1][0]
                for f in range(F))
    two, one = float((count >= 2).float().mean()), float((count == 1).float().mean())
    print(f"item 0: >= 2 frames at {two:.1%} of the entries, exactly one at {one:.1%}")
    assert two >= 0.10 and one >= 0.05, (two, one)
    # (b)
    best2 = torch.topk(viz, 2, dim=1, largest=False)[0]
    near_tie = (best2[:, 0] < 100) & ((best2[:, 1] - best2[:, 0]) < TIE_REL * best2[:, 1].abs())
    share = float(near_tie.float().mean())
    print(f"near ties: {int(near_tie.sum())} pixels = {share:.3%}")
    assert share <= TIE_CAP, share

    np.savez_compressed(OUT, cur=cur.numpy(), lookup=look.numpy(), poses=poses.numpy(), K=K.numpy(), inv_K=inv_K.numpy(),
                        bins=me.depth_bins.numpy(), cost=cost.numpy(), missing=miss.numpy().astype(np.uint8),
                        confidence=conf.numpy(), argmin=argmin.numpy(), lowest_cost=lowest.numpy(),
                        near_tie=near_tie.numpy())
    print(f"wrote {OUT}  {os.path.getsize(OUT) / 1024:.0f} KiB")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
