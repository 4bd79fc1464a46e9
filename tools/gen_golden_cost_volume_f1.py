"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/cost_volume_f1_bits.npz: the bits of the single-frame cost volume.

    python tools/gen_golden_cost_volume_f1.py [--out FILE]          (needs the GPU)

Run at commit 711c3b4, the last one with the dedicated single-frame kernels (one for fp32 features, one for bf16 channel
pairs, four bins per thread): the raw `[3,13,21,37]` fp32 volumes that `ops.cost_volume` returns there for the inputs of
tests/test_cost_volume_multi_gpu.py::_ragged(1, device, dtype), with fp32 and with bf16 features.  The one sweep kernel
that replaced them has to reproduce these bits for F = 1 (test_one_lookup_frame_is_the_single_frame_kernel).  Run at a later
commit it records that commit's bits, which is only of use for comparing them with the committed file.

The inputs come from the test module itself (seeded, made on the CPU), so the fixture holds outputs only.  The volume is
computed twice and the two results must be equal bit for bit; the SHA-256 of each array's bytes is printed so that two runs
of this script can be compared (the .npz container carries time stamps, its bytes are not comparable).
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ppea-depth_amd"), os.path.join(ROOT, "tests")]

OUT = os.path.join(ROOT, "tests", "golden", "cost_volume_f1_bits.npz")


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from ppeadepth import ops
    from test_cost_volume_multi_gpu import _ragged
    dev = torch.device("cuda:0")
    arrays = {}
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        cur, look, T, K, inv_K, bins = _ragged(1, dev, dtype)
        a = ops.cost_volume(cur, look[:, 0], T[:, 0], K, inv_K, bins)
        b = ops.cost_volume(cur, look[:, 0], T[:, 0], K, inv_K, bins)
        assert a.dtype == torch.float32 and tuple(a.shape) == (3, 13, 21, 37) and torch.equal(a, b)
        share = float((a[0] != 0).float().mean())
        assert share > 0.2 and float(a[1].abs().max()) == 0.0, share          # item 1 is skipped
        arrays[name] = a.cpu().numpy()
        print(f"{name}: non-zero share of item 0 {share:.2f}, sha256 {hashlib.sha256(arrays[name].tobytes()).hexdigest()}")
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}  {os.path.getsize(args.out) / 1024:.0f} KiB")
    assert os.path.getsize(args.out) < 1 << 20


if __name__ == "__main__":
    main()
