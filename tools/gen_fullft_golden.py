"""TEST INFRASTRUCTURE ONLY -- the full fine-tuning fixtures (`--adapter --fullft_reb`), from the REFERENCE itself.

    python tools/gen_fullft_golden.py

Runs only where the reference tree exists (oracle.ref_harness.reference_available).  Writes
  tests/golden/e2e_small_fullft.npz   the reference's unmodified Trainer.process_batch + backward at B = 2, 64 x 96 with
                                      every backbone weight trainable (oracle.gen_golden.gen_e2e), gradients of KEYS
  tests/golden/fullft_spec.npz        names / requires_grad of RepDepth(opt).named_parameters() for 31B and 31L
Only arrays and key names are stored.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402


def _encoder_keys(prefix, last=0):
    """`last`: the RepLKBlock of stage 3 that is sampled (with the ConvFFN behind it).  DropPath draws per sample: at B = 2
    the teacher's first stage-3 pair is dropped for both samples under the fixture's seed, so its gradients are exactly zero
    in the reference as well -- the second pair is sampled there."""
    first = {0: 0, 1: 0, 2: 0, 3: last}
    keys = [f"{prefix}stages.{s}.blocks.{first[s]}.large_kernel.lkb_origin.conv.weight" for s in range(4)]   # k = 31, 29, 27, 13
    keys.append(f"{prefix}stages.0.blocks.0.large_kernel.small_conv.conv.weight")
    for s in (0, 2, 3):
        for blk in (first[s], first[s] + 1):                                  # a RepLKBlock and the ConvFFN behind it
            keys += [f"{prefix}stages.{s}.blocks.{blk}.{pw}.conv.weight" for pw in ("pw1", "pw2")]
    keys += [f"{prefix}stem.{i}.conv.weight" for i in range(4)]
    keys += [f"{prefix}transitions.{t}.{i}.conv.weight" for t in (0, 2) for i in (0, 1)]
    keys += [f"{prefix}stages.1.blocks.1.pw1.bn.weight", f"{prefix}stages.1.blocks.1.pw1.bn.bias"]
    return keys


KEYS = (_encoder_keys("encoder.replk.") + _encoder_keys("mono_encoder.", last=2)
        + ["encoder.replk.stages.0.blocks.0.adapter.D_fc1.weight",
           "mono_encoder.stages.1.blocks.2.adapter.D_fc1.weight",
           "depth.upconvs_0.0.conv.conv.weight"])
assert all(k in gg.GRAD_KEYS for k in KEYS[-3:])


def gen_spec():
    """Names and trainable flags of RepDepth(opt).named_parameters() under --adapter --fullft_reb (31B and 31L)."""
    arrays = {}
    for size in ("b", "l"):
        opt = rh.parse_options(["--rep_size", size, "--adapter", "--fullft_reb"])
        torch.manual_seed(0)
        with rh.scratch_cwd():
            from ppeadepth import networks
            model = networks.RepDepth(opt)
        named = list(model.named_parameters())
        arrays[f"{size}:names"] = np.array([n for n, _ in named])
        arrays[f"{size}:trainable"] = np.array([int(p.requires_grad) for _, p in named])
        del model
    gg.save("fullft_spec", **arrays)


def main():
    if not rh.reference_available():
        raise SystemExit("reference tree not present: goldens can only be regenerated in the build container")
    rh.install_stubs()
    torch.set_num_threads(8)
    gen_spec()
    gg.gen_e2e("e2e_small_fullft", 2, 64, 96, extra=["--fullft_reb"], stride=2, grad_keys=KEYS)
    ref = os.path.getsize(os.path.join(gg.OUT, "e2e_small.npz"))
    got = os.path.getsize(os.path.join(gg.OUT, "e2e_small_fullft.npz"))
    print(f"e2e_small_fullft.npz {got} bytes (e2e_small.npz: {ref})")
    z = np.load(os.path.join(gg.OUT, "e2e_small_fullft.npz"))
    dead = [k for k in KEYS if float(z["grad_abs:" + k]) == 0.0]
    assert not dead, f"the reference's gradient is exactly zero (DropPath dropped every sample): {dead}"
    assert got <= ref, "fixture larger than e2e_small.npz"


if __name__ == "__main__":
    main()
