"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/infer.npz from the REFERENCE itself.

    python tools/gen_infer_golden.py

The reference's unmodified modules in eval() with `synth.fill_state_dict(model, conditioned=True)` (non-trivial running
statistics) on `synth.make_rendered_inputs(2, H, W)`, computed the way the reference's `Trainer.val` does it
(trainer.py:676-752): pose of the lookup frame from the pose network, depth-bin tracker at its initial bins (0.1, 10),
matching encoder + decoder, and the single-frame teacher.  Stored per size: the network disparities `("disp", 0)` of the
teacher and of the multi-frame network, `lowest_cost` and the 4x4 pose.  At 192x640 the maps are stored at spatial
stride 4, at 64x96 whole.  Like oracle/gen_golden.py this imports the reference at run time; the fixture is data only.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as rh  # noqa: E402
from oracle import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "infer.npz")
MIN_BIN, MAX_BIN = 0.1, 10.0          # DepthBinTracker before its first update (trainer.py:41-69, 736-739)


@torch.no_grad()
def run(B, H, W, stride):
    opt = rh.parse_options(["--height", str(H), "--width", str(W), "--batch_size", str(B)])
    torch.manual_seed(0)
    with rh.scratch_cwd():
        from ppeadepth import networks
        from ppeadepth.layers import transformation_from_parameters
        model = networks.RepDepth(opt)
    synth.fill_state_dict(model, conditioned=True)
    model.eval()
    data = synth.make_rendered_inputs(B, H, W)
    c0, cm1 = data[("color", 0, 0)], data[("color", -1, 0)]
    axisangle, translation = model.pose([model.pose_encoder(torch.cat([cm1, c0], 1))])
    pose = transformation_from_parameters(axisangle[:, 0], translation[:, 0], invert=True)
    feats, lowest_cost, _ = model.encoder(c0, cm1[:, None], pose[:, None], data[("K", 2)], data[("inv_K", 2)],
                                          torch.Tensor([MIN_BIN]), torch.Tensor([MAX_BIN]))
    disp = model.depth(feats)[("disp", 0)]
    disp_mono = model.mono_depth(model.mono_encoder(c0))[("disp", 0)]
    tag = f"{H}x{W}:"
    return {tag + "meta": np.array([B, H, W, stride]),
            tag + "disp": disp[..., ::stride, ::stride].numpy(),
            tag + "disp_mono": disp_mono[..., ::stride, ::stride].numpy(),
            tag + "lowest_cost": lowest_cost[..., ::stride, ::stride].numpy(),
            tag + "pose": pose.numpy()}


def main():
    assert rh.reference_available(), "the reference checkout is needed to regenerate this fixture"
    rh.install_stubs()
    arrays = {"bins": np.array([MIN_BIN, MAX_BIN], dtype=np.float32)}
    arrays.update(run(2, 192, 640, 4))
    arrays.update(run(2, 64, 96, 1))
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}  {os.path.getsize(OUT) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
