"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/e2e_mf_two_past.npz and e2e_mf_future.npz from the REFERENCE itself.

    python tools/gen_golden_multiframe.py

The reference's unmodified `Trainer.process_batch` + backward with several matching frames, by the recipe of
`oracle/gen_golden.py::gen_e2e(..., conditioned=True)`: B = 2, 64x96, RepLKNet-31B, `synth.fill_state_dict(model,
conditioned=True)`, `synth.make_rendered_inputs(B, H, W, frame_ids=(0, -1, 1, -2))`, torch / random seed 1 for the step.

    e2e_mf_two_past   --num_matching_frames 2   matching_ids [0, -1, -2]
    e2e_mf_future     --use_future_frame        matching_ids [0, 1, -1]

Same key scheme as gen_e2e (`loss:`, `out:`, `grad_sum:` / `grad_abs:` / `grad_head:`, `buf:`, `bins_after`, `meta`; the
4096-element `grad_sample:` of the bf16 comparisons is left out, which keeps each file under 1 MiB), plus `in:relative_pose|f` for every
lookup frame and `matching_ids`.  Like oracle/gen_golden.py this imports the reference at run time; the fixtures are data only.
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as rh  # noqa: E402
from oracle import synth  # noqa: E402
from oracle.gen_golden import GRAD_KEYS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
B, H, W, SEED = 2, 64, 96, 1
FRAMES = (0, -1, 1, -2)
CONFIGS = {"e2e_mf_two_past": ["--num_matching_frames", "2"], "e2e_mf_future": ["--use_future_frame"]}
BUFFERS = ("encoder.replk.stem.0.bn.running_mean", "encoder.replk.stem.0.bn.running_var",
           "mono_encoder.stages.3.blocks.3.pw2.bn.running_var", "pose_encoder.encoder.bn1.running_mean",
           "pose_encoder.encoder.layer4.1.bn2.running_var")


def run(name, extra):
    opt = rh.parse_options(["--height", str(H), "--width", str(W), "--batch_size", str(B)] + list(extra))
    torch.manual_seed(0)
    random.seed(0)
    with rh.scratch_cwd():
        from ppeadepth import networks
        model = networks.RepDepth(opt)
    model.train()
    synth.fill_state_dict(model, conditioned=True)
    tr = rh.build_reference_trainer(opt, model)
    inputs = synth.make_rendered_inputs(B, H, W, frame_ids=FRAMES)
    torch.manual_seed(SEED)
    random.seed(SEED)
    outputs, losses = tr.process_batch(inputs, True)
    losses["loss"].backward()
    arrays = {"meta": np.array([B, H, W, 1, SEED]), "matching_ids": np.array(model.matching_ids)}
    for k, v in losses.items():
        arrays["loss:" + k] = v
    for k, v in outputs.items():
        arrays["out:" + ("|".join(str(s) for s in k) if isinstance(k, tuple) else k)] = v
    for f in model.matching_ids[1:]:
        arrays[f"in:relative_pose|{f}"] = inputs[("relative_pose", f)]
    params = dict(model.named_parameters())
    for k in GRAD_KEYS:
        g = params[k].grad
        arrays["grad_sum:" + k] = g.double().sum().float()
        arrays["grad_abs:" + k] = g.double().abs().sum().float()
        arrays["grad_head:" + k] = g.reshape(-1)[:32].clone()
    sd = model.state_dict()
    for k in BUFFERS:
        arrays["buf:" + k] = sd[k]
    mn, mx = tr.depth_bin_tracker.compute()
    arrays["bins_after"] = torch.stack([mn.reshape(()), mx.reshape(())])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in arrays.items()})
    low = outputs["lowest_cost"]
    print(f"{name}: matching_ids {model.matching_ids} loss {float(losses['loss']):.6f} "
          f"augmentation_mask {outputs['augmentation_mask'].flatten().tolist()} "
          f"t_z {[round(float(inputs[('relative_pose', f)][1, 2, 3]), 4) for f in model.matching_ids[1:]]} "
          f"lowest_cost below its maximum at {float((low < low.max()).float().mean()):.1%} of the pixels; "
          f"wrote {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    if not rh.reference_available():
        raise SystemExit("reference tree not present: goldens can only be regenerated where the reference is")
    rh.install_stubs()
    torch.set_num_threads(8)
    for name, extra in CONFIGS.items():
        run(name, extra)


if __name__ == "__main__":
    main()
