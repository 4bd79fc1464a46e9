"""TEST INFRASTRUCTURE ONLY -- what the REFERENCE's own checkpoint files look like.

    python tools/gen_checkpoint_golden.py

Runs only where the reference tree exists (oracle.ref_harness.reference_available).  Calls the reference's unmodified
`Trainer.save_model_debug` (trainer.py:1290-1321) on the harness trainer (oracle.ref_harness.build_reference_trainer) with a
stub accelerator and a stock `torch.optim.Adam` over `[p for p in model.parameters() if p.requires_grad]` (trainer.py:141-142)
that has taken one step on zero gradients, writes the three files into a scratch folder, reads them back and stores ONLY
names, shapes, dtypes and scalars in tests/golden/checkpoint_spec.npz:
  files                      the file names in the folder
  track_keys                 the key set of track.pth
  group_keys / state_keys    the keys of adam.pth's param_groups[0] and of one state entry
  step_dtype / step_shape    of a state entry's `step`
  adam_names / adam_shapes   the parameter name and moment shape behind every index of adam.pth (31B, Stage 1)
  model_keys_match           1 when model.pth's keys are the model's state_dict keys in order
No tensor of the checkpoint and no reference code is stored.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402


class _Accelerator(rh.FakeAccelerator):
    """The two Accelerate methods save_model_debug touches (trainer.py:1305-1306), on one process."""

    def unwrap_model(self, model):
        return model

    def save(self, obj, path):
        torch.save(obj, path)


def main():
    assert rh.reference_available(), "the reference tree is not on this machine"
    opt = rh.parse_options(["--rep_size", "b"])
    torch.manual_seed(0)
    with rh.scratch_cwd():
        from ppeadepth import networks
        model = networks.RepDepth(opt)
    tr = rh.build_reference_trainer(opt, model)
    tr.acc = _Accelerator()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    params = [p for p in model.parameters() if p.requires_grad]
    assert [id(p) for _, p in named] == [id(p) for p in params]
    tr.model_optimizer = torch.optim.Adam(params, opt.learning_rate)
    for p in params:
        p.grad = torch.zeros_like(p)
    tr.model_optimizer.step()
    folder = tempfile.mkdtemp(prefix="ppea_ckpt_")
    try:
        tr.save_model_debug(folder)
        files = sorted(os.listdir(folder))
        model_sd = torch.load(os.path.join(folder, "model.pth"), map_location="cpu")
        track = torch.load(os.path.join(folder, "track.pth"), map_location="cpu")
        adam = torch.load(os.path.join(folder, "adam.pth"), map_location="cpu")
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    group, entry = adam["param_groups"][0], adam["state"][0]
    assert group["params"] == list(range(len(params))) and sorted(adam["state"]) == group["params"]
    for i, (n, p) in enumerate(named):
        assert tuple(adam["state"][i]["exp_avg"].shape) == tuple(p.shape), n
    gg.save("checkpoint_spec",
            files=np.array(files), track_keys=np.array(sorted(track)), group_keys=np.array(sorted(group)),
            state_keys=np.array(sorted(entry)), step_dtype=np.array(str(entry["step"].dtype)),
            step_shape=np.array(entry["step"].shape, dtype=np.int64),
            adam_names=np.array([n for n, _ in named]),
            adam_shapes=np.array([";".join(str(d) for d in p.shape) for _, p in named]),
            model_keys_match=np.array(int(list(model_sd) == list(model.state_dict()))))


if __name__ == "__main__":
    main()
