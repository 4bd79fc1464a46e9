"""Checkpoint FILES (reference: trainer.py:1290-1381, `save_model_debug` / `load_model`).  No engine knowledge: this
module reads and writes the reference's three files and checks what can be checked on the documents alone.

  model.pth   a plain `state_dict` (fp32); applied with strict=False, read with map_location="cpu".
  track.pth   {"height", "width"} and, only when the adaptive depth bins are live (not --notadabins and not
              --freeze_teacher_and_pose, trainer.py:1313-1317), {"min_depth_bin", "max_depth_bin"} from `DepthBins.compute()`.
              Everything this build needs beyond the reference sits under ONE extra key, "ppea" (`PPEA_FIELDS`); the
              reference reads track.pth with `.get`, so the key does not disturb it, and a file without it loads here.
  adam.pth    `torch.optim.Adam.state_dict()` in the REFERENCE's parameter order: index i is the i-th of
              `[p for p in model.parameters() if p.requires_grad]` (trainer.py:141-142), with exp_avg, exp_avg_sq and step
              per index and torch's own keys in param_groups[0].
"""
import collections
import os

import torch

FORMAT_VERSION = 1

# what track.pth["ppea"] holds
PPEA_FIELDS = ("version", "step", "epoch", "scheduler", "lr", "bins_updated", "rng_mode", "python_random", "torch_cpu_rng",
               "device_rng", "world_size", "bf16_params")

Documents = collections.namedtuple("Documents", ["model", "track", "adam"])


def bins_live(opt, freeze_tp):
    """trainer.py:1313: the depth-bin estimates are saved only while the adaptive bins are being tracked."""
    return not getattr(opt, "notadabins", False) and not freeze_tp


def track_document(opt, freeze_tp, bins, ppea=None):
    """trainer.py:1309-1317.  bins: (min, max) of `DepthBins.compute()` -- a collective with several ranks, so every rank
    calls it -- or None; they are written only when `bins_live`."""
    track = {"height": opt.height, "width": opt.width}
    if bins_live(opt, freeze_tp):
        track["min_depth_bin"], track["max_depth_bin"] = bins
    if ppea is not None:
        missing = [k for k in PPEA_FIELDS if k not in ppea]
        if missing:
            raise KeyError(f"track.pth['ppea'] lacks {missing}")
        track["ppea"] = ppea
    return track


def write_folder(folder, model_sd, track, adam_sd):
    """The reference's three files.  With several ranks only rank 0 calls this."""
    os.makedirs(folder, exist_ok=True)
    torch.save(model_sd, os.path.join(folder, "model.pth"))
    torch.save(track, os.path.join(folder, "track.pth"))
    torch.save(adam_sd, os.path.join(folder, "adam.pth"))


def read_folder(folder, transfer=False):
    """-> Documents(model, track, adam).  transfer (the reference's --ktf): model.pth only, track and adam are None.
    A folder without adam.pth gives adam = None (a fresh optimizer), with the reference's message."""
    folder = os.path.expanduser(folder)
    assert os.path.isdir(folder), "Cannot find folder {}".format(folder)
    print("loading model from folder {}".format(folder))
    model_sd = torch.load(os.path.join(folder, "model.pth"), map_location="cpu")
    if transfer:
        return Documents(model_sd, None, None)
    track = torch.load(os.path.join(folder, "track.pth"), map_location="cpu")
    adam_path = os.path.join(folder, "adam.pth")
    adam_sd = None
    if os.path.isfile(adam_path):
        print("Loading Adam weights")
        adam_sd = torch.load(adam_path, map_location="cpu")
    else:
        print("Cannot find Adam weights so Adam is randomly initialized")
    return Documents(model_sd, track, adam_sd)


def check_adam(adam_sd, shapes):
    """An Adam document against the shapes of the trainable tensors in the reference's order.  ValueError when the number of
    parameters or a moment's shape disagrees (what `Optimizer.load_state_dict` raises, and what trainer.py:1374-1379
    catches), or when the per-index `step` values differ from one another (the engine keeps ONE counter).
    -> the common step (0.0 for a document without state)."""
    groups = adam_sd["param_groups"]
    n = sum(len(g["params"]) for g in groups)
    if len(groups) != 1 or n != len(shapes):
        raise ValueError(f"adam.pth describes {n} parameters in {len(groups)} group(s), the model trains {len(shapes)} in one")
    steps = set()
    for i, st in adam_sd["state"].items():
        if not 0 <= int(i) < n:
            raise ValueError(f"adam.pth has state for index {i} of {n} parameters")
        for k in ("exp_avg", "exp_avg_sq"):
            if tuple(st[k].shape) != tuple(shapes[int(i)]):
                raise ValueError(f"adam.pth {k}[{i}] has shape {tuple(st[k].shape)}, the parameter {tuple(shapes[int(i)])}")
        steps.add(float(st["step"]))
    if len(steps) > 1:
        raise ValueError(f"adam.pth holds different step counts per parameter ({sorted(steps)[:4]}...): "
                         "the flat optimizer has one counter for all tensors")
    return steps.pop() if steps else 0.0


def remap_adam(adam_sd, perm):
    """Optimizer document with its indices re-ordered: entry j of the result is entry perm[j] of `adam_sd`."""
    state = {j: adam_sd["state"][i] for j, i in enumerate(perm) if i in adam_sd["state"]}
    groups = [dict(g) for g in adam_sd["param_groups"]]
    groups[0]["params"] = list(range(len(perm)))
    return {"state": state, "param_groups": groups}
