"""Watching a run without stalling it: a ring of per-step rows that lives where the step runs.

    log = RunLog(device, capacity=256, names=("loss", "lr"))
    log.append(step, {"loss": losses["loss"], "lr": engine.adam_state[1]}, engine.flat.flat, engine.flat.numel)
    rows = log.read()           # ONE device -> host copy, every log interval

`append` is `ops.run_monitor`: two launches on the caller's stream (csrc/run_monitor.hip), no host read and -- after the
first call -- no allocation.  The slot a row goes to is counted on the device; the host only remembers how many rows it has
read.  On the host (`device="cpu"`) the same rows are computed with torch in float64.
"""
import numpy as np
import torch

from . import ops
from ._abi import PpeaKernelError

GRAD_COLUMNS = ("grad_l2", "grad_max_abs", "grad_nonfinite")


class Rows(list):
    """What `RunLog.read()` returns: the rows appended since the last read, oldest first, each a dict of `step` (int), the
    named scalars (numpy float32 with the source's bits, or None where the scalar was absent in that row), `grad_l2`,
    `grad_max_abs` (numpy float32) and `grad_nonfinite` (int).  `dropped`: rows that were overwritten before they were read;
    `first_bad_step`: the step of the first row ever appended with a non-finite scalar or gradient element, or -1."""

    dropped = 0
    first_bad_step = -1


class RunLog:
    def __init__(self, device, capacity=256, names=("loss", "loss/0", "reproj_loss/0", "consistency_loss/0",
                                                     "min_depth_bin", "max_depth_bin", "lr")):
        names = tuple(names)
        if len(names) > ops.MONITOR_MAX_SCALARS:
            raise PpeaKernelError(f"RunLog: {len(names)} scalars, a row holds {ops.MONITOR_MAX_SCALARS}")
        if len(set(names)) != len(names) or set(names) & ({"step"} | set(GRAD_COLUMNS)):
            raise ValueError(f"RunLog: scalar names must be distinct and none of step, {', '.join(GRAD_COLUMNS)}: {names}")
        if int(capacity) < 1:
            raise ValueError(f"RunLog: capacity {capacity}")
        self.device = torch.device(device)
        self.names, self.capacity = names, int(capacity)
        W = ops.MONITOR_ROW_WORDS
        # state and ring share one buffer, so that one copy brings both to the host: row 0 holds the state
        host = torch.zeros((self.capacity + 1) * W, dtype=torch.int32)
        host[:4].view(torch.int64)[1] = -1
        on_gpu = self.device.type == "cuda"
        self._host = host.pin_memory() if on_gpu else None
        self._buf = host.to(self.device) if on_gpu else host
        self.state = self._buf[:4].view(torch.int64)
        self.ring = self._buf[W:].view(self.capacity, W)
        self._scratch = None
        self._read = 0

    def append(self, step, scalars, grads=None, n=None, grad_scale=1.0):
        """One row: `scalars` maps names of this log to 0-dim / one-element fp32 tensors (a name left out, or None, is
        absent in the row); `grads` the flat fp32 gradient buffer, of which the first `n` elements count (default all)."""
        unknown = [k for k in scalars if k not in self.names]
        if len(scalars) > ops.MONITOR_MAX_SCALARS or unknown:
            raise PpeaKernelError(f"RunLog.append: {len(scalars)} scalars {sorted(map(str, scalars))}; this log holds {self.names}")
        if grads is not None and self._scratch is None and self.device.type == "cuda":
            self._scratch = ops.run_monitor_scratch(self.device)
        ops.run_monitor([scalars.get(k) for k in self.names], grads, n, step, grad_scale, self.ring, self.state,
                        self._scratch)

    def read(self):
        """-> `Rows` appended since the last read.  ONE device -> host copy (on the current stream, behind the appends)."""
        if self._host is not None:
            self._host.copy_(self._buf, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            words = self._host.numpy()
        else:
            words = self._buf.numpy()
        W = ops.MONITOR_ROW_WORDS
        count, first_bad = (int(v) for v in words[:4].view(np.int64))
        ring = words[W:].reshape(self.capacity, W).copy()
        rows = Rows()
        new = count - self._read
        rows.dropped = max(0, new - self.capacity)
        rows.first_bad_step = first_bad
        for i in range(count - min(new, self.capacity), count):
            w = ring[i % self.capacity]
            f, mask = w.view(np.float32), int(w[10])
            step, bad = (int(v) for v in w[12:16].view(np.int64))
            row = {"step": step}
            for k, name in enumerate(self.names):
                row[name] = f[k] if mask >> k & 1 else None
            row.update(grad_l2=f[8], grad_max_abs=f[9], grad_nonfinite=bad)
            rows.append(row)
        self._read = count
        return rows
