"""The validation set resident on the device.

A run validates on the same frames every time, and the reference re-decodes them every time (for Cityscapes 2 x 1525 PNGs
of 2048 x 1024).  `ValidationStore` keeps, while the FIRST validation's batches pass, what `Trainer.predict_disps` reads of
them and nothing else:

    ("color", f, 0)   frame 0 and the lookup frames, as uint8 [N, F, 3, H, W]
    ("K", 2), ("inv_K", 2)                            fp32 [N, 4, 4] each

and every later validation reads its batches from there: no loader worker starts, nothing is decoded or uploaded.

Why uint8 is enough.  A colour entry is a `ToTensor` product, exactly k / 255 in fp32 for a byte k, so rint(x * 255) recovers
k and the pipeline's own conversion gives x back: `ops.color_jitter_u8` with the all-zero parameter table (backend "hip",
what `_PyramidPipeline._colors_hip` launches without augmentation) or the true division by `_PyramidPipeline.unit` (backend
"torch").  Never a multiplication by 1 / 255: that is another fp32 value for 126 of the 256 levels (input_pipeline.py).
The store does not trust this: while a batch is added, its bytes are converted back by the path `batches()` uses and
compared with the floats they came from, the mismatches are counted on the device, and `finish()` reads the count once
and raises if it is not zero.  A pipeline change that breaks the equivalence cannot go unnoticed.

Footprint: N x F x 3 x H x W bytes -- 1525 x 2 x 3 x 192 x 512 = 0.84 GiB for Cityscapes, 697 x 2 x 3 x 192 x 640 = 0.49 GiB
for the eigen split.
"""
import torch


class ValidationStoreError(RuntimeError):
    """A value that went into the store does not come back as the float it was."""


class ValidationStore:
    """frame_ids: frame 0 and the lookup frames, in the order the batches are rebuilt with; count: items of the split;
    unit: the pipeline's `ToTensor` divisor (a tensor on `device`)."""

    def __init__(self, frame_ids, count, device, unit, backend):
        if backend not in ("hip", "torch"):
            raise ValueError(f"backend {backend!r}: expected 'hip' or 'torch'")
        self.frame_ids, self.count, self.device = tuple(int(f) for f in frame_ids), int(count), torch.device(device)
        self.unit, self.backend = unit, backend
        self.colors = self.K = self.inv_K = None
        self._zero_tables = {}
        self.begin()

    def begin(self):
        """Start (or start over) the pass that fills the store."""
        self.filled, self.complete = 0, False
        self._bad = torch.zeros((), device=self.device, dtype=torch.int64)

    def nbytes(self):
        return 0 if self.colors is None else self.colors.numel() + 4 * (self.K.numel() + self.inv_K.numel())

    def _to_float(self, u8):
        """uint8 [M,3,H,W] -> the fp32 `ToTensor` product, by the pipeline's own conversion."""
        if self.backend == "hip":
            from . import ops
            M = u8.shape[0]
            if M not in self._zero_tables:
                self._zero_tables[M] = torch.zeros(M, ops.JITTER_PARAM_WORDS, device=self.device, dtype=torch.int32)
            return ops.color_jitter_u8(u8, self._zero_tables[M], None)[0]
        return u8.to(torch.float32) / self.unit

    @torch.no_grad()
    def add(self, data):
        """Keep the next batch of the split.  data: the row-P dictionary of the evaluation pipeline."""
        first = data[("color", self.frame_ids[0], 0)]
        B, _, H, W = first.shape
        if self.filled + B > self.count:
            raise ValueError(f"{self.filled + B} items for a store of {self.count}")
        if self.colors is None:
            self.colors = torch.empty(self.count, len(self.frame_ids), 3, H, W, device=self.device, dtype=torch.uint8)
            self.K = torch.empty(self.count, 4, 4, device=self.device, dtype=torch.float32)
            self.inv_K = torch.empty_like(self.K)
        x = torch.stack([data[("color", f, 0)].to(self.device) for f in self.frame_ids])             # [F,B,3,H,W]
        if x.dtype != torch.float32 or tuple(x.shape[1:]) != (B,) + tuple(self.colors.shape[2:]):
            raise ValueError(f"colour entries {x.dtype} {tuple(x.shape[1:])}: the store holds fp32 "
                             f"{(B,) + tuple(self.colors.shape[2:])}")
        k = torch.round(x * 255).clamp_(0, 255).to(torch.uint8)
        self._bad += (self._to_float(k.view(-1, 3, H, W)).view_as(x) != x).sum()      # NaN counts: it equals nothing
        rows = slice(self.filled, self.filled + B)
        self.colors[rows] = k.transpose(0, 1)
        self.K[rows] = data[("K", 2)]
        self.inv_K[rows] = data[("inv_K", 2)]
        self.filled += B

    def finish(self):
        """End of the filling pass: ONE read of the device, the number of values that do not convert back."""
        if self.filled != self.count:
            raise ValueError(f"{self.filled} items passed for a store of {self.count}")
        bad = int(self._bad.item())
        if bad:
            self.begin()
            raise ValidationStoreError(f"{bad} colour values of the validation batches are not k / 255 for a byte k: the "
                                       "uint8 store cannot reproduce them (has the evaluation pipeline's ToTensor changed?)")
        self.complete = True

    @torch.no_grad()
    def batches(self, batch_size):
        """The batches of the filling pass again (the last one partial), equal to them bit for bit in the kept entries."""
        if not self.complete:
            raise ValueError("the store is read after a complete filling pass (add ... finish)")
        F = len(self.frame_ids)
        for b0 in range(0, self.count, batch_size):
            b1 = min(b0 + batch_size, self.count)
            u8 = self.colors[b0:b1].transpose(0, 1).contiguous()                                # frame-major, as the pipeline
            color = self._to_float(u8.view((-1,) + tuple(u8.shape[2:]))).view((F, b1 - b0) + tuple(u8.shape[2:]))
            data = {("color", f, 0): color[fi] for fi, f in enumerate(self.frame_ids)}
            data[("K", 2)], data[("inv_K", 2)] = self.K[b0:b1], self.inv_K[b0:b1]
            yield data
