"""Input pipeline on the device: raw uint8 frames -> the row-P dictionary `process_batch` consumes.

Replaces, for a whole batch at once, what the reference does per item on CPU workers with PIL / torchvision
(datasets/mono_dataset.py:89-112 `preprocess`, :143-190 `__getitem__`): horizontal flip, the LANCZOS image pyramid
(scale s is resized from scale s-1, like the reference's chained `transforms.Resize`), ColorJitter with one parameter
draw per item shared by all its frames, `ToTensor`, and the per-scale intrinsics.

* The pyramid reproduces PIL's `Image.resize(..., LANCZOS)` on 8-bit images BIT-EXACTLY: same support (3 x scale), same
  coefficient normalisation, same 22-bit fixed-point coefficients, horizontal pass then vertical pass with an 8-bit
  intermediate (Pillow `Resample.c`); the fixed-point dot products are evaluated as fp64 GEMMs, which are exact for these
  magnitudes (< 2^53).  tests/test_host_cpu.py compares against Pillow itself.
* ColorJitter is torchvision's PIL path (what the reference runs: PIL images through `transforms.ColorJitter`) restated
  on uint8 batches -- ImageEnhance blends, Pillow's RGB <-> HSV integer conversions, 8-bit quantisation after every
  operation, a fresh parameter draw for every frame and scale -- BIT-EXACT with Pillow (tests/test_host_cpu.py against
  a Pillow-based restatement kept with the test infrastructure).
* On a GPU the pipeline runs in HIP kernels (csrc/input_pipeline.hip through ops.lanczos_resize_u8 / ops.color_jitter_u8):
  the same integer / IEEE arithmetic on uint8, every byte of output equal.  The torch formulation below stays as the CPU
  path, as `backend="torch"` on a GPU, and as the comparison target of tests/test_input_pipeline_gpu.py.
* `_PyramidPipeline` is the one core of the four pipelines: the pyramid, the backend choice and, per backend, the way from
  the level-0 sources of every frame to the colour entries, with or without augmentation.  `DeviceInputPipeline` (KITTI),
  `DDADInputPipeline`, `CityscapesInputPipeline` and `CityscapesEvalPipeline` supply their level-0 sources, whether they
  augment and their intrinsics; the Cityscapes ones read the decoder's HWC frames in place (ops.lanczos_resize_view_u8).
* `DeviceInputPipeline(None, ...)` takes the frames of a batch at their own sizes (`RaggedFrames`, `pack_frames`,
  `RaggedLevel0`; ops.lanczos_resize_ragged_u8): what ppeadepth/datasets.py reads from a KITTI folder.
"""
import math

import numpy as np
import torch

KITTI_K = ((0.58, 0, 0.5, 0), (0, 1.92, 0.5, 0), (0, 0, 1, 0), (0, 0, 0, 1))      # kitti_dataset.py:26-29
PRECISION_BITS = 32 - 8 - 2                                                        # Pillow Resample.c


def _lanczos(x):
    def sinc(v):                                # Pillow Resample.c sinc_filter
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    if -3.0 <= x < 3.0:
        return sinc(x) * sinc(x / 3)
    return 0.0


def _bilinear(x):
    x = abs(x)                                  # Pillow Resample.c bilinear_filter
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bilinear": (_bilinear, 1.0)}      # Pillow's (filter, support)


def resample_matrix(insize, outsize, filter="lanczos"):
    """[outsize, insize] fp64 matrix of Pillow's fixed-point coefficients of an 8-bit resize (precompute_coeffs +
    normalize_coeffs_8bpc) with `filter` "lanczos" (support 3) or "bilinear" (the triangle 1 - |x|, support 1)."""
    if filter not in FILTERS:
        raise ValueError(f"filter {filter!r}: expected one of {sorted(FILTERS)}")
    kernel, support = FILTERS[filter]
    scale = insize / outsize
    filterscale = max(scale, 1.0)
    support = support * filterscale
    m = np.zeros((outsize, insize), dtype=np.float64)
    for xx in range(outsize):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), insize)
        ss = 1.0 / filterscale
        w = np.array([kernel((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)], dtype=np.float64)
        w /= w.sum()
        fixed = np.where(w < 0, np.trunc(-0.5 + w * (1 << PRECISION_BITS)), np.trunc(0.5 + w * (1 << PRECISION_BITS)))
        m[xx, xmin:xmax] = fixed
    return m


def lanczos_matrix(insize, outsize):
    """[outsize, insize] fp64 matrix of Pillow's fixed-point LANCZOS coefficients."""
    return resample_matrix(insize, outsize, "lanczos")


def compact_taps(matrix):
    """Dense [outsize, insize] coefficient matrix -> int32 [outsize, 2 + kmax]: per output (first input index, tap count n,
    the n coefficients, zero-padded to the longest row): the form the HIP kernels read (Pillow's own `bounds` / `kk`)."""
    out = []
    for row in np.asarray(matrix):
        nz = np.flatnonzero(row)
        out.append((int(nz[0]), row[nz[0]:nz[-1] + 1].astype(np.int64)))
    kmax = max(len(c) for _, c in out)
    table = np.zeros((len(out), 2 + kmax), dtype=np.int32)
    for i, (lo, c) in enumerate(out):
        table[i, 0], table[i, 1], table[i, 2:2 + len(c)] = lo, len(c), c
    return table


def dense_taps(table, insize):
    """Inverse of compact_taps: the dense [outsize, insize] fp64 matrix."""
    m = np.zeros((len(table), insize), dtype=np.float64)
    for i, row in enumerate(np.asarray(table)):
        m[i, row[0]:row[0] + row[1]] = row[2:2 + row[1]]
    return m


def identity_taps(size):
    """One tap of weight 1.0 per output: a pass that changes no byte (the flip-only first horizontal pass)."""
    return np.stack([np.arange(size), np.ones(size, np.int64), np.full(size, 1 << PRECISION_BITS)], 1).astype(np.int32)


class LanczosResize:
    """uint8 [.., Hin, Win] -> uint8 [.., Hout, Wout], bit-exact with PIL's LANCZOS resize of an 8-bit image (or, with
    filter="bilinear", its BILINEAR resize: the kernels read generic tap tables).
    backend "torch": fp64 GEMMs over the dense coefficient matrices; "hip": ops.lanczos_resize_u8 over the compact tables
    ([N,C,Hin,Win] input, or a list of such tensors; `flip` / `nonzero` as there; `first` = this is the pipeline's first
    level, whose horizontal pass always runs because it carries the flip and the blank-frame mark)."""

    def __init__(self, in_hw, out_hw, device, backend="torch", first=False, filter="lanczos"):
        self.in_hw, self.out_hw, self.backend = tuple(in_hw), tuple(out_hw), backend
        mh, mv = resample_matrix(in_hw[1], out_hw[1], filter), resample_matrix(in_hw[0], out_hw[0], filter)
        if backend == "hip":
            th = compact_taps(mh) if in_hw[1] != out_hw[1] else (identity_taps(in_hw[1]) if first else None)
            tv = compact_taps(mv) if in_hw[0] != out_hw[0] else None
            self.taps_h = None if th is None else torch.from_numpy(th).to(device)
            self.taps_v = None if tv is None else torch.from_numpy(tv).to(device)
            return
        self.mh = torch.from_numpy(mh).to(device)      # horizontal: [Wout, Win]
        self.mv = torch.from_numpy(mv).to(device)      # vertical:   [Hout, Hin]

    @staticmethod
    def _clip8(acc):
        return torch.floor((acc + float(1 << (PRECISION_BITS - 1))) / float(1 << PRECISION_BITS)).clamp_(0, 255)

    def __call__(self, img_u8, flip=None, nonzero=None):
        if self.backend == "hip":
            from ppeadepth import ops
            return ops.lanczos_resize_u8(img_u8, self.out_hw, self.taps_h, self.taps_v, flip, nonzero)
        return self._torch(img_u8)

    def views(self, views, flip=None, nonzero=None):
        """The same resize of uint8 [n,Hin,Win,C] HWC views (a list of them: as if concatenated) -> planar [N,C,Hout,Wout].
        "hip": ops.lanczos_resize_view_u8 reads the views through their strides (`first` pipelines only: the horizontal pass
        always runs); "torch": slice, permute, then the formulation above."""
        if self.backend == "hip":
            from ppeadepth import ops
            return ops.lanczos_resize_view_u8(views, self.out_hw, self.taps_h, self.taps_v, flip, nonzero)
        if flip is not None or nonzero is not None:
            raise ValueError("backend 'torch' flips and marks blank frames in the pipeline")
        views = list(views) if isinstance(views, (list, tuple)) else [views]
        return self._torch(torch.cat([v.permute(0, 3, 1, 2) for v in views]))

    def _torch(self, img_u8):
        x = img_u8.to(torch.float64)
        if self.in_hw[1] != self.out_hw[1]:
            x = self._clip8(x @ self.mh.t())                        # rows stay, columns resampled; 8-bit intermediate
        if self.in_hw[0] != self.out_hw[0]:
            x = self._clip8(self.mv @ x)
        return x.to(torch.uint8)


# ---- frames of different sizes: KITTI raw has one frame size per recording day, and a training batch mixes the days ----
MAX_RAGGED_BYTES = (1 << 31) - 1                # the descriptor's byte offsets are int32


def ragged_layout(hws):
    """[(H, W) or None per image] -> (desc int32 [N,4] = (byte offset, H, W, size class), sizes, total bytes): the images'
    HWC bytes back to back; None is an absent image, H = W = 0 (the reference's 100x100 zero dummy for a missing neighbour,
    mono_dataset.py:161-166); the size class is the index into `sizes`, the distinct (H, W) in order of first sight.
    Nothing is allocated; a total of 2^31 bytes or more is refused."""
    desc, sizes, total = np.zeros((len(hws), 4), np.int64), [], 0
    for n, hw in enumerate(hws):
        if hw is None:
            desc[n, 0] = total
            continue
        h, w = int(hw[0]), int(hw[1])
        if h <= 0 or w <= 0:
            raise ValueError(f"image {n}: size {(h, w)}")
        if (h, w) not in sizes:
            sizes.append((h, w))
        desc[n] = (total, h, w, sizes.index((h, w)))
        total += h * w * 3
        if total > MAX_RAGGED_BYTES:
            raise ValueError(f"the frames of one batch hold 2^31 bytes or more (image {n} ends at byte {total})")
    return torch.from_numpy(desc.astype(np.int32)), sizes, total


class RaggedFrames:
    """The raw frames of one batch, of any sizes, as the ragged level-0 pass reads them: `buf` ONE host byte buffer with
    the images' HWC bytes back to back, `desc` int32 [N,4] (`ragged_layout`; the size classes index `sizes`), image
    n = fi * batch + b (frame-major).  What a DataLoader's collate step hands over (`pack_frames`)."""

    def __init__(self, buf, desc, sizes, batch):
        self.buf, self.desc, self.sizes, self.batch = buf, desc, list(sizes), batch
        if desc.shape[0] % batch != 0:
            raise ValueError(f"{desc.shape[0]} images are no whole number of frames for a batch of {batch}")

    def __len__(self):
        return self.desc.shape[0]

    def pin_memory(self):                       # what DataLoader(pin_memory=True) calls on a custom batch
        self.buf = self.buf.pin_memory()
        return self

    def image(self, n):
        """Image n as a uint8 [H,W,3] view of the buffer, or None when it is absent."""
        off, h, w, _ = self.desc[n].tolist()
        return self.buf[off:off + h * w * 3].view(h, w, 3) if h else None


def pack_frames(raw, frame_idxs, pin=None):
    """raw = {frame id: list of B items}, an item a uint8 [H,W,3] array / tensor as an image decoder returns it, of any size,
    or None for a missing neighbour -> `RaggedFrames` in the order of frame_idxs.  The collate step of a DataLoader: host
    work only, so it can run in a worker (pin=False there; pin=None pins the buffer when a GPU is present, so that the one
    copy of the frame bytes to the device can be asynchronous)."""
    B = len(raw[frame_idxs[0]])
    items = []
    for f in frame_idxs:
        if len(raw[f]) != B:
            raise ValueError(f"frame {f}: {len(raw[f])} items in a batch of {B}")
        items += list(raw[f])
    for n, it in enumerate(items):
        if it is not None and (len(it.shape) != 3 or it.shape[2] != 3 or str(it.dtype).split(".")[-1] != "uint8"):
            raise ValueError(f"image {n}: expected uint8 [H,W,3], got {it.dtype} {tuple(it.shape)}")
    desc, sizes, total = ragged_layout([None if it is None else it.shape[:2] for it in items])
    pin = torch.cuda.is_available() if pin is None else pin
    buf = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=bool(pin))
    for it, (off, h, w, _) in zip(items, desc.tolist()):
        if it is not None:
            t = it if torch.is_tensor(it) else torch.from_numpy(np.ascontiguousarray(it))
            buf[off:off + h * w * 3].view(h, w, 3).copy_(t)
    return RaggedFrames(buf, desc, sizes, B)


class RaggedLevel0:
    """Level 0 of a pipeline whose frames differ in size.  Size classes are keyed by (H, W) and kept for the pipeline's
    life: a class's tables are built on first sight (`resample_matrix` / `compact_taps`; `identity_taps` where a size stays:
    both passes of the ragged level always run), and on the "hip" backend the device tables [K][out][2 + kmax] are rebuilt
    and uploaded only then, so a steady-state call uploads no table (`table_uploads`, `table_builds` count them)."""

    def __init__(self, out_hw, device, backend):
        self.out_hw, self.device, self.backend = tuple(out_hw), device, backend
        self.classes, self.host = {}, []        # (H, W) -> k; per class what its backend needs
        self.taps_h = self.taps_v = None
        self.table_builds = self.table_uploads = 0

    def class_of(self, hw):
        k = self.classes.get(hw)
        if k is None:
            k = self.classes[hw] = len(self.host)
            (h, w), (ho, wo) = hw, self.out_hw
            if self.backend == "hip":
                self.host.append((compact_taps(resample_matrix(w, wo)) if w != wo else identity_taps(w),
                                  compact_taps(resample_matrix(h, ho)) if h != ho else identity_taps(h)))
                self.taps_h = None
            else:
                self.host.append(LanczosResize(hw, self.out_hw, self.device, "torch"))
            self.table_builds += 1
        return k

    def describe(self, frames):
        """-> the frames' descriptor with THIS pipeline's size classes (host int32 [N,4])."""
        desc = frames.desc.clone()
        if frames.sizes:
            mine = torch.tensor([self.class_of(tuple(hw)) for hw in frames.sizes], dtype=torch.int32)
            desc[:, 3] = torch.where(desc[:, 1] > 0, mine[desc[:, 3].long()], torch.zeros_like(desc[:, 3]))
        return desc

    def tables(self):
        """The device tables of all classes seen so far; at least one class (an all-absent batch reads none of it)."""
        if not self.host:
            self.class_of(self.out_hw)
        if self.taps_h is None:
            both = []
            for i in range(2):
                kmax = max(t[i].shape[1] for t in self.host)
                both.append(np.stack([np.pad(t[i], ((0, 0), (0, kmax - t[i].shape[1]))) for t in self.host]))
            self.taps_h, self.taps_v = (torch.from_numpy(t).to(self.device) for t in both)
            self.table_uploads += 1
        return self.taps_h, self.taps_v

    def run_hip(self, frames, desc, words, flip, nonzero):
        from ppeadepth import ops
        taps_h, taps_v = self.tables()
        buf = frames.buf.to(self.device, non_blocking=True)         # the call's one copy of frame bytes
        return ops.lanczos_resize_ragged_u8(buf, (desc, words), self.out_hw, taps_h, taps_v, flip, nonzero)

    def run_torch(self, frames, fi, do_flip):
        """Frame fi of every item -> (uint8 [B,3,Hout,Wout], blank [B]): per item the `LanczosResize` of its class on the
        (flipped) frame; an absent frame is zeros; blank = absent, or no non-zero byte."""
        B, out, blank = frames.batch, [], []
        for b in range(B):
            img = frames.image(fi * B + b)
            blank.append(img is None or not bool(img.any()))
            if img is None:
                out.append(torch.zeros((3,) + self.out_hw, dtype=torch.uint8, device=self.device))
                continue
            img = img.to(self.device).permute(2, 0, 1)
            img = img.flip(-1) if bool(do_flip[b]) else img
            out.append(self.host[self.class_of(tuple(img.shape[1:]))]._torch(img))
        return torch.stack(out), torch.tensor(blank, device=self.device)


# ---- ColorJitter: torchvision's PIL path, bit for bit, on uint8 batches -------------------------------------------------
# The reference jitters PIL images (mono_dataset.py:183-190 -> torchvision functional_pil -> Pillow), i.e. 8-bit images
# with a quantisation after every operation.  Each operation below is Pillow's arithmetic restated on tensors (fp32 / fp64
# exactly where the C code uses float / double), verified bit-exact against Pillow itself (tests/test_host_cpu.py):
#   ImagingBlend (ImageEnhance):  out = clip(trunc(deg + f * (img - deg)))           in fp32
#   RGB -> L:                     (19595 R + 38470 G + 7471 B + 0x8000) >> 16
#   contrast's degenerate image:  int(mean(L) + 0.5);  saturation's: L replicated;  brightness's: zeros
#   hue: Convert.c rgb2hsv / hsv2rgb (8-bit H, S, V) around  H += uint8(h * 255)
def _gray_u8(img):
    """int64 [B,3,H,W] -> [B,1,H,W] (Pillow's RGB -> L)."""
    return ((img[:, 0] * 19595 + img[:, 1] * 38470 + img[:, 2] * 7471 + 0x8000) >> 16).unsqueeze(1)


def _blend_u8(deg, img, f):
    """PIL.Image.blend(degenerate, image, factor) for 8-bit images; f [B]."""
    f = f.to(torch.float32).reshape(-1, 1, 1, 1)
    d, x = deg.to(torch.float32), img.to(torch.float32)
    t = d + f * (x - d)                                       # fp32, one rounding per operation as in C
    return torch.trunc(t).clamp_(0, 255).to(torch.int64)


def adjust_brightness(img, f):
    return _blend_u8(torch.zeros_like(img), img, f)


def adjust_contrast(img, f):
    g = _gray_u8(img)
    mean = torch.floor(g.to(torch.float64).mean((1, 2, 3)) + 0.5).to(torch.int64).reshape(-1, 1, 1, 1)
    return _blend_u8(mean.expand_as(img), img, f)


def adjust_saturation(img, f):
    return _blend_u8(_gray_u8(img).expand_as(img), img, f)


def _rgb2hsv_u8(img):
    r, g, b = img.unbind(1)
    maxc, minc = img.amax(1), img.amin(1)
    eq = maxc == minc
    f32, f64 = torch.float32, torch.float64
    cr = (maxc - minc).to(f32)
    crs = torch.where(eq, torch.ones_like(cr), cr)
    s = cr / torch.where(eq, torch.ones_like(maxc), maxc).to(f32)
    rc, gc, bc = (maxc - r).to(f32) / crs, (maxc - g).to(f32) / crs, (maxc - b).to(f32) / crs
    h = torch.where(r == maxc, bc - gc,
                    torch.where(g == maxc, (2.0 + rc.to(f64) - bc.to(f64)).to(f32), (4.0 + gc.to(f64) - rc.to(f64)).to(f32)))
    h = torch.fmod(h.to(f64) / 6.0 + 1.0, 1.0).to(f32)
    uh = (h.to(f64) * 255.0).to(torch.int64).clamp_(0, 255)
    us = (s.to(f64) * 255.0).to(torch.int64).clamp_(0, 255)
    zero = torch.zeros_like(uh)
    return torch.where(eq, zero, uh), torch.where(eq, zero, us), maxc


def _hsv2rgb_u8(h, s, v):
    f32, f64 = torch.float32, torch.float64
    hf = h.to(f32).to(f64) * 6.0 / 255.0
    i = torch.floor(hf)
    f = (hf - i).to(f32).to(f64)
    fs = (s.to(f32).to(f64) / 255.0).to(f32).to(f64)
    vv = v.to(f32).to(f64)

    def rnd(x):                                                # C round(): positive values, half away from zero
        return torch.floor(x + 0.5).clamp_(0, 255).to(torch.int64)
    p, q, t = rnd(vv * (1.0 - fs)), rnd(vv * (1.0 - fs * f)), rnd(vv * (1.0 - fs * (1.0 - f)))
    sel = i.to(torch.int64) % 6
    pick = lambda opts: torch.stack(opts, 0).gather(0, sel.unsqueeze(0))[0]      # noqa: E731
    r, g, b = pick([v, q, p, p, t, v]), pick([t, v, v, q, p, p]), pick([p, p, t, v, v, q])
    gray = s == 0
    return torch.stack([torch.where(gray, v, r), torch.where(gray, v, g), torch.where(gray, v, b)], 1)


def adjust_hue(img, hue):
    """hue [B] in [-0.5, 0.5]: H (8 bit) += uint8(hue * 255), wrapping (torchvision functional_pil.adjust_hue)."""
    h, s, v = _rgb2hsv_u8(img)
    shift = torch.trunc(hue.to(torch.float64) * 255.0).to(torch.int64) & 255
    return _hsv2rgb_u8((h + shift.to(h.device).reshape(-1, 1, 1)) & 255, s, v)


def draw_jitter_params(batch, generator=None, brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.8, 1.2),
                       hue=(-0.1, 0.1)):
    """One `ColorJitter.get_params` draw per item (torchvision order: randperm(4), then brightness, contrast, saturation,
    hue), as the reference's transform object draws on EVERY call (mono_dataset.py:183-185 builds
    `transforms.ColorJitter(...)`, whose forward re-draws: each frame and scale of an item gets its own parameters)."""
    order, fac = [], {k: [] for k in ("brightness", "contrast", "saturation", "hue")}
    rng = {"brightness": brightness, "contrast": contrast, "saturation": saturation, "hue": hue}
    for _ in range(batch):
        order.append(torch.randperm(4, generator=generator))
        for k in ("brightness", "contrast", "saturation", "hue"):
            fac[k].append(torch.empty(1).uniform_(rng[k][0], rng[k][1], generator=generator))
    out = {k: torch.cat(v) for k, v in fac.items()}
    out["order"] = torch.stack(order)
    return out


def color_jitter(img_u8, params, apply):
    """img_u8 uint8 [B,3,H,W] -> uint8; params from draw_jitter_params; apply [B] bool (mono_dataset.py:143: p = 0.5 per
    item; blank frames are never jittered, :107-110).  Per item the four operations run in the item's own order."""
    dev = img_u8.device
    fac = {k: params[k].to(dev) for k in ("brightness", "contrast", "saturation", "hue")}
    order_host = params["order"].cpu()                 # which operations are due at a step is decided on the host
    order = order_host.to(dev)
    ops = (lambda x: adjust_brightness(x, fac["brightness"]), lambda x: adjust_contrast(x, fac["contrast"]),
           lambda x: adjust_saturation(x, fac["saturation"]), lambda x: adjust_hue(x, fac["hue"]))
    img = img_u8.to(torch.int64)
    out = img
    for step in range(4):                      # per-item operation order: evaluate each op, select where it is due
        nxt = out
        for j, op in enumerate(ops):
            if bool((order_host[:, step] == j).any()):            # no device sync
                due = (order[:, step] == j).reshape(-1, 1, 1, 1)
                nxt = torch.where(due, op(out), nxt)
        out = nxt
    return torch.where(apply.to(dev).reshape(-1, 1, 1, 1), out, img).to(torch.uint8)


def pack_jitter_params(params, apply):
    """Host side of ops.color_jitter_u8: `draw_jitter_params` dicts (one, or a list that is concatenated along the items)
    and apply [items] bool -> int32 [items, 10]: order[4], brightness / contrast / saturation as fp32 bit patterns,
    trunc(hue * 255) & 255, apply, one unused word."""
    ps = list(params) if isinstance(params, (list, tuple)) else [params]
    cat = lambda k: torch.cat([p[k].cpu() for p in ps])       # noqa: E731
    order = cat("order").to(torch.int32)
    fac = torch.stack([cat("brightness"), cat("contrast"), cat("saturation")], 1).to(torch.float32).contiguous()
    shift = torch.trunc(cat("hue").to(torch.float64) * 255.0).to(torch.int64) & 255
    tail = torch.stack([shift, apply.cpu().to(torch.int64), torch.zeros_like(shift)], 1).to(torch.int32)
    return torch.cat([order, fac.view(torch.int32), tail], 1)


def _jitter_of(jitter, f, s, B, generator):
    """The parameters of frame f at scale s.  `jitter`: one `draw_jitter_params` dict for the whole call (tests), or
    {(frame, scale): dict}, or None: a fresh draw, like the reference's transform object on every call.  Both backends ask
    in the same order (frame outer, scale inner), which is the order of the draws."""
    if jitter is None:
        return draw_jitter_params(B, generator)
    return jitter[(f, s)] if (f, s) in jitter else jitter


def _backend_of(device, backend):
    backend = backend or ("hip" if device.type == "cuda" else "torch")
    if backend not in ("hip", "torch"):
        raise ValueError(f"backend {backend!r}: expected 'hip' or 'torch'")
    if backend == "hip" and device.type != "cuda":
        raise ValueError("backend 'hip' needs a GPU device; the CPU path is backend 'torch'")
    return backend


def _k4_and_pinv(k3, scale_rows):
    """3x3 camera matrix -> (K, inv_K): the float32 4x4 with rows 0 and 1 scaled in place by `scale_rows(row0, row1)`, and
    `np.linalg.pinv` of that float32 matrix, in numpy on the host as the loaders do (a float32 SVD is not reproducible bit
    for bit in a kernel)."""
    K = np.zeros((4, 4), np.float32)
    K[:3, :3] = k3
    K[3][3] = 1
    scale_rows(K[0, :], K[1, :])
    return K, np.linalg.pinv(K)


def _camera_matrices(cameras, what):
    cam = cameras.cpu().numpy() if torch.is_tensor(cameras) else np.asarray(cameras)
    if cam.ndim != 3 or cam.shape[1:] != (3, 3):
        raise ValueError(f"{what}: [B,3,3] camera matrices, got {cam.shape}")
    return cam


def _put_intrinsics(inputs, KK):
    """[S,2,B,4,4] -> the ("K", s) and ("inv_K", s) entries."""
    for s in range(KK.shape[0]):
        inputs[("K", s)] = KK[s, 0]
        inputs[("inv_K", s)] = KK[s, 1]
    return inputs


class _PyramidPipeline:
    """What the four pipelines share: the pyramid of `LanczosResize` levels (level 0 from `src_hw` with `level0_filter`,
    level s >= 1 LANCZOS from level s-1), ToTensor's divisor, the backend, and per backend one method from the level-0
    sources of every frame to the ("color" | "color_aug", f, s) entries.  A subclass supplies its level-0 sources (dense
    planar frames, or with `hwc` uint8 [B,H,W,3] views that are read in place), whether it augments, and its intrinsics.

    A "hip" call launches, whatever the batch size: per level the horizontal and the vertical resize pass and the two
    ColorJitter launches, all frames stacked frame-major (image n = fi * B + b): 4 kernels per level, 16 for the 4 levels;
    one memset (the blank-frame marks) or, without augmentation, one fill (the all-zero parameter table); and ONE
    host-to-device copy: flip flags, the jitter parameters of every frame and scale and the subclass's per-sample
    intrinsics in one buffer.  Nothing is copied back to the host."""

    def __init__(self, src_hw, height, width, device, num_scales, frame_idxs, backend, level0_filter="lanczos", hwc=False):
        self.device = torch.device(device)
        self.backend = _backend_of(self.device, backend)
        self.height, self.width, self.num_scales, self.frame_idxs, self.hwc = height, width, num_scales, tuple(frame_idxs), hwc
        # src_hw None: the frames differ in size, level 0 is `RaggedLevel0` and the level-0 source a `RaggedFrames`
        self.ragged = RaggedLevel0((height, width), self.device, self.backend) if src_hw is None else None
        self.resize, prev = [], None if src_hw is None else tuple(src_hw)
        for s in range(num_scales):
            hw = (height // 2 ** s, width // 2 ** s)
            self.resize.append(None if prev is None else LanczosResize(prev, hw, self.device, self.backend, first=(s == 0),
                                                                       filter=level0_filter if s == 0 else "lanczos"))
            prev = hw
        # ToTensor's divisor as a tensor: a true division on every device (the GPU folds a Python scalar into a multiplication
        # by its reciprocal, which is not the same fp32 value for 126 of the 256 levels)
        self.unit = torch.full((), 255.0, device=self.device)

    def _draw_flags(self, B, do_color_aug, do_flip, generator):
        if do_color_aug is None:
            do_color_aug = (torch.rand(B, generator=generator) > 0.5) if self.is_train else torch.zeros(B, dtype=torch.bool)
        if do_flip is None:
            do_flip = (torch.rand(B, generator=generator) > 0.5) if self.is_train else torch.zeros(B, dtype=torch.bool)
        return do_color_aug, do_flip

    def _colors(self, level0, B, aug=None, kk=None):
        """level0: the level-0 source of every frame, in the order of frame_idxs.  aug: None (nothing is flipped, jittered or
        marked blank: color_aug holds the bytes of color) or (do_color_aug, do_flip, jitter, generator).  kk: host float32
        array of intrinsics, or None.  -> (the colour entries, kk on the device)."""
        return (self._colors_hip if self.backend == "hip" else self._colors_torch)(level0, B, aug, kk)

    def _colors_torch(self, level0, B, aug, kk):
        inputs = {}
        for fi, f in enumerate(self.frame_idxs):
            if self.ragged is not None:
                do_color_aug, do_flip, jitter, generator = aug
                img, blank = self.ragged.run_torch(level0, fi, do_flip)          # level 0, flipped, per item
            else:
                img = level0[fi].to(self.device)
                img = img.permute(0, 3, 1, 2) if self.hwc else img
                if aug is not None:
                    do_color_aug, do_flip, jitter, generator = aug
                    img = torch.where(do_flip.to(self.device).reshape(-1, 1, 1, 1), img.flip(-1), img)
                    blank = (img.reshape(B, -1).sum(1) == 0)
            for s in range(self.num_scales):
                if s or self.ragged is None:
                    img = self.resize[s](img)                           # uint8, chained from the previous scale
                color = inputs[("color", f, s)] = img.to(torch.float32) / self.unit      # ToTensor
                if aug is None:
                    inputs[("color_aug", f, s)] = color.clone()
                    continue
                prm = _jitter_of(jitter, f, s, B, generator)
                jit = color_jitter(img, prm, do_color_aug.to(self.device) & ~blank)
                inputs[("color_aug", f, s)] = jit.to(torch.float32) / self.unit
        return inputs, None if kk is None else torch.from_numpy(kk).to(self.device)

    def _colors_hip(self, level0, B, aug, kk):
        from ppeadepth import ops
        F, S = len(self.frame_idxs), self.num_scales
        N = F * B                                                   # all frames stacked, frame-major: image n = fi * B + b
        host, words = [], 0
        if aug is not None:
            do_color_aug, do_flip, jitter, generator = aug
            # parameters in the torch path's order (frame outer, scale inner), then one table for the whole call
            prms = [_jitter_of(jitter, f, s, B, generator) for f in self.frame_idxs for s in range(S)]
            by_scale = [prms[fi * S + s] for s in range(S) for fi in range(F)]
            for t in [do_color_aug, do_flip] + [v for p in prms for v in p.values()]:
                if t.device.type != "cpu":             # a device tensor would cost a device-to-host copy inside the call
                    raise ValueError("backend 'hip' takes do_color_aug, do_flip and the jitter parameters as host tensors")
            table = pack_jitter_params(by_scale, do_color_aug.repeat(S * F))                  # [S * N, 10]
            host, words = [do_flip.to(torch.int32).repeat(F), table.reshape(-1)], N + table.numel()
        desc, ragged_words = None, 0
        if self.ragged is not None:                                 # the frames' descriptor and row prefix ride along
            desc = self.ragged.describe(level0)
            host.append(torch.cat([desc.reshape(-1), ops.ragged_row_prefix(desc)]))
            ragged_words = host[-1].numel()
        if kk is not None:
            host.append(torch.from_numpy(kk).view(torch.int32).reshape(-1))
        dev = torch.cat(host).to(self.device)                       # the call's one host-to-device copy of parameters
        if aug is None:
            # no jitter: an all-zero parameter table (apply = 0, written on the device) turns the ColorJitter launch into the
            # uint8 -> fp32 conversion of both outputs
            flip = nonzero = None
            params = [torch.zeros(N, ops.JITTER_PARAM_WORDS, device=self.device, dtype=torch.int32)] * S
        else:
            flip, params = dev[:N], dev[N:words].view(S, N, -1)
            nonzero = torch.empty(N, device=self.device, dtype=torch.int32)      # 0: a blank (missing) frame, never jittered
        if self.ragged is None:
            level0 = [v.to(self.device) for v in level0]
        levels = []
        for s in range(S):
            if s > 0:
                img = self.resize[s](img)
            elif self.ragged is not None:
                img = self.ragged.run_hip(level0, desc, dev[words:words + ragged_words], flip, nonzero)
            elif self.hwc:
                img = self.resize[0].views(level0, flip, nonzero)
            else:
                img = self.resize[0]([v.contiguous() for v in level0], flip, nonzero)
            levels.append(ops.color_jitter_u8(img, params[s], nonzero))
        inputs = {}
        for fi, f in enumerate(self.frame_idxs):                   # the torch arm's key order
            for s, (color, jit) in enumerate(levels):
                inputs[("color", f, s)] = color[fi * B:(fi + 1) * B]
                inputs[("color_aug", f, s)] = jit[fi * B:(fi + 1) * B]
        return inputs, None if kk is None else dev[words + ragged_words:].view(torch.float32).view(kk.shape)


class DeviceInputPipeline(_PyramidPipeline):
    """The KITTI loader's image path.  backend "hip" (the default on a GPU device; refused on the CPU) runs the whole call
    in HIP kernels, "torch" (the default on the CPU) in the torch formulation above; both return the same bytes.

    A "hip" call is the core's 16 kernels, memset and copy (flip flags and jitter parameters) plus one launch that repeats
    K / inv_K over the batch: 17 kernels.

    raw_hw: the one size of all raw frames, or None: every frame has its own size (KITTI raw has one per recording day, and
    a shuffled batch mixes them) and comes as a decoder returns it (HWC), `None` for a missing neighbour.  Level 0 is then
    the ragged launch pair (`RaggedLevel0`, ops.lanczos_resize_ragged_u8) on all frames at once, whatever the number of
    sizes: still 17 kernels; the frames' descriptor rides in the parameter copy and the frame bytes are one more copy.
    Everything after level 0 is the same code."""

    def __init__(self, raw_hw, height, width, device, num_scales=4, frame_idxs=(0, -1, 1), K=KITTI_K, is_train=True,
                 backend=None):
        super().__init__(raw_hw, height, width, device, num_scales, frame_idxs, backend)
        self.is_train = is_train
        self.K, self.inv_K = [], []
        for s in range(num_scales):                        # mono_dataset.py:173-182
            k = np.array(K, dtype=np.float32)
            k[0, :] *= width // (2 ** s)
            k[1, :] *= height // (2 ** s)
            self.K.append(torch.from_numpy(k).to(self.device))
            self.inv_K.append(torch.from_numpy(np.linalg.pinv(k)).to(self.device))
        self.K_rows = torch.stack([torch.stack(p) for p in zip(self.K, self.inv_K)])      # [scales, 2, 4, 4]

    @torch.no_grad()
    def __call__(self, raw, do_color_aug=None, do_flip=None, jitter=None, generator=None):
        """raw: {frame id: uint8 [B,3,Hraw,Wraw]} (a missing neighbour = all zeros, mono_dataset.py:160-164).
        With raw_hw=None: {frame id: list of B items}, an item a uint8 [H,W,3] array / tensor of any size or None for a
        missing neighbour, or those already packed (`pack_frames`, datasets.collate_raw: a `RaggedFrames`).
        do_color_aug / do_flip: [B] bool (default: drawn with p = 0.5 each when is_train, mono_dataset.py:143-144).
        backend "hip": these flags and the jitter parameters are host tensors (as draw_jitter_params returns them); they go
        to the device in one table, and a device tensor is refused rather than copied back."""
        if self.ragged is not None:
            frames = raw if isinstance(raw, RaggedFrames) else pack_frames(raw, self.frame_idxs, pin=self.backend == "hip")
            if len(frames) != len(self.frame_idxs) * frames.batch:
                raise ValueError(f"{len(frames)} images for {len(self.frame_idxs)} frames of {frames.batch} items")
            B, level0 = frames.batch, frames
        else:
            B, level0 = raw[self.frame_idxs[0]].shape[0], [raw[f] for f in self.frame_idxs]
        do_color_aug, do_flip = self._draw_flags(B, do_color_aug, do_flip, generator)
        inputs, _ = self._colors(level0, B, (do_color_aug, do_flip, jitter, generator))
        if self.backend == "hip":
            from ppeadepth import ops
            KK = ops.repeat_rows(self.K_rows.view(-1, 4, 4), B).view(self.num_scales, 2, B, 4, 4)      # one launch
        else:
            KK = self.K_rows[:, :, None].repeat(1, 1, B, 1, 1)
        return _put_intrinsics(inputs, KK)


DDAD_RAW_HW = (1216, 1936)                      # ddad_dataset.py:137-138


class DDADInputPipeline(_PyramidPipeline):
    """The DDAD loader's image path (datasets/ddad_dataset.py:116-167) for a whole batch: raw uint8 frames 0 and -1 and the
    per-sample intrinsics -> the row-P dictionary.  Not the KITTI pipeline with other sizes:
      * level 0 is Pillow's BILINEAR resize of the raw frame (:121); the loader's LANCZOS resize to that same size (:77) is
        Pillow's copy; level s >= 1 is LANCZOS from level s-1;
      * no ColorJitter (`do_color_aug = False`, :124): color_aug holds the bytes of color; `do_flip` is drawn and never
        applied, so nothing is flipped;
      * ("K", s) / ("inv_K", s) are per sample and the SAME matrix at every scale (:132-143): rows 0 and 1 of the 4x4
        float32 matrix times width / raw width and height / raw height, the inverse `np.linalg.pinv` of that float32 matrix.
        These B small matrices are computed on the host with numpy, exactly as the loader does, and are the call's one
        host-to-device copy.
    backend "hip": the core's 16 kernels, fill and copy plus one launch that repeats the intrinsics over the scales;
    "torch": the formulation above.  Both return the same bytes."""

    def __init__(self, device, height=384, width=640, raw_hw=DDAD_RAW_HW, num_scales=4, frame_idxs=(0, -1), backend=None):
        super().__init__(raw_hw, height, width, device, num_scales, frame_idxs, backend, level0_filter="bilinear")
        self.raw_hw = tuple(raw_hw)

    def intrinsics(self, intrinsics):
        """[B,3,3] camera matrices -> float32 [2,B,4,4]: K and inv_K of ddad_dataset.py:132-143, in numpy on the host."""
        intr = _camera_matrices(intrinsics, "intrinsics")

        def scale(row0, row1):
            row0 *= self.width / self.raw_hw[1]
            row1 *= self.height / self.raw_hw[0]
        out = np.zeros((2, len(intr), 4, 4), np.float32)
        for b in range(len(intr)):
            out[0, b], out[1, b] = _k4_and_pinv(intr[b], scale)
        return out

    @torch.no_grad()
    def __call__(self, raw, intrinsics):
        """raw: {frame id: uint8 [B,3,Hraw,Wraw]}; intrinsics: [B,3,3] (host tensor or array)."""
        B, S = raw[self.frame_idxs[0]].shape[0], self.num_scales
        for f in self.frame_idxs:
            if tuple(raw[f].shape) != (B, 3) + self.raw_hw or raw[f].dtype != torch.uint8:
                raise ValueError(f"frame {f}: expected uint8 {(B, 3) + self.raw_hw}, got {raw[f].dtype} {tuple(raw[f].shape)}")
        kk = self.intrinsics(intrinsics)
        if kk.shape[1] != B:
            raise ValueError(f"{kk.shape[1]} camera matrices for a batch of {B}")
        inputs, kk = self._colors([raw[f] for f in self.frame_idxs], B, kk=kk)
        if self.backend == "hip":
            from ppeadepth import ops
            KK = ops.repeat_rows(kk.reshape(1, -1), S).reshape(S, 2, B, 4, 4)
        else:
            KK = kk[None].repeat(S, 1, 1, 1, 1)
        return _put_intrinsics(inputs, KK)


# ---- Cityscapes: the training triplets and the evaluation frames, read as views ---------------------------------------
CITYSCAPES_TRIPLET_HW = (384, 1024)             # cityscapes_preprocessed_dataset.py:18-19, one frame of the wide image
CITYSCAPES_RAW_HW = (1024, 2048)                # cityscapes_evaldataset.py:19-20


def read_cityscapes_cam_txt(path):
    """`<frame>_cam.txt` of the preprocessed triplets (cityscapes_preprocessed_dataset.py:40-45): nine comma-separated
    values, fx = v[0], u0 = v[2], fy = v[4], v0 = v[5] -> float64 [3,3]."""
    v = np.loadtxt(path, delimiter=",").reshape(-1)
    return np.array([[v[0], 0, v[2]], [0, v[4], v[5]], [0, 0, 1]], dtype=np.float64)


def read_cityscapes_camera_json(path):
    """`<frame>_camera.json` of the raw dataset (cityscapes_evaldataset.py:45-50) -> float64 [3,3]."""
    import json
    with open(path, "r") as f:
        c = json.load(f)["intrinsic"]
    return np.array([[c["fx"], 0, c["u0"]], [0, c["fy"], c["v0"]], [0, 0, 1]], dtype=np.float64)


def cityscapes_intrinsics(cameras, raw_width, raw_height, width, height, num_scales):
    """[B,3,3] camera matrices -> float32 [scales,2,B,4,4]: ("K", s) and ("inv_K", s) of the two Cityscapes loaders, per
    sample AND per level: the float32 4x4 of fx, fy, u0, v0 with row 0 / raw_width and row 1 / raw_height (`load_intrinsics`;
    the evaluation loader passes the Python float 1024 * 0.75), then rows 0 and 1 times width // 2**s and height // 2**s
    (mono_dataset.py:173-182), the inverse `np.linalg.pinv` of that float32 matrix.  In numpy on the host, in the loader's
    operations and order."""
    cam = _camera_matrices(cameras, "cameras")
    out = np.zeros((num_scales, 2, len(cam), 4, 4), np.float32)
    for b, c in enumerate(cam):
        for s in range(num_scales):
            def scale(row0, row1):
                row0 /= raw_width
                row1 /= raw_height
                row0 *= width // (2 ** s)
                row1 *= height // (2 ** s)
            out[s, 0, b], out[s, 1, b] = _k4_and_pinv([[c[0, 0], 0, c[0, 2]], [0, c[1, 1], c[1, 2]], [0, 0, 1]], scale)
    return out


class CityscapesInputPipeline(_PyramidPipeline):
    """The preprocessed-Cityscapes loader (datasets/cityscapes_preprocessed_dataset.py through MonoDataset) for a whole
    batch: one wide image per item that holds frames -1, 0, +1 side by side, uint8 [B, Hraw, 3 * Wraw, 3] as the JPEG
    decoder returns it (HWC), and the item's camera -> the row-P dictionary.
      * frame -1 is columns [0, w), frame 0 [w, 2w), frame +1 [2w, 3w) (:62-66); the flip mirrors each third on its own;
      * pyramid, ColorJitter (same draw order), blank-frame rule and ToTensor are `DeviceInputPipeline`'s, by the core's code;
      * ("K", s) / ("inv_K", s) are per sample and per level (`cityscapes_intrinsics`), uploaded with the call's one
        parameter copy.
    backend "hip": the first horizontal pass reads the three windows in place (ops.lanczos_resize_view_u8: no third is
    sliced out, permuted or copied); 16 kernels, one memset and one host-to-device copy, whatever the batch size.
    backend "torch": slices and permutes, then the torch formulation.  Both return the same bytes."""

    def __init__(self, device, height=192, width=512, raw_hw=CITYSCAPES_TRIPLET_HW, num_scales=4, frame_idxs=(0, -1, 1),
                 is_train=True, backend=None):
        if any(f not in (-1, 0, 1) for f in frame_idxs):
            raise ValueError(f"frame_idxs {tuple(frame_idxs)}: the wide image holds frames -1, 0 and 1")
        super().__init__(raw_hw, height, width, device, num_scales, frame_idxs, backend, hwc=True)
        self.raw_hw, self.is_train = tuple(raw_hw), is_train

    @torch.no_grad()
    def __call__(self, triplets, cameras, do_color_aug=None, do_flip=None, jitter=None, generator=None):
        """triplets: uint8 [B, Hraw, 3 * Wraw, 3]; cameras: [B,3,3] (host tensor or array); the rest as
        `DeviceInputPipeline`'s."""
        Hraw, Wraw = self.raw_hw
        if triplets.dim() != 4 or tuple(triplets.shape[1:]) != (Hraw, 3 * Wraw, 3) or triplets.dtype != torch.uint8:
            raise ValueError(f"expected uint8 [B, {Hraw}, {3 * Wraw}, 3] (three frames side by side, HWC), got "
                             f"{triplets.dtype} {tuple(triplets.shape)}")
        B = triplets.shape[0]
        kk = cityscapes_intrinsics(cameras, Wraw, Hraw, self.width, self.height, self.num_scales)
        if kk.shape[2] != B:
            raise ValueError(f"{kk.shape[2]} camera matrices for a batch of {B}")
        do_color_aug, do_flip = self._draw_flags(B, do_color_aug, do_flip, generator)
        triplets = triplets.to(self.device)
        thirds = [triplets[:, :, (f + 1) * Wraw:(f + 2) * Wraw] for f in self.frame_idxs]
        return _put_intrinsics(*self._colors(thirds, B, (do_color_aug, do_flip, jitter, generator), kk))


class CityscapesEvalPipeline(_PyramidPipeline):
    """The Cityscapes evaluation loader (datasets/cityscapes_evaldataset.py through MonoDataset) for a whole batch: the raw
    frames 0 and -1, uint8 [B, Hraw, Wraw, 3] (HWC), and the item's camera -> the row-P dictionary.
      * the frame is cropped to its top Hraw * 3 // 4 rows (:66-68) before the resize: in HWC a prefix of each image, so
        nothing is copied;
      * LANCZOS pyramid, level s from level s-1; no flip, no jitter: color_aug holds the bytes of color;
      * K row 1 is divided by Hraw * 0.75, the Python float of :56, not by the integer crop height.
    Backends as `CityscapesInputPipeline`; "hip" is the two resize passes and the two jitter launches per level, a fill
    of the parameter table and one host-to-device copy (the intrinsics)."""

    def __init__(self, device, height=192, width=512, raw_hw=CITYSCAPES_RAW_HW, num_scales=4, frame_idxs=(0, -1),
                 backend=None):
        self.raw_hw = tuple(raw_hw)
        self.crop_h = self.raw_hw[0] * 3 // 4
        super().__init__((self.crop_h, self.raw_hw[1]), height, width, device, num_scales, frame_idxs, backend, hwc=True)

    @torch.no_grad()
    def __call__(self, raw, cameras):
        """raw: {frame id: uint8 [B,Hraw,Wraw,3]}; cameras: [B,3,3] (host tensor or array)."""
        B = raw[self.frame_idxs[0]].shape[0]
        for f in self.frame_idxs:
            if tuple(raw[f].shape) != (B,) + self.raw_hw + (3,) or raw[f].dtype != torch.uint8:
                raise ValueError(f"frame {f}: expected uint8 {(B,) + self.raw_hw + (3,)}, got {raw[f].dtype} "
                                 f"{tuple(raw[f].shape)}")
        kk = cityscapes_intrinsics(cameras, self.raw_hw[1], self.raw_hw[0] * 0.75, self.width, self.height, self.num_scales)
        if kk.shape[2] != B:
            raise ValueError(f"{kk.shape[2]} camera matrices for a batch of {B}")
        top = [raw[f].to(self.device)[:, :self.crop_h] for f in self.frame_idxs]
        return _put_intrinsics(*self._colors(top, B, kk=kk))

