"""Shared by tests/test_export_cpu.py and tests/test_export_gpu.py: seeded synthetic planes and the float64 restatement of
the prediction export (resize as `_resize_f64` of tests/test_eval_device_gpu.py, then the formulas in float64)."""
import numpy as np
import torch

RTOL = 1e-5                                   # tests/test_eval_device_gpu.py:16
SRC = (24, 80)
RAGGED = [(47, 157), (24, 80), (12, 41)]      # a non-integer enlargement, the identity, a reduction; 3 * 157, 3 * 41 odd
BIG = ((192, 640), (375, 1242))


def scene(seed, h, w):
    """A smooth depth field with about 8 % multiplicative noise, inverted -> scaled disparity [h,w] fp32 (depth 6 .. 90)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(0, 1, h)[:, None]
    x = torch.linspace(0, 1, w)[None, :]
    field = 6 + 40 * (1 - y) ** 2 + 3 * torch.sin(7 * x + seed) * y + 2 * torch.cos(5 * y * x)
    depth = field * (1 + 0.08 * torch.randn(h, w, generator=g)).clamp(0.5, 1.5) * 1.7
    return (1 / depth).float().numpy()


def resize_f64(img, H, W):
    """Bilinear, half-pixel centres, clamped source coordinates, in float64."""
    h, w = img.shape
    def axis(n_in, n_out):
        s = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, s - i0
    y0, y1, ly = axis(h, H)
    x0, x1, lx = axis(w, W)
    img = img.astype(np.float64)
    top = img[y0][:, x0] * (1 - lx) + img[y0][:, x1] * lx
    bot = img[y1][:, x0] * (1 - lx) + img[y1][:, x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def depth_f64(disp, size, scale, lo, hi, mode):
    """The exported depth in float64; scale, lo and hi are the fp32 values the fp32 paths divide and clamp with."""
    s, lo, hi = (np.float64(np.float32(v)) for v in (scale, lo, hi))
    if mode == "disp":
        d = s / resize_f64(disp, *size)
    else:
        d = s * resize_f64(1 / disp.astype(np.float64), *size)
    return np.clip(d, lo, hi)


def rel(a, b):
    """max |a - b| / |b|; equal entries count as 0, a difference from 0 as inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(d == 0, 0.0, d / np.abs(b))))


def colour_t(plane, size, vmin, vmax):
    """t = x * 256 per pixel in float64 (NaN where the value is); vmin == vmax: x = value * 0."""
    v = plane.astype(np.float64) if tuple(size) == plane.shape else resize_f64(plane, *size)
    vmin, vmax = np.float64(vmin), np.float64(vmax)
    with np.errstate(invalid="ignore"):
        x = (v - vmin) / (vmax - vmin) if vmin != vmax else v * 0.0
    return x * 256.0


def check_colours(img, t, table, what, cap=0.02, band=256e-5):
    """img [H,W,3] against the oracle's t: where t is further than `band` from every integer the bytes are the row of
    floor(t), clipped (NaN: black); elsewhere that row or a neighbour's.  -> the share of excused pixels, asserted < cap on
    the oracle's side first, so the cap cannot hide a failure."""
    nan = np.isnan(t)
    tt = np.where(nan, 0.0, t)
    idx = np.clip(np.floor(tt), 0, 255).astype(np.int64)
    near = (np.abs(tt - np.round(tt)) <= band) & ~nan
    share = float(near.mean())
    print(f"{what}: {share:.2%} of the pixels within {band} of an integer")
    assert share < cap, what
    want = table[idx]
    want[nan] = 0
    same = (img == want).all(-1)
    assert same[~near].all(), (what, int((~same[~near]).sum()))
    up, down = table[np.clip(idx + 1, 0, 255)], table[np.clip(idx - 1, 0, 255)]
    ok = same | (img == up).all(-1) | (img == down).all(-1)
    assert ok.all(), what
    return share
