"""Colour pictures of a predicted plane (the reference's `vis.colorize`, eval_depth_ori.py:275-277).

`colorize` is the reference's function on the host in numpy; `colorize_device` makes the same picture for a whole batch on
the GPU (ops.plane_range + ops.colorize), optionally at another size.  Both look colours up in the 256 x 3 uint8 tables
shipped next to this file (`colormaps.json`, written by tools/gen_colormaps.py from matplotlib's listed colormaps), so the
package does not need matplotlib at run time; the lookup is matplotlib's `Colormap.__call__(bytes=True)`:
row floor(x * 256), x < 0 row 0, x >= 1 row 255, NaN the bytes (0, 0, 0).

`write_ply` / `read_ply` keep a point cloud (`DepthPredictor.points`) as a binary little-endian PLY file.
"""
import json
import os

import numpy as np
import torch

CMAPS = ("plasma", "magma", "viridis", "inferno")
_TABLES = {}
_DEVICE_TABLES = {}


def _table(name):
    if not _TABLES:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "colormaps.json")) as f:
            for k, lines in json.load(f).items():            # 16 strings of 16 "rrggbb" rows
                _TABLES[k] = np.frombuffer(bytes.fromhex("".join(lines).replace(" ", "")), np.uint8).reshape(256, 3).copy()
    if name not in _TABLES:
        raise ValueError(f"colormap {name!r} is not shipped; one of {sorted(_TABLES)}")
    return _TABLES[name]


def lut(name="plasma", device=None):
    """The [256,3] uint8 table of a colormap: a numpy array (device None) or a tensor on `device`, kept per device."""
    if device is None:
        return _table(name)
    key = (name, torch.device(device))
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = torch.from_numpy(_table(name).copy()).to(key[1])
    return _DEVICE_TABLES[key]


def lookup(x, table):
    """matplotlib's Colormap.__call__(x, bytes=True)[..., :3] for a 256-entry table, in x's own float type."""
    x = np.asarray(x)
    if not np.issubdtype(x.dtype, np.floating):
        x = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        bad = np.isnan(x)
        xa = x * x.dtype.type(256)
        xa[xa == 256] = 255
        under, over = xa < 0, xa >= 256
        idx = np.where(bad | under | over, 0, xa).astype(np.int64)
    idx[over] = 255
    out = table[idx]
    out[bad] = 0
    return out


def colorize(value, vmin=10, vmax=1000, cmap="plasma"):
    """value [H,W] -> RGB uint8 [H,W,3].  The reference's semantics: vmin / vmax None = the value's min / max; the plane
    is normalised to (value - vmin) / (vmax - vmin), or to value * 0 when vmin == vmax, then looked up."""
    value = np.asarray(value)
    vmin = value.min() if vmin is None else vmin
    vmax = value.max() if vmax is None else vmax
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if vmin != vmax:
            value = (value - vmin) / (vmax - vmin)
        else:
            value = value * 0.
    return lookup(value, _table(cmap))


@torch.no_grad()
def colorize_device(value, size=None, vmin=None, vmax=None, percentile=100.0, cmap="plasma", out=None):
    """value [B,h,w] (or [B,1,h,w]) fp32 tensor -> RGB uint8 [B,H,W,3], or (flat [sum H W, 3], table [B,3] int64 (offset, H,
    W)) when `size` lists B different sizes.  size None: the value's own size, else (H, W) or B pairs; the resize is
    cv2.resize(INTER_LINEAR), as `evaluate.resize_linear`.
    vmin / vmax None: per image the minimum / the `percentile`-th percentile (100: the maximum) of the values that are not NaN.
    These statistics are taken on the SOURCE plane -- what the network predicted -- not on the resized one; a caller who
    wants anything else passes vmin / vmax.
    On a HIP tensor this is ops.plane_range (only if a bound is missing) + ops.colorize on the current stream; with `out`
    nothing but the [B,2] range is allocated.  A CPU tensor takes the numpy path (`colorize`)."""
    from . import ops
    value = ops._planes(value, "colorize_device")
    B, h, w = value.shape
    sizes = ops.target_sizes((h, w) if size is None else size, B)
    if value.is_cuda:
        value = value.float().contiguous()
        if vmin is None or vmax is None:
            rng = ops.plane_range(value, percentile)
        else:
            rng = torch.empty(B, 2, device=value.device, dtype=torch.float32)
        if vmin is not None:                 # fills on the device: nothing is copied from the host, so this can be captured
            rng[:, 0] = float(vmin)
        if vmax is not None:
            rng[:, 1] = float(vmax)
        return ops.colorize(value, sizes, rng, lut(cmap, value.device), out=out)
    from .evaluate import resize_linear
    planes = value.float().numpy()
    imgs = []
    for b, (H, W) in enumerate(sizes):
        p = planes[b]
        ok = p[~np.isnan(p)]
        lo = (ok.min() if ok.size else np.float32(np.nan)) if vmin is None else np.float32(vmin)
        hi = (np.percentile(ok.astype(np.float64), percentile).astype(np.float32) if ok.size else np.float32(np.nan)) \
            if vmax is None else np.float32(vmax)
        imgs.append(colorize(p if (H, W) == (h, w) else resize_linear(p, W, H), lo, hi, cmap))
    return ops.host_export(imgs, sizes, out)


def _ply_header(n, colour):
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}", "property float x", "property float y",
             "property float z"]
    if colour:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    return lines + ["end_header"]


def _ply_dtype(colour):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    return np.dtype(fields + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if colour else []))


def write_ply(path, xyz, rgb=None):
    """xyz [N,3] float32 (and rgb [N,3] uint8) -> a binary little-endian PLY file: `float x y z`, then `uchar red green
    blue` when colour is given; 12 or 15 bytes per point.  N = 0 is a valid file.  Arrays or host tensors."""
    xyz = np.asarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz {xyz.shape}: expected [N,3]")
    rec = np.empty(xyz.shape[0], dtype=_ply_dtype(rgb is not None))
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgb is not None:
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.shape != xyz.shape:
            raise ValueError(f"rgb {rgb.dtype} {rgb.shape} for xyz {xyz.shape}: expected uint8 of the same shape")
        rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with open(path, "wb") as f:
        f.write(("\n".join(_ply_header(xyz.shape[0], rgb is not None)) + "\n").encode("ascii"))
        f.write(rec.tobytes())


def read_ply(path):
    """A file `write_ply` wrote -> (xyz [N,3] float32, rgb [N,3] uint8 or None)."""
    with open(path, "rb") as f:
        lines = []
        while not lines or lines[-1] != "end_header":
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            lines.append(line.decode("ascii").rstrip("\n"))
        payload = f.read()
    if len(lines) < 3 or not lines[2].startswith("element vertex "):
        raise ValueError(f"{path}: not a vertex-only PLY file")
    n = int(lines[2].split()[2])
    colour = len(lines) > 7
    if lines != _ply_header(n, colour):
        raise ValueError(f"{path}: a PLY layout write_ply does not write")
    dt = _ply_dtype(colour)
    if len(payload) != n * dt.itemsize:
        raise ValueError(f"{path}: {len(payload)} payload bytes for {n} points of {dt.itemsize} bytes")
    rec = np.frombuffer(payload, dtype=dt)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    rgb = (np.stack([rec["red"], rec["green"], rec["blue"]], 1) if n else np.zeros((0, 3), np.uint8)) if colour else None
    return xyz, rgb
