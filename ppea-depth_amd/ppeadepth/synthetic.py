"""Deterministic synthetic inputs and weights (no datasets or checkpoints offline): data generation only,
no algorithm of the training path lives here.  Used by bench.py / smoke() to fill this repo's model; the golden generator fills the reference model
through the same functions, so both sides carry identical weights without shipping them.

The reference ships no weights that fit a fixture (238 M parameters), so golden
runs overwrite every tensor of the model's state_dict with values that are a pure
function of (key name, shape).  The golden generator (which holds the reference
model) and the tests / bench (which hold this repo's model) call the same
function, so both sides carry identical weights without shipping them.

Inputs follow SURVEY.md 8(d) config 1: uniform images from Generator(seed 1234),
KITTI normalised intrinsics (kitti_dataset.py:26-29; mono_dataset.py:173-182).
"""
import zlib

import numpy as np
import torch


def _gen(key: str) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    return g


def synth_tensor(key: str, ref: torch.Tensor, conditioned: bool = False) -> torch.Tensor:
    """Value for state_dict entry `key` with the shape/dtype of `ref`.
    conditioned: the WELL-CONDITIONED variant used by the rendered-frame fixtures (tests/golden/e2e_render.npz): the last
    BatchNorm of every residual branch gets a small scale (a near-identity trunk, like zero-initialised residual
    branches: perturbations of 2^-9 are no longer amplified by ~50 stacked random blocks), and the pose decoder's bias
    puts the predicted translation at the 1 m along the optical axis the frames are rendered with, so that the plane
    sweep has a real minimum instead of an argmin decided by rounding noise."""
    if conditioned:
        t = synth_tensor(key, ref)
        if key.endswith("pw2.bn.weight"):
            return t * 0.03
        if key == "pose.net.3.bias":
            t = t.clone()
            t[5] = 100.0               # translation_z = 0.01 * 100 (pose_decoder.py: outputs are scaled by 0.01)
        return t
    shape = tuple(ref.shape)
    if key.endswith("num_batches_tracked"):
        return torch.zeros(shape, dtype=ref.dtype)
    g = _gen(key)
    if key.endswith("running_mean"):
        return 0.05 * torch.randn(shape, generator=g)
    if key.endswith("running_var"):
        return 1.0 + 0.1 * torch.rand(shape, generator=g)
    is_bn = (".bn" in key or key.split(".")[-2].startswith("bn") or "_bn." in key
             or ".downsample.1." in key)
    if key.endswith(".bias"):
        return 0.05 * torch.randn(shape, generator=g)
    if key.endswith(".weight"):
        if is_bn and len(shape) == 1:
            return 1.0 + 0.1 * torch.randn(shape, generator=g)
        if len(shape) >= 2:
            fan_in = int(np.prod(shape[1:]))
            # adapter output projections are zero-initialised in the reference
            # (replknet_adapter.py:482-493); give them small non-zero values so the
            # adapter branch is exercised by parity tests.
            gain = 0.25 if "D_fc2" in key else 1.0
            return gain * torch.randn(shape, generator=g) / np.sqrt(fan_in)
        return 1.0 + 0.1 * torch.randn(shape, generator=g)
    return 0.05 * torch.randn(shape, generator=g)


@torch.no_grad()
def fill_state_dict(module: torch.nn.Module, conditioned: bool = False) -> None:
    """Overwrite every parameter and buffer of `module` with synth_tensor(key)."""
    sd = module.state_dict()
    for k, v in sd.items():
        v.copy_(synth_tensor(k, v, conditioned).to(v.dtype))


def kitti_K(height: int, width: int, scale: int):
    K = np.array([[0.58, 0, 0.5, 0],
                  [0, 1.92, 0.5, 0],
                  [0, 0, 1, 0],
                  [0, 0, 0, 1]], dtype=np.float32)
    K[0, :] *= width // (2 ** scale)
    K[1, :] *= height // (2 ** scale)
    inv_K = np.linalg.pinv(K)
    return torch.from_numpy(K), torch.from_numpy(inv_K)


def cityscapes_K(height: int, width: int, scale: int):
    """Normalised intrinsics of the preprocessed Cityscapes frames (cityscapes_preprocessed_dataset.py:37-53:
    fx = fy ~ 1131 px, principal point at the centre, divided by RAW_WIDTH 1024 / RAW_HEIGHT 384), scaled like
    mono_dataset.py:173-182."""
    K = np.array([[1131.0 / 1024, 0, 0.5, 0],
                  [0, 1131.0 / 384, 0.5, 0],
                  [0, 0, 1, 0],
                  [0, 0, 0, 1]], dtype=np.float32)
    K[0, :] *= width // (2 ** scale)
    K[1, :] *= height // (2 ** scale)
    inv_K = np.linalg.pinv(K)
    return torch.from_numpy(K), torch.from_numpy(inv_K)


def make_inputs(batch: int, height: int, width: int, seed: int = 1234,
                frame_ids=(0, -1, 1), scales=(0, 1, 2, 3), smooth: bool = False, intrinsics: str = "kitti"):
    """The row-P input dict of SURVEY 8(a).  `smooth=True` low-pass filters the
    images so neighbouring frames look alike (keeps losses in a realistic range)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    inputs = {}
    for f in frame_ids:
        base = torch.rand(batch, 3, height, width, generator=g)
        if smooth:
            k = torch.ones(3, 1, 9, 9) / 81.0
            base = torch.nn.functional.conv2d(
                torch.nn.functional.pad(base, (4, 4, 4, 4), mode="reflect"), k, groups=3)
        for s in scales:
            if s == 0:
                img = base
            else:
                img = torch.nn.functional.avg_pool2d(base, 2 ** s)
            inputs[("color", f, s)] = img.contiguous()
            inputs[("color_aug", f, s)] = img.contiguous().clone()
    for s in scales:
        K, inv_K = (kitti_K if intrinsics == "kitti" else cityscapes_K)(height, width, s)
        inputs[("K", s)] = K[None].repeat(batch, 1, 1).contiguous()
        inputs[("inv_K", s)] = inv_K[None].repeat(batch, 1, 1).contiguous()
    return inputs


# ---------------------------------------------------------------------------------------------
# synthetic validation split in the eigen_zhou on-disk format (kitti_dataset.py:46-62, trainer.py:766-767)
# ---------------------------------------------------------------------------------------------
def _scene(index, height, width, seed):
    """(texture [3,H,W] in [0,1], depth [H,W] in metres): a ground plane receding to the horizon plus smooth blobs."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed * 1000 + index)
    k = torch.ones(3, 1, 15, 15) / 225.0
    tex = torch.rand(1, 3, height + 14, width + 14, generator=g)
    tex = torch.nn.functional.conv2d(tex, k, groups=3)[0]
    tex = (tex - tex.amin()) / (tex.amax() - tex.amin() + 1e-6)
    ys = torch.linspace(0, 1, height)[:, None].expand(height, width)
    ground = 1.6 / (0.04 + 0.9 * (ys - 0.35).clamp_min(0.0))            # camera 1.6 m above the road
    sky = torch.full_like(ground, 70.0)
    depth = torch.where(ys > 0.37, ground.clamp(max=70.0), sky)
    blobs = torch.rand(1, 1, height // 16 + 1, width // 16 + 1, generator=g)
    blobs = torch.nn.functional.interpolate(blobs, (height, width), mode="bilinear", align_corners=False)[0, 0]
    depth = (depth * (0.6 + 0.5 * blobs)).clamp(1.5, 75.0)
    return tex, depth


def _render_neighbour(tex, depth, K, inv_K, tz):
    """Frame seen after moving the camera `tz` metres along its axis: inverse warp of the centre frame with its own
    depth (a first-order rendering: exact for fronto-parallel surfaces, good enough for synthetic data)."""
    H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W)], 0)
    cam = (inv_K[:3, :3] @ pix) * depth.reshape(1, -1)
    cam[2] += tz
    proj = K[:3, :3] @ cam
    u = proj[0] / proj[2].clamp_min(1e-3) / (W - 1) * 2 - 1
    v = proj[1] / proj[2].clamp_min(1e-3) / (H - 1) * 2 - 1
    grid = torch.stack([u, v], -1).reshape(1, H, W, 2)
    return torch.nn.functional.grid_sample(tex[None], grid, padding_mode="border", align_corners=True)[0]


def make_rendered_inputs(batch: int, height: int, width: int, seed: int = 7, tz: float = 1.0, scales=(0, 1, 2, 3),
                         intrinsics: str = "kitti", frame_ids=(0, -1, 1)):
    """Row-P input dict whose frames f != 0 are RENDERED from the centre frame's texture and a known depth map with the
    camera moved f * tz metres along its axis (the renderer of the synthetic validation split): smooth textures and a
    consistent geometry instead of white noise, for fixtures on which a reduced-precision step can be compared tightly."""
    Kf = kitti_K if intrinsics == "kitti" else cityscapes_K
    K, inv_K = Kf(height, width, 0)
    per = {f: [] for f in frame_ids}
    for i in range(batch):
        tex, depth = _scene(i, height, width, seed)
        for f in frame_ids:
            per[f].append(tex if f == 0 else _render_neighbour(tex, depth, K, inv_K, f * tz))
    inputs = {}
    for f in frame_ids:
        base = torch.stack(per[f])
        for s in scales:
            img = base if s == 0 else torch.nn.functional.avg_pool2d(base, 2 ** s)
            inputs[("color", f, s)] = img.contiguous()
            inputs[("color_aug", f, s)] = img.contiguous().clone()
    for s in scales:
        Ks, inv_Ks = Kf(height, width, s)
        inputs[("K", s)] = Ks[None].repeat(batch, 1, 1).contiguous()
        inputs[("inv_K", s)] = inv_Ks[None].repeat(batch, 1, 1).contiguous()
    return inputs


def make_eval_split(root, n=4, height=192, width=640, gt_hw=(375, 1242), seed=7, split="eigen_zhou_synth",
                    frame_ids=(0, -1, 1)):
    """Writes an eigen_zhou-format split under `root`:
         splits/<split>/val_files.txt      lines "<folder> <frame index> <l|r>"   (kitti_dataset.py:46-62)
         splits/<split>/gt_depths.npz      ["data"]: object array of [375,1242] float32 maps, 0 = no LiDAR return
         <folder>/image_02/data/<%010d>.npy frames t + f for f in frame_ids as float32 [3,H,W] in [0,1]
       and returns the list of split lines."""
    import os
    os.makedirs(os.path.join(root, "splits", split), exist_ok=True)
    K, inv_K = kitti_K(height, width, 0)
    lines, gts = [], []
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    for i in range(n):
        folder = f"synth_2011_09_26/synth_drive_{i:04d}_sync"
        frame = 5 + i
        tex, depth = _scene(i, height, width, seed)
        d = os.path.join(root, folder, "image_02", "data")
        os.makedirs(d, exist_ok=True)
        frames = {f: tex if f == 0 else _render_neighbour(tex, depth, K, inv_K, 0.4 * f) for f in frame_ids}
        for off, img in frames.items():
            np.save(os.path.join(d, f"{frame + off:010d}.npy"), img.numpy().astype(np.float32))
        gt = torch.nn.functional.interpolate(depth[None, None], gt_hw, mode="bilinear", align_corners=False)[0, 0]
        keep = torch.rand(gt_hw, generator=g) < 0.05                      # LiDAR-like sparsity
        gts.append((gt * keep).numpy().astype(np.float32))
        lines.append(f"{folder} {frame} l")
    with open(os.path.join(root, "splits", split, "val_files.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    arr = np.empty(len(gts), dtype=object)
    for i, gmap in enumerate(gts):
        arr[i] = gmap
    np.savez_compressed(os.path.join(root, "splits", split, "gt_depths.npz"), data=arr)
    return lines


class SynthEigenDataset(torch.utils.data.Dataset):
    """Reads a split written by `make_eval_split` the way KITTIRAWDataset reads eigen_zhou (kitti_dataset.py:46-62,
    mono_dataset.py:120-201, is_train=False: no augmentation): items are row-P dictionaries."""

    def __init__(self, root, split="eigen_zhou_synth", height=192, width=640, frame_idxs=(0, -1, 1), num_scales=4):
        import os
        self.root, self.height, self.width = root, height, width
        self.frame_idxs, self.num_scales = tuple(frame_idxs), num_scales
        with open(os.path.join(root, "splits", split, "val_files.txt")) as f:
            self.filenames = f.read().splitlines()
        self.gt_path = os.path.join(root, "splits", split, "gt_depths.npz")

    def __len__(self):
        return len(self.filenames)

    def gt_depths(self):
        return np.load(self.gt_path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]

    def __getitem__(self, index):
        import os
        folder, frame, _side = self.filenames[index].split()
        inputs = {}
        for f in self.frame_idxs:
            path = os.path.join(self.root, folder, "image_02", "data", f"{int(frame) + f:010d}.npy")
            img = torch.from_numpy(np.load(path)) if os.path.exists(path) else torch.zeros(3, self.height, self.width)
            for s in range(self.num_scales):
                t = img if s == 0 else torch.nn.functional.avg_pool2d(img[None], 2 ** s)[0]
                inputs[("color", f, s)] = t
                inputs[("color_aug", f, s)] = t
        for s in range(self.num_scales):
            K, inv_K = kitti_K(self.height, self.width, s)
            inputs[("K", s)], inputs[("inv_K", s)] = K, inv_K
        return inputs


def collate(items):
    return {k: torch.stack([it[k] for it in items]) for k in items[0]}


# ---------------------------------------------------------------------------------------------
# synthetic validation set in the DDAD loader's item format (datasets/ddad_dataset.py:116-167, is_train=False)
# ---------------------------------------------------------------------------------------------
def make_ddad_val(n=4, raw_hw=(1216, 1936), seed=7, valid=0.01, tz=0.4):
    """-> n items {"raw": {0, -1: uint8 [3,Hraw,Wraw]}, "intrinsics": float32 [3,3], "depth": float32 [Hraw,Wraw]}: what the
    DDAD loader reads per sample before its image path (`input_pipeline.DDADInputPipeline`), frame -1 rendered from frame 0
    with the camera moved back `tz` metres, the camera matrix of each sample its own, and a projected-LiDAR-like depth map
    with about `valid` of its pixels non-zero.  The road reaches from a few metres to the horizon and the region above it
    lies at 150 .. 250 m, so the map holds values in each class `val_ddad` tells apart: (1e-3, 80), [80, 200) and >= 200."""
    Hr, Wr = raw_hw
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    items = []
    for i in range(n):
        tex, depth = _scene(i, Hr, Wr, seed)
        ys = torch.linspace(0, 1, Hr)[:, None].expand(Hr, Wr)
        blobs = ((depth / torch.where(ys > 0.37, (1.6 / (0.04 + 0.9 * (ys - 0.35).clamp_min(0.0))).clamp(max=70.0),
                                      torch.full_like(depth, 70.0)) - 0.6) / 0.5).clamp(0, 1)
        depth = torch.where(ys > 0.37, depth * 2.0, 150.0 + 100.0 * blobs)
        f = Wr * (1.10 + 0.05 * float(torch.rand((), generator=g)))            # DDAD's front camera: fx ~ 1.13 x width
        intr = torch.tensor([[f, 0, Wr * (0.5 + 0.01 * float(torch.rand((), generator=g)))],
                             [0, f, Hr * (0.5 + 0.01 * float(torch.rand((), generator=g)))],
                             [0, 0, 1]], dtype=torch.float32)
        K = torch.eye(4)
        K[:3, :3] = intr
        prev = _render_neighbour(tex, depth, K, torch.linalg.inv(K), -tz)
        keep = torch.rand(Hr, Wr, generator=g) < valid
        to_u8 = lambda t: (t.clamp(0, 1) * 255).round().to(torch.uint8)      # noqa: E731
        items.append({"raw": {0: to_u8(tex), -1: to_u8(prev)}, "intrinsics": intr.numpy(),
                      "depth": (depth * keep).numpy().astype(np.float32)})
    return items


def collate_ddad(items):
    """-> (raw {f: uint8 [B,3,Hraw,Wraw]}, intrinsics float32 [B,3,3], depth float32 tensor [B,Hraw,Wraw])."""
    raw = {f: torch.stack([it["raw"][f] for it in items]) for f in items[0]["raw"]}
    return (raw, np.stack([it["intrinsics"] for it in items]),
            torch.from_numpy(np.stack([it["depth"] for it in items])))
