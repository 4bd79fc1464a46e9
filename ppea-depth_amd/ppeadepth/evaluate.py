"""Depth evaluation -- the AbsRel harness of SURVEY 8(f)-2.

Restates the reference's metric code: `compute_errors` (evaluate_depth.py:35-54) and the per-image protocol inside
`Trainer.val` (trainer.py:780-835: resize the predicted disparity to the ground-truth size, Eigen crop, validity mask,
median scaling, clamp to [1e-3, 80]).  `cv2.resize(..., INTER_LINEAR)` is bilinear with half-pixel centres and no
antialiasing, i.e. `F.interpolate(mode="bilinear", align_corners=False)`.

Two statements of the same protocol: host-side numpy like the reference (`evaluate_image`, `evaluate_disps`), and the
device path (`DeviceGroundTruth`, `evaluate_disps_device`, `Trainer.val(metrics="device")`) that scores the disparities
where the predictor left them, on `ops.depth_errors` (csrc/eval_metrics.hip), with one copy to the host per split.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

MIN_VAL, MAX_VAL = 1e-3, 80.0          # trainer.py:657-658
MAX_VAL_DDAD = 200.0                   # trainer.py:605, :621: val_ddad's range test and clamp

ERROR_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


def compute_errors(gt, pred):
    """evaluate_depth.py:35-54 (numpy, same operation order)."""
    thresh = np.maximum((gt / pred), (pred / gt))
    a1 = (thresh < 1.25).mean()
    a2 = (thresh < 1.25 ** 2).mean()
    a3 = (thresh < 1.25 ** 3).mean()
    rmse = np.sqrt(((gt - pred) ** 2).mean())
    rmse_log = np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean())
    abs_rel = np.mean(np.abs(gt - pred) / gt)
    sq_rel = np.mean(((gt - pred) ** 2) / gt)
    return abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3


def resize_linear(img, width, height):
    """cv2.resize(img, (width, height)) with the default INTER_LINEAR for a 2-D float array."""
    t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32))[None, None]
    return F.interpolate(t, (height, width), mode="bilinear", align_corners=False)[0, 0].numpy()


def export_depth(pred_disp, size, scale=1.0, lo=1e-3, hi=80.0, mode="disp", dtype=np.float32):
    """The host statement of `ops.disp_export` for one image: pred_disp [h,w] scaled disparity -> depth [H,W] at size (H, W),
    fp32 throughout.  mode "disp": clip(scale / resize(pred), lo, hi) (with scale 5.4, lo 0, hi 80 and (352, 1216):
    eval_depth_ori.py:325-327); mode "depth": clip(scale * resize(1 / pred), lo, hi) (val_ddad).  dtype np.uint16:
    np.uint16(depth * 256) (eval_depth_ori.py:328)."""
    H, W = size
    pred = np.asarray(pred_disp, dtype=np.float32)
    s = np.float32(scale)
    same = (H, W) == pred.shape
    if mode == "disp":
        depth = s / (pred if same else resize_linear(pred, W, H))
    elif mode == "depth":
        depth = s * (1 / pred if same else resize_linear(1 / pred, W, H))
    else:
        raise ValueError(f"mode {mode!r}: 'disp' or 'depth'")
    depth = np.clip(depth, np.float32(lo), np.float32(hi))
    if np.dtype(dtype) == np.uint16:
        if not (lo >= 0 and np.float32(hi) * np.float32(256) <= 65535):
            raise ValueError(f"clamp [{lo}, {hi}] times 256 does not fit 16 bits")
        return np.uint16(depth * np.float32(256))
    return depth


def export_points(pred_disp, size, inv_K, color=None, pose=None, scale=1.0, lo=1e-3, hi=80.0, stride=1, edge=0.0,
                  mode="disp", offset=0):
    """The host statement of `ops.point_cloud` for one image: pred_disp [h,w] scaled disparity -> (xyz [N,3] fp32, rgb [N,3]
    uint8 or None, index [N] int64) at size (H, W), float32 arithmetic in the kernel's order.  d = `export_depth` without its
    clamp; candidates are the pixels with u % stride == v % stride == 0, kept iff lo < d < hi and (edge <= 0 or |d_n - d|
    <= edge * d for the 4-neighbours inside the image; a NaN neighbour drops nothing); point = pose @ (d * inv_K[:3,:3] @
    (u, v, 1)), pose None: the camera point.  inv_K, pose: [4,4] (inv_K at THIS size).  color: uint8 [H,W,3], or float
    [3,H,W] in [0,1] (byte = rint(c * 255) clipped).  index = offset + v * W + u, ascending (raster order)."""
    H, W = size
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"stride {stride}")
    f32 = np.float32
    d = export_depth(pred_disp, size, scale, -np.inf, np.inf, mode)
    lo, hi, edge = f32(lo), f32(hi), f32(edge)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = np.zeros((H, W), dtype=bool)
        keep[::stride, ::stride] = True
        keep &= (d > lo) & (d < hi)
        if edge > 0:
            tol = edge * d
            keep[:, 1:] &= ~(np.abs(d[:, :-1] - d[:, 1:]) > tol[:, 1:])
            keep[:, :-1] &= ~(np.abs(d[:, 1:] - d[:, :-1]) > tol[:, :-1])
            keep[1:] &= ~(np.abs(d[:-1] - d[1:]) > tol[1:])
            keep[:-1] &= ~(np.abs(d[1:] - d[:-1]) > tol[:-1])
        v, u = np.nonzero(keep)                                   # raster order
        dk = d[v, u]
        fu, fv = u.astype(f32), v.astype(f32)
        k = np.asarray(inv_K, dtype=f32)
        c = [((k[i, 0] * fu + k[i, 1] * fv) + k[i, 2]) * dk for i in range(3)]
        if pose is not None:
            m = np.asarray(pose, dtype=f32)
            c = [((m[i, 0] * c[0] + m[i, 1] * c[1]) + m[i, 2] * c[2]) + m[i, 3] for i in range(3)]
    xyz = np.stack(c, 1).astype(f32) if len(v) else np.zeros((0, 3), f32)
    rgb = None
    if color is not None:
        color = np.asarray(color)
        if color.dtype == np.uint8:
            if color.shape != (H, W, 3):
                raise ValueError(f"uint8 colour {color.shape}, expected {(H, W, 3)}")
            rgb = color[v, u]
        else:
            if color.shape != (3, H, W):
                raise ValueError(f"float colour {color.shape}, expected {(3, H, W)}")
            rgb = np.clip(np.rint(color.astype(f32)[:, v, u].T * f32(255)), 0, 255).astype(np.uint8)
    return xyz, rgb, offset + v.astype(np.int64) * W + u.astype(np.int64)


def eigen_crop_mask(gt_depth):
    """trainer.py:804-811: valid LiDAR returns inside Garg/Eigen's crop."""
    gt_height, gt_width = gt_depth.shape[:2]
    mask = np.logical_and(gt_depth > MIN_VAL, gt_depth < MAX_VAL)
    crop = np.array([0.40810811 * gt_height, 0.99189189 * gt_height,
                     0.03594771 * gt_width, 0.96405229 * gt_width]).astype(np.int32)
    crop_mask = np.zeros(mask.shape)
    crop_mask[crop[0]:crop[1], crop[2]:crop[3]] = 1
    return np.logical_and(mask, crop_mask)


def evaluate_image(pred_disp, gt_depth, eval_split="eigen", median_scaling=True, pred_depth_scale_factor=1.0):
    """One validation image (trainer.py:780-835): `pred_disp` [h,w] is the scaled disparity of
    `disp_to_depth(disp, 1e-3, 80)`; returns (the 7 errors, median ratio or None)."""
    gt_height, gt_width = gt_depth.shape[:2]
    if eval_split == "cityscapes":
        # the bottom 25 % (ego car) is cut off the ground truth first -- the loader did the same to the frames
        # (trainer.py:775-778); the prediction is resized to the CROPPED height
        gt_height = int(round(gt_height * 0.75))
        gt_depth = gt_depth[:gt_height]
    pred_depth = 1 / resize_linear(pred_disp, gt_width, gt_height)
    if eval_split == "cityscapes":
        gt_depth = gt_depth[256:, 192:1856]
        pred_depth = pred_depth[256:, 192:1856]
    if eval_split == "eigen":
        mask = eigen_crop_mask(gt_depth)
    else:
        mask = np.logical_and(gt_depth > MIN_VAL, gt_depth < MAX_VAL)
    pred_depth = pred_depth[mask]
    gt_depth = gt_depth[mask]
    pred_depth = pred_depth * pred_depth_scale_factor
    ratio = None
    if median_scaling:
        ratio = np.median(gt_depth) / np.median(pred_depth)
        pred_depth = pred_depth * ratio
    pred_depth[pred_depth < MIN_VAL] = MIN_VAL
    pred_depth[pred_depth > MAX_VAL] = MAX_VAL
    return compute_errors(gt_depth, pred_depth), ratio


def evaluate_disps(pred_disps, gt_depths, eval_split="eigen", median_scaling=True, pred_depth_scale_factor=1.0):
    """Mean of the 7 errors over a split (trainer.py:843)."""
    errors = [evaluate_image(pred_disps[i], gt_depths[i], eval_split, median_scaling, pred_depth_scale_factor)[0]
              for i in range(len(pred_disps))]
    return np.array(errors).mean(0)


def evaluate_image_ddad(pred_disp, gt_depth, median_scaling=True, pred_depth_scale_factor=1.0):
    """One image of `Trainer.val_ddad` (trainer.py:583-623), not `val`'s protocol with another crop: the scaled disparity
    `disp_to_depth(disp, 1e-3, 80)` [h,w] is inverted FIRST and the depth is resized with `F.interpolate(mode="bilinear")`;
    every pixel with 1e-3 < gt < 200 is scored, no crop; the clamp is [1e-3, 200].  Returns (the 7 errors, ratio or None).
    The name "ddad" in `evaluate_image` stays `val`'s 80 m range test (trainer.py:786-815)."""
    gt_depth = np.asarray(gt_depth)
    gt_height, gt_width = gt_depth.shape[-2:]
    pred_depth = 1. / torch.from_numpy(np.ascontiguousarray(pred_disp, dtype=np.float32))[None, None]
    pred_depth = F.interpolate(pred_depth, (gt_height, gt_width), mode="bilinear", align_corners=False)[0, 0].numpy()
    mask = np.logical_and(gt_depth > MIN_VAL, gt_depth < MAX_VAL_DDAD)
    pred_depth = pred_depth[mask]
    gt_depth = gt_depth[mask]
    pred_depth = pred_depth * pred_depth_scale_factor
    ratio = None
    if median_scaling:
        ratio = np.median(gt_depth) / np.median(pred_depth)
        pred_depth = pred_depth * ratio
    pred_depth[pred_depth < MIN_VAL] = MIN_VAL
    pred_depth[pred_depth > MAX_VAL_DDAD] = MAX_VAL_DDAD
    return compute_errors(gt_depth, pred_depth), ratio


def evaluate_disps_ddad(pred_disps, gt_depths, median_scaling=True, pred_depth_scale_factor=1.0):
    """Mean of the 7 errors of `evaluate_image_ddad` over the images (trainer.py:641)."""
    errors = [evaluate_image_ddad(pred_disps[i], gt_depths[i], median_scaling, pred_depth_scale_factor)[0]
              for i in range(len(pred_disps))]
    return np.array(errors).mean(0)


# ---- device path ---------------------------------------------------------------------------------------------------
def region_size(eval_split, gt_height, gt_width):
    """Rows x columns of the rectangle `evaluate_image` scores in a [gt_height, gt_width] map (the crop before the range
    test): the stride of the device workspace.  Mirrors the slicing above and `region_of` in csrc/eval_metrics.hip."""
    if eval_split == "eigen":
        crop = np.array([0.40810811 * gt_height, 0.99189189 * gt_height,
                         0.03594771 * gt_width, 0.96405229 * gt_width]).astype(np.int32)
        return max(int(crop[1] - crop[0]), 0) * max(int(crop[3] - crop[2]), 0)
    if eval_split == "cityscapes":
        return max(int(round(gt_height * 0.75)) - 256, 0) * max(min(1856, gt_width) - 192, 0)
    return gt_height * gt_width          # the range-test splits and "val_ddad": the whole map


class DeviceGroundTruth:
    """A split's ground-truth depth maps on the device, uploaded once and reusable across validations: one flat fp32
    buffer (KITTI maps differ in size) and the per-image table (offset, H_gt, W_gt) `ops.depth_errors` reads."""

    def __init__(self, gt_depths, device):
        maps = [np.ascontiguousarray(g, dtype=np.float32) for g in gt_depths]
        if not maps or any(m.ndim != 2 for m in maps):
            raise ValueError("gt_depths: a non-empty sequence of [H,W] depth maps")
        shapes = [m.shape for m in maps]
        offsets = np.concatenate([[0], np.cumsum([m.size for m in maps])])
        device = torch.device(device)
        self._set(torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).to(device),
                  torch.tensor([[int(offsets[i]), h, w] for i, (h, w) in enumerate(shapes)], dtype=torch.int64).to(device),
                  shapes, device)

    def _set(self, flat, table, shapes, device):
        """Everything an instance holds, for every constructor."""
        self.flat, self.table, self.shapes, self.device = flat, table, list(shapes), device

    @classmethod
    def from_batch(cls, depth, device):
        """The ground truth that arrives inside a batch (`data["depth"]` [B,H,W], ddad_dataset.py:165): a host tensor or array
        is uploaded with one copy, a device tensor is used where it is; the table is written on the device."""
        if not torch.is_tensor(depth):
            depth = torch.from_numpy(np.ascontiguousarray(depth))
        if depth.dim() != 3 or depth.shape[0] == 0:
            raise ValueError(f"depth: a [B,H,W] batch of depth maps, got {tuple(depth.shape)}")
        self = cls.__new__(cls)
        B, H, W = depth.shape
        device = torch.device(device)
        table = torch.stack([torch.arange(B, device=device) * (H * W),
                             torch.full((B,), H, device=device, dtype=torch.int64),
                             torch.full((B,), W, device=device, dtype=torch.int64)], 1)
        self._set(depth.to(device, torch.float32).contiguous().reshape(-1), table, [(H, W)] * B, device)
        return self

    @classmethod
    def from_velodyne(cls, clouds, matrices, shapes, device, vel_depth=True):
        """The ground truth projected from raw LiDAR where it will be scored (export_gt_depth.py without the file): B velodyne
        scans [N_i,4], their `kitti_utils.velo_to_image_matrix` matrices and (H, W) -> the maps of
        `kitti_utils.generate_depth_map(..., vel_depth)`, written by `ops.velodyne_depth_maps` into this layout; they are never
        on the host."""
        from . import kitti_utils
        self = cls.__new__(cls)
        device = torch.device(device)
        self._set(*kitti_utils.project_depth_maps(clouds, matrices, shapes, vel_depth, device), device)
        return self

    @classmethod
    def from_folder(cls, folder, count, device):
        """The ground truth the reference keeps as single files, `<folder>/<str(i).zfill(3)>_depth.npy` for i < count
        (trainer.py:760-780; Cityscapes: 1525 maps of 1024 x 2048).  One file at a time goes through one pinned staging
        buffer into a preallocated device buffer: the split is never whole on the host.  The maps are uploaded whole
        (`region_of` derives the crop from the nominal height); the layout is the constructor's."""
        device = torch.device(device)
        if count < 1:
            raise ValueError(f"count {count}: a split has at least one ground-truth map")
        paths = [os.path.join(folder, str(i).zfill(3) + "_depth.npy") for i in range(count)]
        for p in [folder] + paths:
            if not os.path.exists(p):
                raise FileNotFoundError(f"{p} not found: the Cityscapes ground truth is <splits_dir>/cityscapes/gt_depths/"
                                        "NNN_depth.npy, one file per line of the test split -- download ManyDepth's "
                                        "gt_depths_cityscapes.zip (see the reference's README) and unzip it into "
                                        "<splits_dir>/cityscapes")
        shapes = []
        for p in paths:                                       # the headers only: shapes and the size of the buffer
            m = np.load(p, mmap_mode="r")
            if m.ndim != 2:
                raise ValueError(f"{p}: a [H,W] depth map, got shape {m.shape}")
            shapes.append(tuple(int(d) for d in m.shape))
        sizes = [h * w for h, w in shapes]
        offsets = np.concatenate([[0], np.cumsum(sizes)])
        flat = torch.empty(int(offsets[-1]), device=device, dtype=torch.float32)
        stage = torch.empty(max(sizes), dtype=torch.float32)
        if device.type == "cuda":
            stage = stage.pin_memory()
        for i, p in enumerate(paths):
            if device.type == "cuda":
                torch.cuda.current_stream(device).synchronize()      # the copy that still reads the staging buffer
            np.copyto(stage[:sizes[i]].numpy().reshape(shapes[i]), np.load(p), casting="same_kind")
            flat[int(offsets[i]):int(offsets[i + 1])].copy_(stage[:sizes[i]], non_blocking=True)
        self = cls.__new__(cls)
        table = torch.tensor([[int(offsets[i]), h, w] for i, (h, w) in enumerate(shapes)], dtype=torch.int64).to(device)
        self._set(flat, table, shapes, device)
        return self

    def __len__(self):
        return len(self.shapes)

    def max_region(self, eval_split, first=0, count=None):
        last = len(self) if count is None else first + count
        return max(region_size(eval_split, h, w) for h, w in self.shapes[first:last])

    def score(self, pred_disps, first, eval_split="eigen", median_scaling=True, scale=1.0, out=None):
        """Images [first, first + B) of the split against pred_disps [B,h,w] (device, fp32): `ops.depth_errors`."""
        from . import ops
        B = pred_disps.shape[0]
        if first < 0 or first + B > len(self):
            raise ops._abi.PpeaKernelError(f"images [{first}, {first + B}) are not in a split of {len(self)}")
        return ops.depth_errors(pred_disps, self.flat, self.table[first:first + B], self.max_region(eval_split, first, B),
                                eval_split, median_scaling, scale, out=out)


def evaluate_disps_device(pred_disps, gt, eval_split="eigen", median_scaling=True, pred_depth_scale_factor=1.0, batch=16):
    """`evaluate_disps` on the device: pred_disps [N,h,w] (device tensor, or numpy: uploaded), gt a `DeviceGroundTruth`
    -> the 7 mean errors (numpy fp64).  Scored `batch` images at a time; one copy to the host."""
    from . import ops
    if not torch.is_tensor(pred_disps):
        pred_disps = torch.from_numpy(np.ascontiguousarray(pred_disps)).to(gt.device)
    if pred_disps.shape[0] != len(gt):
        raise ops._abi.PpeaKernelError(f"{pred_disps.shape[0]} predictions for a split of {len(gt)} images")
    errors = torch.empty(len(gt), 7, device=pred_disps.device, dtype=torch.float64)
    for i in range(0, len(gt), batch):
        gt.score(pred_disps[i:i + batch], i, eval_split, median_scaling, pred_depth_scale_factor, out=errors[i:i + batch])
    return ops.depth_errors_mean(errors).cpu().numpy()
