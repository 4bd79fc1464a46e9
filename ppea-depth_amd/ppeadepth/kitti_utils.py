"""KITTI ground truth from raw LiDAR -- the reference's kitti_utils.py under its own names.

`generate_depth_map` is a drop-in for the reference's function (kitti_utils.py:50-102) with a float64 result that equals it bit
for bit: the same numpy operations in the same order up to the scatter, then the `Counter` loop over duplicated keys restated
with `np.unique` / `np.minimum.at`.  (The reference itself stops at `np.int` on a current numpy.)

`project_depth_maps` is the batched form in the layout `evaluate.DeviceGroundTruth` holds: on "cpu" through the host path, on
a GPU through one upload of the scans and one `ops.velodyne_depth_maps` call (csrc/kitti_gt.hip).

One behaviour of the reference is kept on purpose, because it is part of the exported ground truth behind every published
number: duplicates are found through `sub2ind`, key = v * (W - 1) + u - 1, which is not a bijection -- pixel (v, W-1) and pixel
(v+1, 0) share a key.  For every key held by more than one valid point, the pixel of the key's FIRST point (in scan order)
receives the MINIMUM depth over all the key's points; when the key spans two pixels, the other pixel keeps its last-written
value, even if several points landed on it.
"""
import os

import numpy as np
import torch


_NUMERIC = frozenset("0123456789.e+- ")


def load_velodyne_points(filename):
    """KITTI velodyne .bin -> [N,4] float32 rows (forward, left, up, 1): the reflectance column is made homogeneous."""
    scan = np.fromfile(filename, dtype=np.float32).reshape(-1, 4)
    scan[:, 3] = 1.0
    return scan


def read_calib_file(path):
    """KITTI calibration text -> {key: float64 array where the value is a row of numbers, else the stripped string}."""
    data = {}
    with open(path) as f:
        for line in f:
            key, colon, value = line.partition(":")
            if not colon:
                continue
            value = value.strip()
            data[key] = value
            if _NUMERIC.issuperset(value):
                try:
                    data[key] = np.array([float(t) for t in value.split(" ")])
                except ValueError:      # e.g. a date made of digits and dashes: stays a string
                    pass
    return data


def sub2ind(matrixSize, rowSub, colSub):
    """The reference's "linear index": rowSub * (n - 1) + colSub - 1.  Not a bijection (module docstring); kept."""
    m, n = matrixSize
    return rowSub * (n - 1) + colSub - 1


def velo_to_image_matrix(calib_dir, cam=2):
    """-> (P float64 [3,4] = P_rect_0{cam} @ R_cam2rect @ velo2cam, (H, W) from S_rect_02 whatever `cam` is): the numpy
    operations of kitti_utils.py:54-66 in their order, so P has the reference's bits."""
    cam2cam = read_calib_file(os.path.join(calib_dir, 'calib_cam_to_cam.txt'))
    velo2cam = read_calib_file(os.path.join(calib_dir, 'calib_velo_to_cam.txt'))
    velo2cam = np.hstack((velo2cam['R'].reshape(3, 3), velo2cam['T'][..., np.newaxis]))
    velo2cam = np.vstack((velo2cam, np.array([0, 0, 0, 1.0])))
    im_shape = cam2cam["S_rect_02"][::-1].astype(np.int32)
    R_cam2rect = np.eye(4)
    R_cam2rect[:3, :3] = cam2cam['R_rect_00'].reshape(3, 3)
    P_rect = cam2cam['P_rect_0' + str(cam)].reshape(3, 4)
    P_velo2im = np.dot(np.dot(P_rect, R_cam2rect), velo2cam)
    return P_velo2im, (int(im_shape[0]), int(im_shape[1]))


def depth_map_from_points(velo, P_velo2im, im_shape, vel_depth=False):
    """kitti_utils.py:68-102 from the loaded scan on: velo [N,4] float32 (column 3 is taken as 1), P float64 [3,4], (H, W)
    -> float64 [H,W], the reference's bits."""
    velo = np.array(velo, dtype=np.float32).reshape(-1, 4)           # a copy: the caller's scan is not written to
    velo[:, 3] = 1.0
    velo = velo[velo[:, 0] >= 0, :]

    velo_pts_im = np.dot(P_velo2im, velo.T).T
    with np.errstate(divide="ignore", invalid="ignore"):             # q2 == 0: inf / NaN coordinates, invalid below
        velo_pts_im[:, :2] = velo_pts_im[:, :2] / velo_pts_im[:, 2][..., np.newaxis]
    if vel_depth:
        velo_pts_im[:, 2] = velo[:, 0]

    velo_pts_im[:, 0] = np.round(velo_pts_im[:, 0]) - 1
    velo_pts_im[:, 1] = np.round(velo_pts_im[:, 1]) - 1
    val_inds = (velo_pts_im[:, 0] >= 0) & (velo_pts_im[:, 1] >= 0)
    val_inds = val_inds & (velo_pts_im[:, 0] < im_shape[1]) & (velo_pts_im[:, 1] < im_shape[0])
    velo_pts_im = velo_pts_im[val_inds, :]

    depth = np.zeros((int(im_shape[0]), int(im_shape[1])))
    rows, cols, z = velo_pts_im[:, 1].astype(int), velo_pts_im[:, 0].astype(int), velo_pts_im[:, 2]
    depth[rows, cols] = z                                            # the last point in scan order on a pixel wins

    # per duplicated key: the minimum depth, written at the key's first point's pixel (np.unique's indices are first
    # occurrences: it sorts stably when it returns them)
    inds = sub2ind(depth.shape, velo_pts_im[:, 1], velo_pts_im[:, 0])
    keys, first, inverse, counts = np.unique(inds, return_index=True, return_inverse=True, return_counts=True)
    closest = np.full(keys.shape, np.inf)
    np.minimum.at(closest, inverse.reshape(-1), z)
    dupe = counts > 1
    depth[rows[first[dupe]], cols[first[dupe]]] = closest[dupe]
    depth[depth < 0] = 0
    return depth


def generate_depth_map(calib_dir, velo_filename, cam=2, vel_depth=False):
    """Generate a depth map from velodyne data: the reference's function, float64 [H,W], bit for bit."""
    P_velo2im, im_shape = velo_to_image_matrix(calib_dir, cam)
    return depth_map_from_points(load_velodyne_points(velo_filename), P_velo2im, im_shape, vel_depth)


def project_depth_maps(clouds, matrices, shapes, vel_depth=True, device="cpu"):
    """clouds: B scans [N_i,4] float32; matrices: B float64 [3,4] (`velo_to_image_matrix`); shapes: B (H, W).
    -> (flat fp32 [sum H*W], table int64 [B,3] = (offset, H, W), shapes), flat and table on `device`: what
    `evaluate.DeviceGroundTruth` holds.  "cpu": the host path cast to float32; a GPU: the scans are uploaded once, concatenated,
    and projected by one `ops.velodyne_depth_maps` call -- the maps never exist on the host."""
    clouds = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 4) for c in clouds]
    shapes = [(int(h), int(w)) for h, w in shapes]
    if not clouds or not len(clouds) == len(matrices) == len(shapes):
        raise ValueError(f"{len(clouds)} scans, {len(matrices)} matrices, {len(shapes)} shapes: one of each per frame, at least one")
    P = np.ascontiguousarray(np.stack([np.asarray(m, dtype=np.float64).reshape(3, 4) for m in matrices]))
    offsets = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])])
    table = torch.tensor([[int(offsets[i]), h, w] for i, (h, w) in enumerate(shapes)], dtype=torch.int64)
    device = torch.device(device)
    if device.type == "cpu":
        maps = [depth_map_from_points(c, P[i], shapes[i], vel_depth).astype(np.float32) for i, c in enumerate(clouds)]
        return torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps])), table, shapes
    from . import ops
    point_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64))
    points = torch.from_numpy(np.concatenate(clouds)).to(device)
    flat = ops.velodyne_depth_maps(points, point_offsets, torch.from_numpy(P).to(device), table, vel_depth)
    return flat, table.to(device), shapes
