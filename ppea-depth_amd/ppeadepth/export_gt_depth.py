"""Export a KITTI split's ground-truth depth maps -- the reference's export_gt_depth.py.

"eigen": the raw velodyne scans projected with `vel_depth=True` (export_gt_depth.py:44-48), `batch` frames at a time through
`kitti_utils.project_depth_maps`: on a GPU one upload and one kernel call per batch.  "eigen_benchmark": the improved ground
truth's 16-bit PNGs / 256, read on the host.  The `.npz` holds `data`, an object array of float32 [H,W] maps (KITTI frames
differ in size): what `Trainer.val` takes as `np.load(path, allow_pickle=True)["data"]`.

    python -m ppeadepth.export_gt_depth --data_path KITTI --split eigen --split_file splits/eigen/test_files.txt --device cuda

`evaluate.DeviceGroundTruth.from_velodyne` is the same projection without the file.
"""
import argparse
import os

import numpy as np

from . import kitti_utils


def _frames(lines):
    for line in lines:
        if not line.strip():
            continue
        folder, frame_id = line.split()[:2]
        yield folder, int(frame_id)


def export_gt_depths_kitti(data_path, lines, split="eigen", output_path=None, device=None, batch=16):
    """lines: the split file's lines "<folder> <frame index> <side>".  -> the list of float32 [H,W] maps, in the lines' order;
    written to `output_path` (np.savez_compressed, `data=`) when one is given.  device: where "eigen" projects (None: "cpu")."""
    if split not in ("eigen", "eigen_benchmark"):
        raise ValueError(f"split {split!r}: 'eigen' or 'eigen_benchmark'")
    frames = list(_frames(lines))
    gt_depths = []
    if split == "eigen":
        calib = {}                                                   # one projection matrix per recording day
        for i in range(0, len(frames), batch):
            clouds, matrices, shapes = [], [], []
            for folder, frame_id in frames[i:i + batch]:
                calib_dir = os.path.join(data_path, folder.split("/")[0])
                if calib_dir not in calib:
                    calib[calib_dir] = kitti_utils.velo_to_image_matrix(calib_dir, 2)
                clouds.append(kitti_utils.load_velodyne_points(
                    os.path.join(data_path, folder, "velodyne_points/data", "{:010d}.bin".format(frame_id))))
                matrices.append(calib[calib_dir][0])
                shapes.append(calib[calib_dir][1])
            flat, table, _ = kitti_utils.project_depth_maps(clouds, matrices, shapes, True, device or "cpu")
            flat = flat.cpu().numpy()
            gt_depths += [flat[off:off + h * w].reshape(h, w).copy() for off, h, w in table.tolist()]
    else:
        import PIL.Image as pil
        for folder, frame_id in frames:
            path = os.path.join(data_path, folder, "proj_depth", "groundtruth", "image_02", "{:010d}.png".format(frame_id))
            gt_depths.append(np.array(pil.open(path)).astype(np.float32) / 256)
    if output_path is not None:
        data = np.empty(len(gt_depths), dtype=object)                # differently shaped maps: an object array, element-wise
        for i, m in enumerate(gt_depths):
            data[i] = m
        np.savez_compressed(output_path, data=data)
    return gt_depths


def main(argv=None):
    parser = argparse.ArgumentParser(description="export_gt_depth")
    parser.add_argument("--data_path", type=str, required=True, help="path to the root of the KITTI data")
    parser.add_argument("--split", type=str, required=True, choices=["eigen", "eigen_benchmark"],
                        help="which split to export gt from")
    parser.add_argument("--split_file", type=str, required=True, help="the split's file list, e.g. splits/eigen/test_files.txt")
    parser.add_argument("--output", type=str, default=None, help="the .npz to write (default: gt_depths.npz next to --split_file)")
    parser.add_argument("--device", type=str, default="cpu", help="where the eigen split is projected: cpu, cuda, cuda:1 ...")
    opt = parser.parse_args(argv)
    with open(opt.split_file) as f:
        lines = f.read().splitlines()
    output = opt.output or os.path.join(os.path.dirname(os.path.abspath(opt.split_file)), "gt_depths.npz")
    print("Exporting ground truth depths for {}".format(opt.split))
    maps = export_gt_depths_kitti(opt.data_path, lines, opt.split, output, opt.device)
    print("Saved {} maps to {}".format(len(maps), output))


if __name__ == "__main__":
    main()
