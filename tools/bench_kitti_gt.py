"""KITTI ground truth from raw LiDAR: the device path (csrc/kitti_gt.hip) against this project's host path on the same scans.

    python tools/bench_kitti_gt.py [--reps 5] [--out profiles/kitti_gt.json]            on the GPU
    python tools/bench_kitti_gt.py --reference-cpu [--out profiles/kitti_gt.json]       where the reference tree is (no GPU)

Synthetic full-turn scans of 120 000 points (64 beams, elevation -24.8 .. 2 degrees, 3 .. 80 m) against a KITTI-like rig at
375x1242 -- about a seventh of a scan lands in the image, as with real data -- in batches of 1, 16 and 64 frames,
`vel_depth=True` as export_gt_depth.py projects.  Per batch size, alternating the paths inside one process, median of `--reps`
after one warm-up each:
  host           `kitti_utils.project_depth_maps(..., "cpu")`: the vectorised numpy path, one frame after another
  device         `kitti_utils.project_depth_maps(..., "cuda")` from the same host arrays: concatenate, ONE upload, one
                 `ops.velodyne_depth_maps` call; the clock stops after a device synchronise, the maps stay on the device
  device_resident `ops.velodyne_depth_maps` alone on scans that are already on the device (workspace allocation and memset
                 included), host clock around a synchronised call
The device maps are compared with the host maps first (exact with vel_depth).  No figure here is a pass criterion.

--reference-cpu times the reference's own `generate_depth_map` (its file loaded by path, `np.int = int` set here; scan and
calibration written to a temporary directory, so it includes the file reads) beside this project's `generate_depth_map` on the
same files, and merges the result into the JSON under "reference_cpu".  It runs where the reference tree is, not on the GPU box.
"""
import argparse
import importlib.util
import json
import os
import platform
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ppea-depth_amd")]

SHAPE = (375, 1242)
POINTS = 120000
BATCHES = (1, 16, 64)
P_RECT = [[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]]
R_RECT = [[0.9999239, 0.00983776, -0.00744505], [-0.0098698, 0.9999421, -0.00427846], [0.00740253, 0.00435161, 0.9999631]]
VELO_R = [[0.007533745, -0.9999714, -0.000616602], [0.01480249, 0.0007280733, -0.9998902], [0.9998621, 0.00752379, 0.01480755]]
VELO_T = [-0.004069766, -0.07631618, -0.2717806]


def matrix():
    R = np.eye(4)
    R[:3, :3] = R_RECT
    V = np.eye(4)
    V[:3, :3], V[:3, 3] = VELO_R, VELO_T
    return np.array(P_RECT) @ R @ V


def calibration_text():
    row = lambda v: " ".join("{:.9e}".format(float(x)) for x in np.asarray(v).reshape(-1))      # noqa: E731
    cam = "".join(f"S_rect_0{c}: {row([SHAPE[1], SHAPE[0]])}\nR_rect_0{c}: {row(R_RECT)}\nP_rect_0{c}: {row(P_RECT)}\n" for c in range(4))
    return "calib_time: 09-Jan-2012 13:57:47\n" + cam, f"calib_time: 15-Mar-2012 11:37:16\nR: {row(VELO_R)}\nT: {row(VELO_T)}\n"


def scan(seed):
    rs = np.random.RandomState(seed)
    az = rs.uniform(-np.pi, np.pi, POINTS)
    el = np.deg2rad(np.linspace(-24.8, 2.0, 64))[rs.randint(0, 64, POINTS)]
    r = rs.uniform(3.0, 80.0, POINTS)
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rs.uniform(0, 1, POINTS)], 1)
    return pts.astype(np.float32)


def median_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)


def merge(path, update):
    res = {}
    if os.path.exists(path):
        with open(path) as f:
            res = json.load(f)
    res.update(update)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


def reference_cpu(args):
    from oracle import ref_harness as rh
    from ppeadepth import kitti_utils
    if not rh.reference_available():
        raise SystemExit("the reference tree is not present: --reference-cpu runs in the build container only")
    spec = importlib.util.spec_from_file_location("_reference_kitti_utils", os.path.join(rh.REFERENCE_ROOT, "ppeadepth", "kitti_utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    np.int = int                                               # the reference still says np.int
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in zip(("calib_cam_to_cam.txt", "calib_velo_to_cam.txt"), calibration_text()):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        velo = os.path.join(tmp, "0000000000.bin")
        scan(0).tofile(velo)
        a, b = ref.generate_depth_map(tmp, velo, 2, True), kitti_utils.generate_depth_map(tmp, velo, 2, True)
        assert a.tobytes() == b.tobytes()
        cell = {"what": "one frame, generate_depth_map(calib_dir, velo_filename, 2, True) including the file reads, ms: "
                        "median, min, max of %d calls after one warm-up" % args.reps,
                "reference_ms": median_ms(lambda: ref.generate_depth_map(tmp, velo, 2, True), args.reps),
                "this_project_host_ms": median_ms(lambda: kitti_utils.generate_depth_map(tmp, velo, 2, True), args.reps),
                "bit_equal": True, "valid_pixels": int((a > 0).sum()),
                "host": {"nproc": os.cpu_count(), "machine": platform.machine(), "numpy": np.__version__},
                "command": "python tools/bench_kitti_gt.py --reference-cpu --reps %d" % args.reps}
    print(json.dumps(merge(args.out, {"reference_cpu": cell})["reference_cpu"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti_gt.json"))
    ap.add_argument("--reference-cpu", action="store_true")
    args = ap.parse_args()
    if args.reference_cpu:
        return reference_cpu(args)
    import torch
    from ppeadepth import kitti_utils, ops
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the device path is timed on an MI355X, there is nothing to fall back to")
    dev = torch.device("cuda:0")
    P = matrix()
    scans = [scan(s) for s in range(8)]
    cells = {}
    for B in BATCHES:
        clouds = [scans[i % len(scans)] for i in range(B)]
        matrices, shapes = [P] * B, [SHAPE] * B
        want, table, _ = kitti_utils.project_depth_maps(clouds, matrices, shapes, True, "cpu")
        got = kitti_utils.project_depth_maps(clouds, matrices, shapes, True, dev)[0]
        assert torch.equal(got.cpu(), want), "device maps differ from the host path"
        points = torch.from_numpy(np.concatenate(clouds)).to(dev)
        offsets = torch.arange(B + 1, dtype=torch.int64) * POINTS
        Pd = torch.from_numpy(np.stack(matrices)).to(dev)

        def host():
            kitti_utils.project_depth_maps(clouds, matrices, shapes, True, "cpu")

        def device():
            kitti_utils.project_depth_maps(clouds, matrices, shapes, True, dev)
            torch.cuda.synchronize()

        def resident():
            ops.velodyne_depth_maps(points, offsets, Pd, table, True)
            torch.cuda.synchronize()

        host_reps = max(2, args.reps // (1 if B < 16 else 2))
        rows = {"host": [], "device": [], "device_resident": []}
        for fn in (host, device, resident):                    # warm-up of every path
            fn()
        for rep in range(args.reps):                           # alternating: the paths share whatever else the host is doing
            for name, fn in (("host", host), ("device", device), ("device_resident", resident)):
                if name == "host" and rep >= host_reps:
                    continue
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                rows[name].append((time.perf_counter() - t) * 1e3)
        cell = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                    "ms_per_frame": round(statistics.median(v) / B, 4), "calls": len(v)} for k, v in rows.items()}
        cell["valid_pixels_per_frame"] = int((want > 0).sum()) // B
        cell["workspace_MB"] = round(ops._abi.lib.ppea_velodyne_depth_workspace_bytes(B * SHAPE[0] * SHAPE[1]) / 2 ** 20, 1)
        cell["upload_MB"] = round(B * POINTS * 16 / 2 ** 20, 1)
        cell["device_maps_equal_host_maps"] = True
        cells[f"batch_{B}"] = cell
        print(f"B={B}: " + json.dumps(cell), flush=True)
    res = merge(args.out, {
        "metric": "wall ms to project B synthetic 120 000-point velodyne scans into 375x1242 depth maps (vel_depth=True), "
                  "host clock around work that ends in a device synchronise; median / min / max over alternating calls",
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "cells": cells,
        "command": "python tools/bench_kitti_gt.py --reps %d" % args.reps})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
