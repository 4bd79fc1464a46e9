"""KITTI ground truth from raw LiDAR, host side (no GPU): `ppeadepth.kitti_utils.generate_depth_map` against the reference's
own output bit for bit (tests/golden/kitti_gt.npz, written by tools/gen_kitti_gt_golden.py from the unmodified reference), the
semantics of the duplicate resolution on a hand-built image, the flat layout of `project_depth_maps`, the exported `.npz`, and
the refusals of the new entry point that need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

CASES = ("a", "b")


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(GOLDEN, "kitti_gt.npz")) as z:
        return {k: z[k] for k in z.files}


def write_drive(folder, fixture, case):
    """The two calibration files of a golden case in KITTI's layout."""
    os.makedirs(folder, exist_ok=True)
    for name, key in (("calib_cam_to_cam.txt", "cam2cam"), ("calib_velo_to_cam.txt", "velo2cam")):
        with open(os.path.join(folder, name), "w") as f:
            f.write(str(fixture[f"{case}:{key}"]))


@pytest.mark.parametrize("vel_depth", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_generate_depth_map_equals_the_reference_bit_for_bit(fixture, tmp_path, case, vel_depth):
    from ppeadepth import kitti_utils
    write_drive(tmp_path, fixture, case)
    velo = os.path.join(tmp_path, "0000000000.bin")
    fixture[f"{case}:points"].tofile(velo)
    want = fixture[f"{case}:depth_vel" if vel_depth else f"{case}:depth"]
    got = kitti_utils.generate_depth_map(str(tmp_path), velo, 2, vel_depth)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()
    assert (got > 0).sum() > got.size // 2                                        # a populated map, not a trivial match


@pytest.mark.parametrize("case", CASES)
def test_velo_to_image_matrix_is_bit_equal_to_the_reference(fixture, tmp_path, case):
    from ppeadepth import kitti_utils
    write_drive(tmp_path, fixture, case)
    P, shape = kitti_utils.velo_to_image_matrix(str(tmp_path), 2)
    want = fixture[f"{case}:P"]
    assert P.dtype == np.float64 and P.shape == (3, 4) and P.tobytes() == want.tobytes()
    assert shape == fixture[f"{case}:depth"].shape
    P3, shape3 = kitti_utils.velo_to_image_matrix(str(tmp_path), 3)               # another camera: its P, still S_rect_02
    assert shape3 == shape and not np.array_equal(P3, P)
    calib = kitti_utils.read_calib_file(os.path.join(tmp_path, "calib_cam_to_cam.txt"))
    assert isinstance(calib["calib_time"], str) and calib["P_rect_02"].shape == (12,)
    assert kitti_utils.sub2ind((3, 4), 0, 0) == -1 and kitti_utils.sub2ind((3, 4), 0, 3) == kitti_utils.sub2ind((3, 4), 1, 0)


# ---- a hand-built 3x4 image ------------------------------------------------------------------------------------------------
# P maps a velodyne point (x, y, z) to q = (y, z, x - 0.5): a point made by `at(v, u, d)` lands on pixel (v, u) with q2 = d
# exactly (every number is a small multiple of 1/4), so its depth is d, or x = d + 0.5 with vel_depth.
HAND_SHAPE = (3, 4)
HAND_P = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, -0.5]], dtype=np.float64)


def at(v, u, d):
    return [d + 0.5, (u + 1) * d, (v + 1) * d, 0.25]


HAND_SCANS = {
    # the first point of the shared key 2 sits on (0, 3)
    "first_on_row_end": np.array([
        at(0, 3, 5), at(1, 0, 2), at(0, 3, 7),          # (0,3) and (1,0) share key 2: (0,3) <- min over BOTH pixels = 2
        at(2, 2, 8), at(2, 2, 4), at(2, 2, 6),          # one pixel, three points: last is 6, the minimum 4 wins
        at(0, 0, 3), at(0, 0, 9),                       # pixel (0,0): key -1
        [0.5, 1, 1, 0], [0.5, 0, 0, 0],                 # q2 == 0: inf and NaN coordinates, invalid
        [-0.0, -0.5, -1.5, 0], at(2, 0, 4),             # x = -0.0 passes x >= 0 and lands on (2,0) with q2 = -0.5
        [-1.0, -3, -3, 0], at(1, 1, 5),                 # x < 0 is dropped; kept, it would drag (1,1) to 0
        at(0, 4, 1), at(3, 0, 1),                       # out of bounds; (0,4) would share key 3 with (1,1)
        at(1, 2, 2.5),                                  # a single hit
    ], dtype=np.float32),
    # the first point of the shared key sits on (1, 0); (0, 3) keeps its last-written 7 although a 3 landed there
    "first_on_row_start": np.array([at(1, 0, 6), at(0, 3, 3), at(0, 3, 7)], dtype=np.float32),
    "empty": np.zeros((0, 4), dtype=np.float32),
}
HAND_WANT = {        # (scan, vel_depth) -> the map
    ("first_on_row_end", False): [[3, 0, 0, 2], [2, 5, 2.5, 0], [0, 0, 4, 0]],
    ("first_on_row_end", True): [[3.5, 0, 0, 2.5], [2.5, 5.5, 3, 0], [0, 0, 4.5, 0]],
    ("first_on_row_start", False): [[0, 0, 0, 7], [3, 0, 0, 0], [0, 0, 0, 0]],
    ("first_on_row_start", True): [[0, 0, 0, 7.5], [3.5, 0, 0, 0], [0, 0, 0, 0]],
    ("empty", False): np.zeros(HAND_SHAPE),
    ("empty", True): np.zeros(HAND_SHAPE),
}


@pytest.mark.parametrize("vel_depth", [False, True])
@pytest.mark.parametrize("scan", sorted(HAND_SCANS))
def test_duplicate_resolution_on_a_hand_built_image(scan, vel_depth):
    from ppeadepth import kitti_utils
    points = HAND_SCANS[scan].copy()
    got = kitti_utils.depth_map_from_points(points, HAND_P, HAND_SHAPE, vel_depth)
    assert got.dtype == np.float64 and np.array_equal(got, np.array(HAND_WANT[scan, vel_depth], dtype=np.float64))
    assert np.array_equal(points, HAND_SCANS[scan], equal_nan=True)               # the caller's scan is not written to


def test_the_x_filter_keeps_minus_zero():
    """Without the x = -0.0 point, pixel (2,0) of the hand-built scan would hold its other point's depth."""
    from ppeadepth import kitti_utils
    points = HAND_SCANS["first_on_row_end"]
    keep = np.ones(len(points), bool)
    keep[10] = False
    assert np.signbit(points[10, 0]) and points[10, 0] == 0
    assert kitti_utils.depth_map_from_points(points[keep], HAND_P, HAND_SHAPE, False)[2, 0] == 4
    assert kitti_utils.depth_map_from_points(points, HAND_P, HAND_SHAPE, False)[2, 0] == 0


# ---- the batched layout ----------------------------------------------------------------------------------------------------
def test_project_depth_maps_on_the_host_is_the_device_ground_truth_layout(fixture):
    from ppeadepth import evaluate, kitti_utils
    clouds = [fixture["a:points"], fixture["b:points"]]
    matrices = [fixture["a:P"], fixture["b:P"]]
    shapes = [fixture["a:depth"].shape, fixture["b:depth"].shape]
    for vel_depth, key in ((True, "depth_vel"), (False, "depth")):
        maps = [fixture[f"a:{key}"], fixture[f"b:{key}"]]
        want = evaluate.DeviceGroundTruth(maps, "cpu")
        flat, table, got_shapes = kitti_utils.project_depth_maps(clouds, matrices, shapes, vel_depth, "cpu")
        assert flat.dtype == torch.float32 and table.dtype == torch.int64
        assert torch.equal(table, want.table) and table.tolist() == [[0, 5, 7], [35, 8, 11]]
        assert torch.equal(flat, want.flat) and got_shapes == want.shapes
        gt = evaluate.DeviceGroundTruth.from_velodyne(clouds, matrices, shapes, "cpu", vel_depth)
        assert torch.equal(gt.flat, want.flat) and torch.equal(gt.table, want.table) and gt.shapes == want.shapes and len(gt) == 2
    with pytest.raises(ValueError):
        kitti_utils.project_depth_maps(clouds, matrices[:1], shapes)
    with pytest.raises(ValueError):
        kitti_utils.project_depth_maps([], [], [])


# ---- export ------------------------------------------------------------------------------------------------------------------
def kitti_tree(root, fixture):
    """Two frames of two recording days in KITTI's raw layout -> the split file's lines."""
    lines = []
    for case, day, drive, frame, side in (("a", "2011_09_26", "2011_09_26_drive_0001_sync", 5, "l"),
                                          ("b", "2011_09_28", "2011_09_28_drive_0002_sync", 17, "r")):
        write_drive(os.path.join(root, day), fixture, case)
        data = os.path.join(root, day, drive, "velodyne_points", "data")
        os.makedirs(data)
        fixture[f"{case}:points"].tofile(os.path.join(data, f"{frame:010d}.bin"))
        lines.append(f"{day}/{drive} {frame} {side}")
    return lines


def test_export_gt_depths_kitti_round_trips_through_the_npz(fixture, tmp_path):
    from ppeadepth import evaluate, export_gt_depth
    root = str(tmp_path / "kitti")
    lines = kitti_tree(root, fixture)
    out = str(tmp_path / "gt_depths.npz")
    want = [fixture["a:depth_vel"].astype(np.float32), fixture["b:depth_vel"].astype(np.float32)]
    for batch in (16, 1):                                                         # one batch, and one frame per batch
        maps = export_gt_depth.export_gt_depths_kitti(root, lines, "eigen", out, batch=batch)
        data = np.load(out, allow_pickle=True)["data"]
        assert data.dtype == object and len(data) == len(maps) == 2
        for got, back, ref in zip(maps, data, want):
            assert got.dtype == back.dtype == np.float32
            assert got.tobytes() == ref.tobytes() and back.tobytes() == ref.tobytes() and back.shape == ref.shape
    assert torch.equal(evaluate.DeviceGroundTruth(data, "cpu").flat, evaluate.DeviceGroundTruth(want, "cpu").flat)
    # the command line: the split file is the caller's
    split_file = tmp_path / "test_files.txt"
    split_file.write_text("\n".join(lines) + "\n")
    export_gt_depth.main(["--data_path", root, "--split", "eigen", "--split_file", str(split_file)])
    data = np.load(str(tmp_path / "gt_depths.npz"), allow_pickle=True)["data"]
    assert all(np.array_equal(a, b) for a, b in zip(data, want))
    with pytest.raises(ValueError):
        export_gt_depth.export_gt_depths_kitti(root, lines, "odom")


def test_export_eigen_benchmark_reads_the_pngs(tmp_path):
    from PIL import Image
    from ppeadepth import export_gt_depth
    rs = np.random.RandomState(0)
    raw = (rs.randint(0, 65536, size=(6, 9)) * (rs.uniform(size=(6, 9)) < 0.4)).astype(np.uint16)
    folder = "2011_09_26/2011_09_26_drive_0002_sync"
    png = tmp_path / folder / "proj_depth" / "groundtruth" / "image_02"
    os.makedirs(png)
    Image.fromarray(raw).save(str(png / "0000000007.png"))
    out = str(tmp_path / "bench.npz")
    maps = export_gt_depth.export_gt_depths_kitti(str(tmp_path), [f"{folder} 7 l"], "eigen_benchmark", out)
    assert maps[0].dtype == np.float32 and np.array_equal(maps[0], raw.astype(np.float32) / 256)
    assert np.array_equal(np.load(out, allow_pickle=True)["data"][0], maps[0])


# ---- the entry point, as far as it goes without a device ---------------------------------------------------------------------
def test_velodyne_depth_abi_and_host_side_refusals():
    """The launcher reads its two host arrays before it touches the device: every refusal comes back from a call whose device
    pointers are never used, on a machine with or without a GPU."""
    from ppeadepth import _abi
    assert _abi.lib.ppea_abi_version() == _abi.ABI_VERSION >= 25                  # 25: the version these entry points arrived with
    assert len(_abi.SIGNATURES["ppea_velodyne_depth_f32"]) == 9 and len(_abi.SIGNATURES["ppea_velodyne_depth_workspace_bytes"]) == 1
    ws = _abi.lib.ppea_velodyne_depth_workspace_bytes
    # per pixel: two 64-bit words (last point of the pixel, first point of the key) and two 32-bit words (highest order, minimum)
    n = 375 * 1242
    assert 24 * n <= ws(n) <= 24 * n + 4 * 256 and ws(0) == 0 and ws(-1) == -2 and ws(2 * n) > ws(n)

    def run(offsets, table, B=None):
        off = np.asarray(offsets, dtype=np.int64)
        tab = np.ascontiguousarray(table, dtype=np.int64)
        dummy = ctypes.c_void_p(256)                                              # never dereferenced by a refused call
        return _abi.lib.ppea_velodyne_depth_f32(dummy, off.ctypes.data_as(ctypes.c_void_p), len(tab) if B is None else B, dummy,
                                                tab.ctypes.data_as(ctypes.c_void_p), 1, dummy, dummy, None)
    good = [[0, 5, 7], [35, 8, 11]]
    assert run([0, 10, 20], good, B=0) == -2
    assert run([0, 10, 5], good) == -2                                            # descending offsets
    assert run([-1, 10, 20], good) == -2
    assert run([0, 10, 20], [[0, 5, 7], [35, -8, 11]]) == -2                      # a negative size
    assert run([0, 10, 20], [[-1, 5, 7], [35, 8, 11]]) == -2
    assert run([0, 2 ** 31, 2 ** 31 + 1], good) == -1                             # the scan order would not fit its 32 bits
    assert run([0, 10, 20], [[0, 5, 7], [35, 2 ** 16, 2 ** 16]]) == -1
    assert run([0, 10, 20], [[0, 0, 7], [0, 8, 0]]) == 0                          # no pixel anywhere: nothing to do


def test_velodyne_depth_maps_refuses_what_is_not_where_the_launcher_expects_it():
    from ppeadepth import _abi, kitti_utils, ops
    points, P = torch.zeros(10, 4), torch.zeros(2, 3, 4, dtype=torch.float64)
    offsets, table = torch.tensor([0, 4, 10]), torch.tensor([[0, 5, 7], [35, 8, 11]])
    with pytest.raises(_abi.PpeaKernelError):
        ops.velodyne_depth_maps(points, offsets, P, table)                        # host tensors: there is no CPU kernel
    with pytest.raises(_abi.PpeaKernelError):
        ops.velodyne_depth_maps(points, offsets.to(torch.int32), P, table)
    with pytest.raises(_abi.PpeaKernelError):
        ops.velodyne_depth_maps(points, offsets, P, table[:1])
    with pytest.raises(_abi.PpeaKernelError):
        ops.velodyne_depth_maps(points[:, :3], offsets, P, table)
    assert kitti_utils.project_depth_maps([np.zeros((0, 4), np.float32)], [HAND_P], [HAND_SHAPE])[0].tolist() == [0.0] * 12
