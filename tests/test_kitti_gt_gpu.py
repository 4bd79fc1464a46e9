"""KITTI ground truth from raw LiDAR on the device (csrc/kitti_gt.hip through `ops.velodyne_depth_maps`): against the
reference's maps (tests/golden/kitti_gt.npz), the hand-built 3x4 image of test_kitti_gt_cpu.py, and the host path on a ragged
batch.

The comparison rule.  With `vel_depth=True` the depth is the point's own float32 x: the maps are EXACT.  With `vel_depth=False`
the depth is q2, an fp64 dot product of four terms that differs by a few fp64 ulps between summation orders (numpy's BLAS, the
kernel's fma chain); the cast to float32 can turn that into at most ONE float32 ulp, and the zero pattern is identical.  Pixel
coordinates could differ only if a projected coordinate sat within those few fp64 ulps of a half-integer: the golden's margin
is 1e-3 (asserted by its generator), a random scan's margin is computed here and the scan redrawn below 1e-9 -- a condition on
the input, not a tolerance."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_kitti_gt_cpu import HAND_P, HAND_SCANS, HAND_SHAPE, HAND_WANT

pytestmark = pytest.mark.gpu

KITTI_SHAPE = (375, 1242)


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(GOLDEN, "kitti_gt.npz")) as z:
        return {k: z[k] for k in z.files}


def kitti_matrix():
    """velodyne -> image 2 of a KITTI-like rig (focal length 721.5 px, velodyne 0.27 m behind the camera plane)."""
    P_rect = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
    R_rect = np.eye(4)
    R_rect[:3, :3] = [[0.9999239, 0.00983776, -0.00744505], [-0.0098698, 0.9999421, -0.00427846], [0.00740253, 0.00435161, 0.9999631]]
    velo2cam = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                         [0.9998621, 0.00752379, 0.01480755, -0.2717806], [0, 0, 0, 1]])
    return P_rect @ R_rect @ velo2cam


def half_integer_margin(points, P):
    p = points[points[:, 0] >= 0].astype(np.float64)
    p[:, 3] = 1.0
    q = p @ P.T
    with np.errstate(divide="ignore", invalid="ignore"):
        c = q[:, :2] / q[:, 2:3]
    c = c[np.isfinite(c).all(1) & (np.abs(c) < 1e6).all(1)]
    return float(np.abs(c - np.floor(c) - 0.5).min())


def random_scan(n, P, shape, seed, focal, spread=1.2, near=0.05):
    """[n,4] float32 around the field of view of `shape` (about half in bounds), some behind the sensor, a share `near` between
    the sensor and the camera plane (negative q2); redrawn with the next seed while a projected coordinate lies within 1e-9 of a
    half-integer."""
    while True:
        rs = np.random.RandomState(seed)
        d = np.where(rs.uniform(size=n) < near, rs.uniform(-0.27, -0.02, n), rs.uniform(2.0, 80.0, n))
        wide, tall = spread * shape[1] / (2 * focal), spread * shape[0] / (2 * focal)
        pts = np.stack([d + 0.27, rs.uniform(-wide, wide, n) * d, rs.uniform(-tall, tall, n) * d, rs.uniform(0, 1, n)], 1)
        behind = rs.uniform(size=n) < 0.05
        pts[behind, 0] = rs.uniform(-5.0, -0.01, int(behind.sum()))
        pts = pts.astype(np.float32)
        if half_integer_margin(pts, P) >= 1e-9:
            return pts
        seed += 1


def host_maps(clouds, matrices, shapes, vel_depth):
    from ppeadepth import kitti_utils
    return [kitti_utils.depth_map_from_points(c, P, s, vel_depth).astype(np.float32) for c, P, s in zip(clouds, matrices, shapes)]


def device_maps(clouds, matrices, shapes, vel_depth, device):
    from ppeadepth import kitti_utils
    flat, table, _ = kitti_utils.project_depth_maps(clouds, matrices, shapes, vel_depth, device)
    assert flat.is_cuda and flat.dtype == torch.float32 and table.is_cuda
    flat = flat.cpu().numpy()
    return [flat[off:off + h * w].reshape(h, w) for off, h, w in table.tolist()]


def assert_maps_agree(got, want, exact):
    """exact: equal values; else the same zero pattern and every value within one float32 ulp (module docstring)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    if exact:
        assert np.array_equal(got, want)
        return
    hit = want != 0
    assert np.array_equal(got != 0, hit)
    ulps = np.abs(got[hit].view(np.int32).astype(np.int64) - want[hit].view(np.int32).astype(np.int64))
    assert ulps.size == 0 or int(ulps.max()) <= 1, int(ulps.max())


@pytest.fixture(scope="module")
def big():
    """Two 375x1242 frames of 20 000 points and their matrix, shared by the tests that need a full-size image."""
    P = kitti_matrix()
    return P, [random_scan(20000, P, KITTI_SHAPE, seed, 721.5377) for seed in (0, 100)]


@pytest.mark.parametrize("vel_depth", [False, True])
@pytest.mark.parametrize("case", ["a", "b"])
def test_kernel_against_the_reference_maps(fixture, device, case, vel_depth):
    want = fixture[f"{case}:depth_vel" if vel_depth else f"{case}:depth"]
    got, = device_maps([fixture[f"{case}:points"]], [fixture[f"{case}:P"]], [want.shape], vel_depth, device)
    assert_maps_agree(got, want.astype(np.float32), exact=vel_depth)


@pytest.mark.parametrize("vel_depth", [False, True])
def test_kernel_on_the_hand_built_image_is_exact(device, vel_depth):
    """Every number of these scans is a small multiple of 1/4: q2 is exact in either summation order, so both modes are exact.
    One launch for the three scans."""
    names = sorted(HAND_SCANS)
    got = device_maps([HAND_SCANS[n] for n in names], [HAND_P] * 3, [HAND_SHAPE] * 3, vel_depth, device)
    for n, g in zip(names, got):
        assert np.array_equal(g, np.array(HAND_WANT[n, vel_depth], dtype=np.float32)), n


@pytest.mark.parametrize("vel_depth", [False, True])
def test_ragged_batch_in_one_launch(fixture, device, big, vel_depth):
    P_big, scans = big
    clouds = [fixture["a:points"], np.zeros((0, 4), np.float32), scans[0]]
    matrices = [fixture["a:P"], fixture["b:P"], P_big]
    shapes = [(5, 7), (8, 11), KITTI_SHAPE]
    want = host_maps(clouds, matrices, shapes, vel_depth)
    got = device_maps(clouds, matrices, shapes, vel_depth, device)
    assert not want[1].any() and not got[1].any()                                 # the empty scan: an all-zero map
    hit = int((want[2] != 0).sum())
    assert 5000 < hit < 20000                                                     # a populated full-size map with duplicates
    for g, w in zip(got, want):
        assert_maps_agree(g, w, exact=vel_depth)


def test_two_launches_give_the_same_bytes(fixture, device):
    """Every pixel of a 5x7 image is hit hundreds of times: whatever order the atomics land in, the bytes are the same, and
    they are the host path's."""
    from ppeadepth import kitti_utils
    P = fixture["a:P"]
    scan = random_scan(20000, P, (5, 7), 3, 6.0, spread=0.9, near=0.0)     # no negative depth: no pixel clamps to 0
    for vel_depth in (True, False):
        runs = [kitti_utils.project_depth_maps([scan], [P], [(5, 7)], vel_depth, device)[0] for _ in range(2)]
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
        want, = host_maps([scan], [P], [(5, 7)], vel_depth)
        assert (want != 0).all()
        assert_maps_agree(runs[0].cpu().numpy().reshape(5, 7), want, exact=vel_depth)


def test_from_velodyne_scores_like_uploaded_ground_truth(device, big):
    """Same ground-truth bytes in, same errors out: `DeviceGroundTruth.from_velodyne` against the host path's maps uploaded."""
    from ppeadepth import evaluate
    P, scans = big
    gt = evaluate.DeviceGroundTruth.from_velodyne(scans, [P, P], [KITTI_SHAPE] * 2, device)
    ref = evaluate.DeviceGroundTruth(host_maps(scans, [P, P], [KITTI_SHAPE] * 2, True), device)
    assert len(gt) == 2 and gt.shapes == ref.shapes and torch.equal(gt.table, ref.table)
    assert torch.equal(gt.flat.view(torch.int32), ref.flat.view(torch.int32))
    pred = torch.rand(2, 96, 320, generator=torch.Generator().manual_seed(0)).mul(0.3).add(0.02).to(device)
    got, want = gt.score(pred, 0, "eigen"), ref.score(pred, 0, "eigen")
    assert int(want[2].min()) > 1000                                              # scored pixels in the Eigen crop
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)


def test_launcher_refusals(device):
    from ppeadepth import _abi, ops
    points = torch.zeros(10, 4, device=device)
    P = torch.zeros(2, 3, 4, dtype=torch.float64, device=device)
    table = torch.tensor([[0, 5, 7], [35, 8, 11]])
    with pytest.raises(_abi.PpeaKernelError, match="inconsistent arguments"):     # B = 0
        ops.velodyne_depth_maps(points, torch.tensor([0]), P[:0], table[:0])
    with pytest.raises(_abi.PpeaKernelError, match="inconsistent arguments"):     # descending offsets
        ops.velodyne_depth_maps(points, torch.tensor([0, 10, 5]), P, table)
    with pytest.raises(_abi.PpeaKernelError, match="float64"):
        ops.velodyne_depth_maps(points, torch.tensor([0, 4, 10]), P.float(), table)
    with pytest.raises(_abi.PpeaKernelError, match="holds 10 points"):            # offsets past the buffer
        ops.velodyne_depth_maps(points, torch.tensor([0, 4, 11]), P, table)
    with pytest.raises(_abi.PpeaKernelError, match="on the host"):                # the launcher reads the table itself
        ops.velodyne_depth_maps(points, torch.tensor([0, 4, 10]), P, table.to(device))
    out = ops.velodyne_depth_maps(points, torch.tensor([0, 4, 10]), P, table)     # all-zero P: q2 = 0, no valid point
    assert out.shape == (35 + 88,) and not out.any()
