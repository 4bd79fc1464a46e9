"""Writes tests/golden/kitti_gt.npz: the reference's UNMODIFIED `kitti_utils.generate_depth_map` (kitti_utils.py:50-102) run on
two small synthetic KITTI drives.

    python tools/gen_kitti_gt_golden.py [--out tests/golden/kitti_gt.npz]

Needs the reference tree (its kitti_utils.py is loaded by path when this runs; nothing of it is kept here).  The reference uses
`np.int`, which a current numpy no longer has: `np.int = int` is set HERE before the call, the reference stays untouched.  The
two calibration files and the scan are written to a temporary directory in KITTI's layout.

The fixture holds only data, per case `a` (5x7 image, 300 points) and `b` (8x11, 600 points): the text of
calib_cam_to_cam.txt / calib_velo_to_cam.txt, the [N,4] float32 scan, the reference's float64 maps for vel_depth False / True
and the projection matrix the reference computed on the way (the result of its second `np.dot`, recorded while it ran).

A toy rig with KITTI's geometry: focal length about 6 px, the velodyne 0.27 m behind the camera plane, so points with x in
[0, 0.27) pass the reference's `x >= 0` filter with a negative projected depth.  The generator asserts what makes each case
discriminating: a sub2ind key that spans two pixels, a pixel hit more than once, an in-bounds point with negative q2, and no
projected coordinate within 1e-9 of a half-integer (so no fp64 summation order can move a point across a pixel border).
"""
import argparse
import importlib.util
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ppea-depth_amd")]

CASES = {"a": (5, 7, 300, 11), "b": (8, 11, 600, 12)}          # H, W, points, seed
FOCAL = 6.0
BEHIND = 0.27                                                  # metres from the velodyne to the camera plane, along x


def _row(values):
    return " ".join("{:.12e}".format(float(v)) for v in np.asarray(values).reshape(-1))


def calibration(H, W, rs):
    """-> (calib_cam_to_cam.txt, calib_velo_to_cam.txt) of a toy drive: KITTI's keys and axes, slightly rotated."""
    def small_rotation(scale):
        a = rs.uniform(-scale, scale, 3)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        return np.eye(3) + K + K @ K / 2
    lines = ["calib_time: 09-Jan-2012 13:57:47", "corner_dist: 9.950000e-02"]
    for cam, tx in ((0, 0.0), (1, -0.54 * FOCAL), (2, 0.06 * FOCAL), (3, -0.47 * FOCAL)):
        P = np.array([[FOCAL, 0, W / 2 + 0.37, tx], [0, FOCAL, H / 2 + 0.21, 0.013 * (cam == 2)], [0, 0, 1, 0.0027 * (cam >= 2)]])
        lines.append("S_rect_0{}: {}".format(cam, _row([W, H])))
        lines.append("R_rect_0{}: {}".format(cam, _row(small_rotation(0.01))))
        lines.append("P_rect_0{}: {}".format(cam, _row(P)))
    axes = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])      # velodyne (forward, left, up) -> camera (right, down, forward)
    velo = ["calib_time: 15-Mar-2012 11:37:16",
            "R: " + _row(small_rotation(0.01) @ axes),
            "T: " + _row([-0.004, -0.076, -BEHIND]),
            "delta_f: 0.000000e+00 0.000000e+00", "delta_c: 0.000000e+00 0.000000e+00"]
    return "\n".join(lines) + "\n", "\n".join(velo) + "\n"


def scan(n, H, W, rs):
    """[n,4] float32: a tenth behind the sensor (dropped), a tenth between the sensor and the camera plane (negative q2), the
    rest 1 .. 30 m ahead; lateral ratios drawn so that about half of the points land in the image."""
    d = np.where(rs.uniform(size=n) < 0.125, rs.uniform(-BEHIND, -0.02, n), rs.uniform(1.0, 30.0, n))
    wide, tall = 1.4 * W / (2 * FOCAL), 1.4 * H / (2 * FOCAL)      # 1.4 x the half field of view on either axis
    pts = np.stack([d + BEHIND, rs.uniform(-wide, wide, n) * d, rs.uniform(-tall, tall, n) * d, rs.uniform(0, 1, n)], 1)
    behind = rs.uniform(size=n) < 0.1
    pts[behind, 0] = rs.uniform(-5.0, -0.01, int(behind.sum()))
    return pts.astype(np.float32)


def reference_module():
    from oracle import ref_harness as rh
    if not rh.reference_available():
        raise SystemExit("the reference tree is not present: this generator runs in the build container only")
    path = os.path.join(rh.REFERENCE_ROOT, "ppeadepth", "kitti_utils.py")
    spec = importlib.util.spec_from_file_location("_reference_kitti_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(ref, cam2cam, velo2cam, points):
    """-> (depth float64 for vel_depth False, for True, the reference's own P [3,4])."""
    np.int = int                                               # removed in numpy 1.24; the reference still says np.int
    recorded = []
    dot = np.dot

    def recording_dot(*a, **k):
        out = dot(*a, **k)
        recorded.append(out)
        return out
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "calib_cam_to_cam.txt"), "w") as f:
            f.write(cam2cam)
        with open(os.path.join(tmp, "calib_velo_to_cam.txt"), "w") as f:
            f.write(velo2cam)
        velo = os.path.join(tmp, "0000000000.bin")
        points.tofile(velo)
        np.dot = recording_dot
        try:
            plain = ref.generate_depth_map(tmp, velo, 2, False)
        finally:
            np.dot = dot
        with_x = ref.generate_depth_map(tmp, velo, 2, True)
    P = recorded[1]
    assert P.shape == (3, 4) and P.dtype == np.float64
    return plain, with_x, P.copy()


def check_case(name, H, W, points, P):
    """The properties the tests lean on, from a projection of our own (fp64, as the reference's)."""
    p = points[points[:, 0] >= 0].astype(np.float64)
    p[:, 3] = 1.0
    q = p @ P.T
    with np.errstate(divide="ignore", invalid="ignore"):
        c = q[:, :2] / q[:, 2:3]
    near = np.isfinite(c).all(1) & (np.abs(c) < 1e6).all(1)
    frac = np.abs(c[near] - np.floor(c[near]) - 0.5)
    margin = float(frac.min())
    assert margin > 1e-9, (name, margin)
    u, v = np.rint(c[:, 0]) - 1, np.rint(c[:, 1]) - 1
    ok = (u >= 0) & (v >= 0) & (u < W) & (v < H)
    u, v, q2 = u[ok].astype(int), v[ok].astype(int), q[ok, 2]
    assert 0.35 < ok.mean() < 0.65, (name, ok.mean())
    pix = v * W + u
    key = v * (W - 1) + u - 1
    spanning = sum(len(set(pix[key == k])) > 1 for k in set(key))
    assert spanning >= 1, name
    assert len(pix) > len(set(pix)), name
    assert (q2 < 0).any(), name
    print(f"case {name}: {H}x{W}, {len(points)} points, {int(ok.sum())} in bounds, {spanning} keys spanning two pixels, "
          f"{int((q2 < 0).sum())} in-bounds points with q2 < 0, half-integer margin {margin:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kitti_gt.npz"))
    args = ap.parse_args()
    ref = reference_module()
    out = {}
    for name, (H, W, n, seed) in CASES.items():
        rs = np.random.RandomState(seed)
        cam2cam, velo2cam = calibration(H, W, rs)
        points = scan(n, H, W, rs)
        plain, with_x, P = run_reference(ref, cam2cam, velo2cam, points)
        assert plain.shape == with_x.shape == (H, W) and plain.dtype == np.float64
        check_case(name, H, W, points, P)
        assert (plain == 0).any() and (with_x > 0).any()
        out.update({f"{name}:cam2cam": np.array(cam2cam), f"{name}:velo2cam": np.array(velo2cam), f"{name}:points": points,
                    f"{name}:depth": plain, f"{name}:depth_vel": with_x, f"{name}:P": P})
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    assert size < 200 * 1024, size
    print(f"wrote {args.out}: {size} bytes")


if __name__ == "__main__":
    main()
