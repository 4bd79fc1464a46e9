"""Shared by tests/test_points_cpu.py and tests/test_points_gpu.py: the float64 restatement of the point-cloud rule
(include/ppea_depth.h, "Point clouds") on the fp32 inputs, the set of pixels whose decision float64 and fp32 may take
differently, the seeded inputs and the comparison."""
import numpy as np

import export_oracle as eo

SRC, RAGGED = eo.SRC, eo.RAGGED
LO, HI = 12.0, 60.0                 # the scenes' depth is 6 .. 90 times 1.7 / scale: both ends cut
SLACK = 2e-5                        # twice eo.RTOL, the relative bound the export tests hold the depth to
CAP = 0.02                          # largest share of undecided candidates (the export tests' cap)
CHAIN = 1e-6                        # pose chain: per step and per unit of the largest absolute row sum
_scenes = {}


def planes(B, hw=SRC):
    """[B,h,w] fp32 scaled disparity, built once per shape and never modified."""
    key = (B,) + tuple(hw)
    if key not in _scenes:
        _scenes[key] = np.stack([eo.scene(11 + b, *hw) for b in range(B)])
    return _scenes[key]


def inv_K(sizes, seed=5, centred=True):
    """[B,4,4] fp32: the inverse of KITTI's intrinsics at each size, every entry of the upper-left 3x3 made non-zero.
    centred=False: the principal point lies a quarter of the image outside it (the intrinsics of an off-centre crop), so
    that no ray component passes through zero inside the image.  The coordinate bound is relative to |c_i| alone when there
    is no pose, and at a pixel on the principal point's row or column ray_i = (k_i0 u + k_i1 v) + k_i2 cancels to the
    rounding error of its own terms (6e-8 of 0.86 against a ray of 0 .. 3e-3): no fp32 evaluation in the prescribed order
    can meet a bound relative to the result there, so the cases without a pose use centred=False.  With a pose the bound
    carries |t_i| and the other components, and the centred intrinsics are used."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(sizes), 4, 4), np.float32)
    c = 0.5 if centred else -0.25
    for b, (H, W) in enumerate(sizes):
        K = np.eye(4)
        K[0, 0], K[0, 2], K[1, 1], K[1, 2] = 0.58 * W, c * W, 1.92 * H, c * H
        inv = np.linalg.inv(K)
        inv[:3, :3] += rng.normal(0, 1e-4, (3, 3))
        out[b] = inv
    return out


def poses(B, seed=6):
    """[B,4,4] fp32 camera-to-world: a rotation of about 0.3 rad and a translation of a few metres."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, 4, 4), np.float32)
    for b in range(B):
        a = rng.normal(0, 0.2, 3)
        A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        th = np.linalg.norm(a)
        R = np.eye(3) + np.sin(th) / th * A + (1 - np.cos(th)) / th ** 2 * A @ A
        out[b, :3, :3], out[b, :3, 3], out[b, 3, 3] = R, rng.normal(0, 3, 3), 1
    return out


def colours(sizes, seed=7):
    """(flat uint8 buffer of the HWC frames back to back, byte offsets [B])."""
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in sizes]
    offs = np.cumsum([0] + [f.size for f in frames])[:-1]
    return np.concatenate([f.reshape(-1) for f in frames]), offs.astype(np.int64)


class Image:
    """The rule for one image in float64: cand, keep, undecided [H,W] bool; d [H,W]; point and bound [H,W,3]."""

    def __init__(self, disp, size, inv_k, pose=None, scale=1.0, lo=LO, hi=HI, stride=1, edge=0.0, mode="disp"):
        H, W = size
        lo, hi, edge = (np.float64(np.float32(v)) for v in (lo, hi, edge))
        d = eo.depth_f64(disp, size, scale, -np.inf, np.inf, mode)
        self.d = d
        cand = np.zeros((H, W), bool)
        cand[::stride, ::stride] = True
        with np.errstate(invalid="ignore", over="ignore"):
            keep = cand & (d > lo) & (d < hi)
            und = (np.abs(d - lo) <= SLACK * d) | (np.abs(d - hi) <= SLACK * d)
            if edge > 0:
                for sl, nb in (((slice(None), slice(1, None)), (slice(None), slice(None, -1))),
                               ((slice(None), slice(None, -1)), (slice(None), slice(1, None))),
                               ((slice(1, None), slice(None)), (slice(None, -1), slice(None))),
                               ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
                    diff = np.abs(d[nb] - d[sl])
                    keep[sl] &= ~(diff > edge * d[sl])
                    und[sl] |= np.abs(diff - edge * d[sl]) <= SLACK * (np.abs(d[nb]) + 2 * d[sl])
        self.cand, self.keep, self.undecided = cand, keep, und & cand
        v, u = np.mgrid[0:H, 0:W].astype(np.float64)
        k = inv_k.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.stack([(k[i, 0] * u + k[i, 1] * v + k[i, 2]) * d for i in range(3)], -1)
            m = np.eye(4) if pose is None else pose.astype(np.float64)
            self.point = c @ m[:3, :3].T + m[:3, 3]
            self.bound = SLACK * (np.abs(c) @ np.abs(m[:3, :3]).T + np.abs(m[:3, 3]))


def undecided_share(images, what):
    """Asserted on the oracle's side, over the whole batch of a case, before any result is looked at."""
    share = sum(int(im.undecided.sum()) for im in images) / max(sum(int(im.cand.sum()) for im in images), 1)
    kept = sum(int(im.keep.sum()) for im in images) / max(sum(int(im.cand.sum()) for im in images), 1)
    print(f"{what}: {share:.2%} of the candidates undecided, {kept:.1%} kept")
    assert share < CAP, what
    return share


def check_image(im, xyz, index, offset, what, exact=False):
    """The points of ONE image (index still global) against the oracle -> the largest |p - ref| / bound."""
    H, W = im.cand.shape
    local = np.asarray(index, np.int64) - offset
    assert ((local >= 0) & (local < H * W)).all(), what
    assert (np.diff(local) > 0).all(), what                                   # raster order, no pixel twice
    got = np.zeros(H * W, bool)
    got[local] = True
    got = got.reshape(H, W)
    assert not (got & ~im.cand).any(), what
    if exact:
        assert not im.undecided.any(), what
    sure = im.cand & ~im.undecided
    assert (got == im.keep)[sure].all(), (what, int((got != im.keep)[sure].sum()))
    if not len(local):
        return 0.0
    ref, bound = im.point.reshape(-1, 3)[local], im.bound.reshape(-1, 3)[local]
    err = np.abs(np.asarray(xyz, np.float64) - ref)
    assert (err <= bound).all(), (what, float((err / bound).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


def check_batch(images, xyz, index, counts, rows, what, exact=False):
    """A whole call: images in order, `counts` the per-image split; rows = the (offset, H, W) table."""
    counts = [int(c) for c in counts]
    assert sum(counts) == len(index) == len(xyz), what
    worst, at = 0.0, 0
    for b, im in enumerate(images):
        worst = max(worst, check_image(im, xyz[at:at + counts[b]], index[at:at + counts[b]], rows[b][0], f"{what} image {b}",
                                       exact))
        at += counts[b]
    return worst


def chain_f64(pose_list, present_list):
    """The float64 product of the same fp32 poses: per push (pose [B,F,4,4], present [B,F]) -> world [B,4,4] after it."""
    B = pose_list[0].shape[0]
    world, out = np.tile(np.eye(4), (B, 1, 1)), []
    for pose, present in zip(pose_list, present_list):
        for b in range(B):
            world[b] = world[b] @ pose[b, 0].astype(np.float64) if present[b, 0] else np.eye(4)
        out.append(world.copy())
    return out


def chain_bound(ref, n):
    return n * CHAIN * max(1.0, float(np.abs(ref).sum(-1).max()))
