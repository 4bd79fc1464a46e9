"""Host side of the point clouds (no GPU): the ABI of the entry points, the numpy statement `evaluate.export_points` (what a
device="cpu" predictor runs) against the float64 rule of tests/points_oracle.py, the PLY writer and reader, the CPU
`DepthPredictor.points`, `StreamMap` and `full_inv_K`, and the CLI's flags."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from oracle import synth

import points_oracle as po

NEW_SYMBOLS = {"ppea_point_cloud_workspace_bytes": 3, "ppea_point_cloud_f32": 25, "ppea_pose_accumulate_f32": 6}
H, W, B = 64, 96, 2
_cache = {}


def test_points_abi():
    from ppeadepth import _abi
    assert _abi.lib.ppea_abi_version() == _abi.ABI_VERSION >= 32
    header = open(os.path.join(ROOT, "include", "ppea_depth.h")).read()
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^(?:int|long)\s+(ppea_\w+)\s*\(([^;]*)\)\s*;", header, flags=re.M)}
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared, name
        assert len(declared[name].split(",")) == nargs, name
        assert len(_abi.SIGNATURES[name]) == nargs and hasattr(_abi.lib, name), name
    assert "point_cloud.hip" in open(os.path.join(ROOT, "ppea-depth_amd", "csrc", "Makefile")).read()


def test_ops_refuse_host_tensors():
    from ppeadepth import _abi, ops
    eye = torch.eye(4).repeat(1, 1, 1)
    with pytest.raises(_abi.PpeaKernelError):
        ops.point_cloud(torch.rand(1, 4, 6), (8, 12), eye)
    with pytest.raises(_abi.PpeaKernelError):
        ops.pose_accumulate(eye.clone(), eye[:, None].clone(), torch.ones(1, 1, dtype=torch.bool))


@pytest.mark.parametrize("mode", ["disp", "depth"])
@pytest.mark.parametrize("edge", [0.0, 0.05, 0.1, 0.2])
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_export_points_against_float64(stride, edge, mode):
    from ppeadepth.evaluate import export_points
    sizes = po.RAGGED
    disp, pose = po.planes(len(sizes)), po.poses(len(sizes))
    buf, offs = po.colours(sizes)
    for with_pose in (True, False):
        ik = po.inv_K(sizes, centred=with_pose)
        images = [po.Image(disp[b], sizes[b], ik[b], pose[b] if with_pose else None, 1.0 + 0.25 * b, stride=stride, edge=edge,
                           mode=mode) for b in range(len(sizes))]
        po.undecided_share(images, f"stride {stride} edge {edge} {mode}")
        worst, off, kept = 0.0, 0, 0
        for b, (Ht, Wt) in enumerate(sizes):
            frame = buf[offs[b]:offs[b] + Ht * Wt * 3].reshape(Ht, Wt, 3)
            xyz, rgb, index = export_points(disp[b], sizes[b], ik[b], frame, pose[b] if with_pose else None, 1.0 + 0.25 * b,
                                            po.LO, po.HI, stride, edge, mode, offset=off)
            assert xyz.dtype == np.float32 and rgb.dtype == np.uint8 and index.dtype == np.int64
            worst = max(worst, po.check_image(images[b], xyz, index, off, f"image {b}"))
            assert np.array_equal(rgb, frame.reshape(-1, 3)[index - off])
            kept += len(index)
            off += Ht * Wt
        assert 0 < kept < sum(int(im.cand.sum()) for im in images)            # the case cuts, and not everything
        print(f"stride {stride} edge {edge} {mode} pose {with_pose}: largest |p - ref| / bound {worst:.3f}")


def test_export_points_float_colour():
    from ppeadepth.evaluate import export_points
    size = po.RAGGED[0]
    rng = np.random.default_rng(2)
    col = rng.random((3,) + size, dtype=np.float32) * 1.2 - 0.1               # some values outside [0, 1]
    xyz, rgb, index = export_points(po.planes(1)[0], size, po.inv_K([size])[0], col, stride=2, lo=po.LO, hi=po.HI)
    want = np.clip(np.round(col.astype(np.float64) * 255), 0, 255).reshape(3, -1)[:, index].T
    t = col.astype(np.float64).reshape(3, -1)[:, index].T * 255
    near_half = np.abs(t - np.floor(t) - 0.5) < 1e-4                          # fp32 product vs float64 at a rounding tie
    assert len(index) and (rgb.astype(np.int64) == want)[~near_half].all() and near_half.mean() < 0.01
    assert rgb.min() == 0 and rgb.max() == 255


def test_ply_round_trip(tmp_path):
    from ppeadepth import vis
    rng = np.random.default_rng(1)
    xyz = rng.normal(0, 10, (37, 3)).astype(np.float32)
    xyz[3, 1], xyz[4, 2] = np.float32("inf"), -0.0
    rgb = rng.integers(0, 256, (37, 3), dtype=np.uint8)
    for n in (37, 0):
        for colour in (True, False):
            path = str(tmp_path / f"{n}_{colour}.ply")
            vis.write_ply(path, xyz[:n], rgb[:n] if colour else None)
            raw = open(path, "rb").read()
            lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}", "property float x", "property float y",
                     "property float z"] + (["property uchar red", "property uchar green", "property uchar blue"] if colour
                                            else []) + ["end_header"]
            head = ("\n".join(lines) + "\n").encode("ascii")
            assert raw.startswith(head) and len(raw) - len(head) == n * (15 if colour else 12)
            got_xyz, got_rgb = vis.read_ply(path)
            assert got_xyz.dtype == np.float32 and got_xyz.tobytes() == xyz[:n].tobytes() and got_xyz.shape == (n, 3)
            assert (got_rgb is None) == (not colour)
            if colour:
                assert got_rgb.dtype == np.uint8 and np.array_equal(got_rgb, rgb[:n])
    with pytest.raises(ValueError):
        vis.write_ply(str(tmp_path / "bad.ply"), xyz, rgb[:5])
    with pytest.raises(ValueError):
        vis.write_ply(str(tmp_path / "bad.ply"), xyz[:, :2])
    # torch tensors are taken as they are
    vis.write_ply(str(tmp_path / "t.ply"), torch.from_numpy(xyz), torch.from_numpy(rgb))
    assert vis.read_ply(str(tmp_path / "t.ply"))[0].tobytes() == xyz.tobytes()


def _predictor():
    if not _cache:
        from ppeadepth import networks, options
        from ppeadepth.inference import DepthPredictor
        opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False)
        torch.manual_seed(0)
        model = networks.RepDepth(opt)
        synth.fill_state_dict(model, conditioned=True)
        model.train()
        _cache["p"] = DepthPredictor(model, opt, device="cpu")
    return _cache["p"]


def test_cpu_predictor_points_is_export_points():
    from ppeadepth.evaluate import export_points
    from ppeadepth.layers import disp_to_depth
    p = _predictor()
    sizes = po.RAGGED
    n = len(sizes)
    # a network's disparity in (0, 1) whose scaled depth covers the range 12 .. 60
    depth = 1 / po.planes(n)
    disp = torch.from_numpy(((1 / depth - 1 / 100.0) / (1 / 0.1 - 1 / 100.0)).astype(np.float32))[:, None]
    scaled = disp_to_depth(disp, 0.1, 100.0)[0][:, 0].numpy()
    ik, pose = torch.from_numpy(po.inv_K(sizes)), torch.from_numpy(po.poses(n))
    buf, offs = po.colours(sizes)
    cloud = p.points(disp, sizes, ik, torch.from_numpy(buf), torch.from_numpy(offs), pose, lo=po.LO, hi=po.HI, stride=2, edge=0.1,
                     min_depth=0.1, max_depth=100.0)
    xyz, rgb, index, dropped = cloud.trim()
    assert dropped == 0 and cloud.xyz.shape[0] == sum(((h + 1) // 2) * ((w + 1) // 2) for h, w in sizes)
    at = off = 0
    for b, (Ht, Wt) in enumerate(sizes):
        want = export_points(scaled[b], sizes[b], ik[b].numpy(), buf[offs[b]:offs[b] + Ht * Wt * 3].reshape(Ht, Wt, 3),
                             pose[b].numpy(), 1.0, po.LO, po.HI, 2, 0.1, "disp", off)
        k = len(want[2])
        assert k > 0 and int(cloud.counts[b]) == k
        assert xyz[at:at + k].numpy().tobytes() == want[0].tobytes() and np.array_equal(rgb[at:at + k].numpy(), want[1])
        assert np.array_equal(index[at:at + k].numpy(), want[2])
        at, off = at + k, off + Ht * Wt
    assert at == len(index)
    # a capacity below the total: the first points, and the count of the rest
    small = p.points(disp, sizes, ik, pose=pose, lo=po.LO, hi=po.HI, stride=2, edge=0.1, min_depth=0.1, max_depth=100.0,
                     capacity=10)
    assert small.cursor.tolist() == [10, at - 10] and torch.equal(small.xyz, xyz[:10]) and small.rgb is None


def test_cpu_stream_map_chain():
    p = _predictor()
    s = p.stream(B)
    m = s.map(capacity=4096, stride=4, edge=0.1, lo=0.5, hi=80.0)
    eye = torch.eye(4).repeat(B, 1, 1)
    assert torch.equal(m.world, eye) and m.cloud().cursor.tolist() == [0, 0]
    rng = np.random.default_rng(9)
    g = torch.Generator().manual_seed(4)
    ik = p.full_inv_K(np.array([[0.58, 0, 0.5], [0, 1.92, 0.5], [0, 0, 1]]), [(H, W)] * B)
    poses, presents, since = [], [], np.zeros(B, int)
    for t in range(6):
        pose = np.stack([po.poses(1, seed=100 + 7 * t + b) for b in range(B)]).astype(np.float32)       # [B,1,4,4]
        pose[:, 0, :3, 3] *= 0.1
        present = np.array([[t > 0], [t > 0 and t != 3]])                     # camera 1 is reset before push 3
        poses.append(pose), presents.append(present)
        smooth = 0.05 + 0.3 * torch.linspace(0, 1, H)[None, None, :, None] * torch.linspace(0.5, 1, W) + 0.01 * t
        out = {"disp": smooth.repeat(B, 1, 1, 1), "pose": torch.from_numpy(pose),
               "present": torch.from_numpy(present)}
        held = m.cloud().cursor.tolist()[0]
        m.add(out, torch.rand(B, 3, H, W, generator=g), ik)
        assert m.cloud().cursor.tolist()[0] > held
        ref = po.chain_f64(poses, presents)[-1]
        since = np.where(present[:, 0], since + 1, 0)
        for b in range(B):
            if since[b] == 0:
                assert torch.equal(m.world[b], torch.eye(4)), (t, b)
            else:
                err = np.abs(m.world[b].numpy().astype(np.float64) - ref[b]).max()
                assert err <= po.chain_bound(ref[b], since[b]), (t, b, err)
    assert since.tolist() == [5, 2]
    m.clear()
    assert torch.equal(m.world, eye) and m.cloud().cursor.tolist() == [0, 0]


def test_full_inv_K_against_float64():
    p = _predictor()
    K3 = np.array([[0.58, 0.001, 0.5], [0, 1.92, 0.5], [0, 0, 1]])
    K4 = np.eye(4)
    K4[:3, :3] = K3
    sizes = [(375, 1242), (370, 1226)]
    for K in (K3, K4, torch.from_numpy(K4).float(), np.stack([K3, K3 * [[1.1], [0.9], [1]]])):
        got = p.full_inv_K(K, sizes)
        assert tuple(got.shape) == (2, 4, 4) and got.dtype == torch.float32
        Kn = np.asarray(K, np.float64)
        for b, (Ht, Wt) in enumerate(sizes):
            full = np.eye(4)
            k = Kn[b] if Kn.ndim == 3 else Kn
            full[:k.shape[0], :k.shape[1]] = k
            full[0] *= Wt
            full[1] *= Ht
            assert np.array_equal(got[b].numpy(), np.linalg.inv(full).astype(np.float32))
            assert np.allclose(got[b].numpy().astype(np.float64) @ full, np.eye(4), atol=1e-4)
    assert tuple(p.full_inv_K(K3, (375, 1242)).shape) == (1, 4, 4)


def test_predict_parser_knows_ply(monkeypatch):
    from ppeadepth import predict
    args, rest = predict._parser().parse_known_args(["--data_path", "d", "--split_file", "s", "--out", "o", "--ply",
                                                     "--ply_stride", "2", "--ply_edge", "0.1"])
    assert args.ply and args.ply_stride == 2 and args.ply_edge == 0.1 and not rest
    # --ply alone is something to write: the run gets past that check, to the construction of the model
    from ppeadepth import networks

    class Reached(Exception):
        pass

    def stop(opt):
        raise Reached()
    monkeypatch.setattr(networks, "RepDepth", stop)
    common = ["--data_path", "d", "--split_file", "s", "--out", "o", "--load_weights_folder", "w", "--device", "cpu"]
    with pytest.raises(Reached):
        predict.main(common + ["--ply"])
    with pytest.raises(SystemExit, match="nothing to write"):
        predict.main(common)
