"""Point clouds on the GPU (csrc/point_cloud.hip through ops.point_cloud / pose_accumulate, DepthPredictor.points,
DepthStream.map, python -m ppeadepth.predict --ply) against the float64 rule of tests/points_oracle.py.

Source planes are 24 x 80 with targets (47, 157), (24, 80), (12, 41) as one ragged batch and alone; planted planes at
identity size, (1, 1), (1, 4097), (3, 1025), (64, 65) and five images of (3, 1025), cross every plausible chunk and wave
edge; the largest |p - ref| / bound of each case is printed."""
import os

import numpy as np
import pytest
import torch

from oracle import synth

import points_oracle as po

pytestmark = pytest.mark.gpu

INF = float("inf")
_oracles = {}


def _image(b, size, centred, with_pose, scale, stride, edge, mode):
    """The float64 rule for scene b at `size`, computed once per argument set."""
    key = (b, size, centred, with_pose, scale, stride, edge, mode)
    if key not in _oracles:
        ik = po.inv_K([size], seed=5 + b, centred=centred)[0]
        _oracles[key] = po.Image(po.planes(3)[b], size, ik, po.poses(1, seed=6 + b)[0] if with_pose else None, scale,
                                 stride=stride, edge=edge, mode=mode)
    return _oracles[key]


def _host(cloud):
    xyz, rgb, index, dropped = cloud.trim()
    return xyz.cpu().numpy(), None if rgb is None else rgb.cpu().numpy(), index.cpu().numpy(), dropped


def _rows(sizes):
    rows, off = [], 0
    for h, w in sizes:
        rows.append((off, h, w))
        off += h * w
    return rows


CASES = {"ragged": [0, 1, 2], "alone0": [0], "alone1": [1], "alone2": [2]}
# (pose, colour, per-image scale): each value of each with each value of the others at least once
COMBOS = ((True, True, False), (False, False, True), (True, False, True), (False, True, False))


@pytest.mark.parametrize("mode", ["disp", "depth"])
@pytest.mark.parametrize("case", list(CASES))
def test_ragged_against_float64(device, case, mode):
    from ppeadepth import ops
    which = CASES[case]
    sizes = [po.RAGGED[b] for b in which]
    rows = _rows(sizes)
    pred = torch.from_numpy(po.planes(3)[which]).to(device)
    buf, offs = po.colours(sizes)
    colour, colour_off = torch.from_numpy(buf).to(device), torch.from_numpy(offs).to(device)
    worst = 0.0
    for stride in (1, 2, 3):
        for edge in (0.0, 0.05, 0.2):
            for with_pose, with_colour, per_image in COMBOS:
                scales = [1.0 + 0.25 * b if per_image else 1.0 for b in which]
                images = [_image(b, po.RAGGED[b], with_pose, with_pose, sc, stride, edge, mode)
                          for b, sc in zip(which, scales)]
                what = f"{case} {mode} stride {stride} edge {edge} pose {with_pose} colour {with_colour} scales {per_image}"
                po.undecided_share(images, what)                              # before the device result is looked at
                ik = torch.from_numpy(np.stack([po.inv_K([po.RAGGED[b]], seed=5 + b, centred=with_pose)[0] for b in which]))
                pose = torch.from_numpy(np.stack([po.poses(1, seed=6 + b)[0] for b in which])).to(device) if with_pose else None
                cloud = ops.point_cloud(pred, sizes, ik.to(device), pose, colour if with_colour else None,
                                        colour_off if with_colour else None,
                                        torch.tensor(scales, dtype=torch.float32, device=device) if per_image else 1.0,
                                        po.LO, po.HI, stride, edge, mode)
                xyz, rgb, index, dropped = _host(cloud)
                assert dropped == 0 and cloud.xyz.shape[0] == sum(int(im.cand.sum()) for im in images)
                counts = cloud.counts.cpu().tolist()
                worst = max(worst, po.check_batch(images, xyz, index, counts, rows, what))
                assert (rgb is None) == (not with_colour)
                if with_colour:
                    assert np.array_equal(rgb, buf.reshape(-1, 3)[index])     # frames back to back: byte 3 * index
    print(f"{case} {mode}: largest |p - ref| / bound {worst:.3f}")


def test_float_colour_and_default_offsets(device):
    from ppeadepth import ops
    size = po.RAGGED[0]
    pred = torch.from_numpy(po.planes(3)[:2]).to(device)
    ik = torch.from_numpy(po.inv_K([size] * 2)).to(device)
    rng = np.random.default_rng(2)
    col = (rng.random((2, 3) + size, dtype=np.float32) * 1.2 - 0.1)
    cloud = ops.point_cloud(pred, size, ik, colour=torch.from_numpy(col).to(device), lo=po.LO, hi=po.HI, stride=2)
    xyz, rgb, index, _ = _host(cloud)
    want = np.clip(np.rint(col * np.float32(255)), 0, 255).astype(np.uint8)   # the fp32 product, as the kernel
    pix, img = index % (size[0] * size[1]), index // (size[0] * size[1])
    assert len(index) and np.array_equal(rgb, want.reshape(2, 3, -1)[img, :, pix])
    assert rgb.min() == 0 and rgb.max() == 255
    # uint8 frames without offsets are taken back to back
    buf, offs = po.colours([size] * 2)
    a = ops.point_cloud(pred, size, ik, colour=torch.from_numpy(buf).to(device), lo=po.LO, hi=po.HI, stride=2)
    assert np.array_equal(_host(a)[1], buf.reshape(-1, 3)[index]) and np.array_equal(_host(a)[0], xyz)


@pytest.mark.parametrize("mode", ["disp", "depth"])
def test_z_is_the_exported_depth_bit_for_bit(device, mode):
    from ppeadepth import ops
    sizes = po.RAGGED
    pred = torch.from_numpy(po.planes(3)).to(device)
    eye = torch.eye(4, device=device).repeat(3, 1, 1).contiguous()
    scale = torch.tensor([1.0, 1.25, 0.7], device=device)
    depth, table = ops.disp_export(pred, sizes, scale, 0.0, INF, mode)
    for pose in (eye, None):
        cloud = ops.point_cloud(pred, sizes, eye, pose, scale=scale, lo=0.0, hi=INF, edge=0.0, mode=mode)
        xyz, _, index, dropped = cloud.trim()
        assert dropped == 0
        assert torch.equal(xyz[:, 2].view(torch.int32), depth[index].view(torch.int32))
        present = torch.zeros(depth.numel(), dtype=torch.bool, device=device)
        present[index] = True
        assert torch.equal(present, torch.isfinite(depth) & (depth > 0)) and bool(present.all())
        assert torch.equal(xyz[:, 0], (index - table[:, 0].repeat_interleave(cloud.counts)).remainder(
            table[:, 2].repeat_interleave(cloud.counts)).float() * xyz[:, 2])


def _planted(shape, pattern):
    """[h,w] disparity at identity size whose depth is 30 (kept, far from 12 and 60) or 100 (dropped)."""
    h, w = shape
    v, u = np.mgrid[0:h, 0:w]
    if pattern == "all":
        keep = np.ones(shape, bool)
    elif pattern == "checker":
        keep = (u + v) % 2 == 0
    else:                                            # single kept pixels: first, last, around multiples of 64, 256 and 2048
        keep = np.zeros(h * w, bool)
        for i in (0, 63, 64, 255, 256, 1023, 1024, 2047, 2048, 2049, 4095, 4096, h * w - 1):
            if i < h * w:
                keep[i] = True
        keep = keep.reshape(shape)
    return (1 / np.where(keep, 30.0, 100.0)).astype(np.float32), keep


@pytest.mark.parametrize("shape", [(1, 1), (1, 4097), (3, 1025), (64, 65)])
def test_chunk_and_wave_edges(device, shape):
    from ppeadepth import ops
    ik = po.inv_K([shape], centred=False)
    for pattern in ("all", "none", "checker", "single"):
        disp, keep = _planted(shape, "all" if pattern == "none" else pattern)
        lo, hi = (po.HI, po.LO) if pattern == "none" else (po.LO, po.HI)
        for stride in (1, 2):
            im = po.Image(disp, shape, ik[0], lo=lo, hi=hi, stride=stride)
            assert not im.undecided.any()
            cloud = ops.point_cloud(torch.from_numpy(disp[None]).to(device), shape, torch.from_numpy(ik).to(device), lo=lo,
                                    hi=hi, stride=stride)
            xyz, _, index, dropped = _host(cloud)
            po.check_image(im, xyz, index, 0, f"{shape} {pattern} stride {stride}", exact=True)
            want = 0 if pattern == "none" else int(keep[::stride, ::stride].sum())
            assert dropped == 0 and len(index) == want == int(cloud.counts[0])


def test_a_batch_whose_third_image_keeps_nothing(device):
    from ppeadepth import ops
    shape = (3, 1025)
    patterns = ("checker", "all", "none", "single", "checker")
    planes = [_planted(shape, "all" if p == "none" else p)[0] for p in patterns]
    planes[2] = np.full(shape, 1 / 100.0, np.float32)
    ik = po.inv_K([shape] * 5, centred=False)
    images = [po.Image(planes[b], shape, ik[b]) for b in range(5)]
    assert po.undecided_share(images, "five images") == 0
    cloud = ops.point_cloud(torch.from_numpy(np.stack(planes)).to(device), shape, torch.from_numpy(ik).to(device), lo=po.LO,
                            hi=po.HI)
    xyz, _, index, _ = _host(cloud)
    counts = cloud.counts.cpu().tolist()
    assert counts[2] == 0 and counts[1] == 3 * 1025 and min(counts[0], counts[3], counts[4]) > 0
    po.check_batch(images, xyz, index, counts, _rows([shape] * 5), "five images", exact=True)


def _guarded(cap, B, device, guard=64):
    """A `PointCloud` of `cap` points between poisoned guard regions -> (cloud, the whole buffers, their poison)."""
    from ppeadepth import ops
    whole = (torch.full((cap + 2 * guard, 3), float("nan"), device=device), torch.full((cap + 2 * guard, 3), 0xA5, device=device,
             dtype=torch.uint8), torch.full((cap + 2 * guard,), -7, device=device, dtype=torch.int64))
    cloud = ops.PointCloud(*(t[guard:guard + cap] for t in whole), torch.zeros(2, dtype=torch.int64, device=device),
                           torch.full((B,), -1, dtype=torch.int64, device=device))
    return cloud, whole, [t.clone() for t in whole]


def _untouched(whole, poison, first, guard=64):
    """Everything but rows [guard, guard + first) still holds the poison (bit patterns: the NaNs too)."""
    for t, p in zip(whole, poison):
        a, b = t.view(torch.int32) if t.dtype == torch.float32 else t, p.view(torch.int32) if p.dtype == torch.float32 else p
        if not (torch.equal(a[:guard], b[:guard]) and torch.equal(a[guard + first:], b[guard + first:])):
            return False
    return True


def _args(device, which=(0, 1, 2)):
    sizes = [po.RAGGED[b] for b in which]
    buf, offs = po.colours(sizes)
    return dict(pred=torch.from_numpy(po.planes(3)[list(which)]).to(device), sizes=sizes,
                inv_K=torch.from_numpy(po.inv_K(sizes)).to(device), cam_to_world=torch.from_numpy(po.poses(len(sizes))).to(device),
                colour=torch.from_numpy(buf).to(device), colour_off=torch.from_numpy(offs).to(device), lo=po.LO, hi=po.HI, stride=2,
                edge=0.1)


def test_capacity_and_append(device):
    from ppeadepth import ops
    kw = _args(device)
    full = ops.point_cloud(**kw)
    fx, fr, fi, _ = full.trim()
    total = len(fi)
    counts = full.counts.clone()
    assert total > 200
    for cap in (total + 50, total, total - 1, 100, 1, 0):                     # a tail that stays, exact, too small, nothing
        cloud, whole, poison = _guarded(cap, 3, device)
        got = ops.point_cloud(out=cloud, **kw)
        fit = min(cap, total)
        assert got.cursor.tolist() == [fit, total - fit] and torch.equal(got.counts, counts)
        assert _untouched(whole, poison, fit)
        assert torch.equal(cloud.xyz[:fit], fx[:fit]) and torch.equal(cloud.rgb[:fit], fr[:fit]) and torch.equal(cloud.index[:fit], fi[:fit])
    assert ops.point_cloud(capacity=0, **kw).cursor.tolist() == [0, total]    # the buffers of the op's own making
    # two appended calls are the two separate results one after the other; a third that does not fit is cut and counted
    other = dict(kw, stride=3, edge=0.0)
    second = ops.point_cloud(**other)
    sx, sr, si, _ = second.trim()
    cap = total + len(si) + 40
    cloud, whole, poison = _guarded(cap, 3, device)
    ops.point_cloud(out=cloud, **kw)
    ops.point_cloud(out=cloud, **other)
    assert cloud.cursor.tolist() == [total + len(si), 0] and torch.equal(cloud.counts, second.counts)
    assert torch.equal(cloud.xyz[:total + len(si)], torch.cat([fx, sx])) and torch.equal(cloud.rgb[:total + len(si)], torch.cat([fr, sr]))
    assert torch.equal(cloud.index[:total + len(si)], torch.cat([fi, si])) and _untouched(whole, poison, total + len(si))
    ops.point_cloud(out=cloud, **kw)
    assert cloud.cursor.tolist() == [cap, total - 40] and torch.equal(cloud.xyz[-40:], fx[:40]) and _untouched(whole, poison, cap)


def test_refusals_write_nothing(device):
    import ctypes
    from ppeadepth import _abi, ops
    from ppeadepth._abi import ptr
    kw = _args(device)
    cloud, whole, poison = _guarded(4000, 3, device)
    cloud.cursor.copy_(torch.tensor([5, 9], device=device))
    for bad in (dict(stride=0), dict(mode="inverse"), dict(colour=torch.rand(3, 3, 47, 157, device=device), colour_off=None),
                dict(colour=kw["colour"].float()), dict(capacity=17), dict(scale=torch.ones(2, device=device)),
                dict(inv_K=kw["inv_K"][:2])):
        with pytest.raises(_abi.PpeaKernelError):
            ops.point_cloud(out=cloud, **dict(kw, **bad))
    # the entry point's own refusals: (stride, capacity, B, colour_mode, mode) -> status
    ws = torch.zeros(_abi.lib.ppea_point_cloud_workspace_bytes(3, 47 * 157, 1), dtype=torch.uint8, device=device)
    scale = torch.ones(3, device=device)
    table, _, _, largest = ops.export_targets(kw["sizes"], 3, torch.device(device))
    for (stride, cap, B, cmode, mode), status in (((0, 4000, 3, 1, 0), -2), ((1, -1, 3, 1, 0), -2), ((1, 4000, 65536, 1, 0), -2),
                                                  ((1, 4000, 3, 3, 0), -2), ((1, 4000, 3, -1, 0), -2), ((1, 4000, 3, 1, 2), -1)):
        got = _abi.lib.ppea_point_cloud_f32(ptr(kw["pred"]), ptr(scale), ptr(table), B, 24, 80, largest, po.LO, po.HI, mode, stride,
                                            0.1, ptr(kw["inv_K"]), None, ptr(kw["colour"]), ptr(kw["colour_off"]), cmode,
                                            ptr(cloud.xyz), ptr(cloud.rgb), ptr(cloud.index), cap, ptr(cloud.cursor),
                                            ptr(cloud.counts), ptr(ws), _abi.stream_ptr())
        assert got == status, (stride, cap, B, cmode, mode, got)
    assert _abi.lib.ppea_point_cloud_workspace_bytes(3, 100, 0) < 0
    torch.cuda.synchronize()
    assert _untouched(whole, poison, 0) and cloud.cursor.tolist() == [5, 9] and cloud.counts.tolist() == [-1] * 3
    assert not bool(ws.any())
    world = torch.eye(4, device=device).repeat(2, 1, 1)
    with pytest.raises(_abi.PpeaKernelError):
        ops.pose_accumulate(world, torch.zeros(2, 1, 4, 4, device=device), torch.ones(3, 1, dtype=torch.bool, device=device))


def test_two_calls_are_bit_equal(device):
    from ppeadepth import ops
    kw = _args(device)
    a, b = ops.point_cloud(**kw), ops.point_cloud(**kw)
    assert a.cursor.tolist() == b.cursor.tolist() and a.cursor.tolist()[0] > 200
    n = a.cursor.tolist()[0]
    assert torch.equal(a.xyz[:n].view(torch.int32), b.xyz[:n].view(torch.int32)) and torch.equal(a.rgb[:n], b.rgb[:n])
    assert torch.equal(a.index[:n], b.index[:n]) and torch.equal(a.counts, b.counts)


def test_pose_accumulate_against_float64(device):
    from ppeadepth import ops
    B, F, n = 5, 2, 12                                                        # two workgroups, the second partly filled
    world = torch.eye(4, device=device).repeat(B, 1, 1).contiguous()
    poses, presents, since, worst = [], [], np.zeros(B, int), 0.0
    for t in range(n):
        pose = np.stack([po.poses(F, seed=50 + 11 * t + b) for b in range(B)])
        present = np.ones((B, F), bool)
        present[t % B, 0] = t % 3 == 0                                        # some cameras are reset now and then
        present[:, 1] = False                                                 # only column 0 is read
        poses.append(pose), presents.append(present)
        ops.pose_accumulate(world, torch.from_numpy(pose).to(device), torch.from_numpy(present).to(device))
        ref = po.chain_f64(poses, presents)[-1]
        since = np.where(present[:, 0], since + 1, 0)
        got = world.cpu().numpy().astype(np.float64)
        for b in range(B):
            if since[b] == 0:
                assert np.array_equal(got[b], np.eye(4)), (t, b)
            else:
                err = np.abs(got[b] - ref[b]).max()
                worst = max(worst, err / po.chain_bound(ref[b], since[b]))
                assert err <= po.chain_bound(ref[b], since[b]), (t, b, err)
    print(f"pose chain: largest error / bound {worst:.3f} over {n} steps")


# ---- predictor, stream, CLI ---------------------------------------------------------------------------------------------
H, W, B = 64, 96, 2
K_NORM = np.array([[0.58, 0, 0.5], [0, 1.92, 0.5], [0, 0, 1]])
_model = {}


def _setup(device):
    """(model, opt, trainer, engine, predictor): the predictor tests' cheapest configuration, built once per module."""
    if not _model:
        from ppeadepth import networks, options
        from ppeadepth.dist import TrainEngine
        from ppeadepth.inference import DepthPredictor
        from ppeadepth.trainer import Trainer
        opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False)
        torch.manual_seed(0)
        model = networks.RepDepth(opt)
        synth.fill_state_dict(model, conditioned=True)
        model.to(device).train()
        tr = Trainer(opt, model, device)
        _model["v"] = (model, opt, tr, TrainEngine(tr, lr=1e-4), DepthPredictor(model, opt))
    return _model["v"]


def _clip(device):
    data = {k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W, frame_ids=(0, -1, 1, -2)).items()}
    return [data[("color", f, 0)] for f in (-2, -1, 0, 1)], data[("K", 2)], data[("inv_K", 2)]


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                         # warm-up: tables, scales and the workspace reach the device here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                    # one stream, no parallel branches
        fn()
    return graph


KW = dict(lo=0.2, hi=80.0, stride=2, edge=0.3)


def test_points_are_captured_after_a_push(device):
    from ppeadepth import ops
    model, opt, tr, eng, p = _setup(device)
    clip, K2, inv_K2 = _clip(device)
    s = p.stream(B)
    size = (75, 121)
    ik = p.full_inv_K(K_NORM, size).repeat(B, 1, 1).contiguous()
    pose = torch.from_numpy(po.poses(B)).to(device)
    outs = [s.push(c, K2, inv_K2, 0.1, 10.0) for c in clip[:3]]
    static = outs[1]["disp"].clone()
    captured = ops.new_point_cloud(B * 38 * 61, B, device, False)

    def run(disp, cloud):
        p.points(disp, size, ik, pose=pose, out=cloud.clear(), **KW)

    graph = _capture(lambda: run(static, captured))
    for r in (outs[2], s.push(clip[3], K2, inv_K2, 0.1, 10.0)):               # new input
        static.copy_(r["disp"])
        graph.replay()
        eager = ops.new_point_cloud(B * 38 * 61, B, device, False)
        run(r["disp"], eager)
        n, dropped = eager.cursor.tolist()
        assert captured.cursor.tolist() == [n, 0] and dropped == 0 and n > 50
        assert torch.equal(captured.xyz[:n].view(torch.int32), eager.xyz[:n].view(torch.int32))
        assert torch.equal(captured.index[:n], eager.index[:n]) and torch.equal(captured.counts, eager.counts)
    # the thin call is the op
    from ppeadepth import layers
    scaled, _ = layers.disp_to_depth(outs[2]["disp"], opt.min_depth, opt.max_depth)
    a, b = p.points(outs[2]["disp"], size, ik, pose=pose, **KW), ops.point_cloud(scaled, size, ik, pose, **KW)
    k = a.cursor.tolist()[0]
    assert k > 50 and torch.equal(a.cursor, b.cursor) and torch.equal(a.xyz[:k].view(torch.int32), b.xyz[:k].view(torch.int32))


def test_stream_map(device):
    from ppeadepth import ops
    model, opt, tr, eng, p = _setup(device)
    clip, K2, inv_K2 = _clip(device)
    frames = clip + [clip[2]]                                                 # five pushes
    ik = p.full_inv_K(K_NORM, (H, W)).repeat(B, 1, 1).contiguous()
    cap = 5 * B * (H // 4) * (W // 4)
    mask = torch.tensor([False, True])

    def feed(s, m, add):
        outs, worlds = [], []
        for t, c in enumerate(frames):
            if t == 3:
                s.reset(mask)                                                 # camera 1 starts a new clip in the middle
            out = s.push(c, K2, inv_K2, 0.1, 10.0)
            add(out, c)
            outs.append(out), worlds.append(m.world.clone())
        return outs, worlds

    s = p.stream(B)
    m = s.map(cap, **dict(KW, stride=4))
    assert torch.equal(m.world, torch.eye(4, device=device).repeat(B, 1, 1))
    parts = []

    def eager_add(out, c):
        m.add(out, c, ik)
        parts.append(p.points(out["disp"], (H, W), ik, color=c, pose=m.world, **dict(KW, stride=4)).trim())

    outs, worlds = feed(s, m, eager_add)
    refs = po.chain_f64([o["pose"].cpu().numpy() for o in outs], [o["present"].cpu().numpy() for o in outs])
    since, worst = np.zeros(B, int), 0.0
    for t, (world, ref, out) in enumerate(zip(worlds, refs, outs)):
        present = out["present"][:, 0].cpu().numpy()
        assert present.tolist() == [t > 0, t > 0 and t != 3]
        since = np.where(present, since + 1, 0)
        got = world.cpu().numpy().astype(np.float64)
        for b in range(B):
            if since[b] == 0:
                assert np.array_equal(got[b], np.eye(4)), (t, b)              # also the reset camera, at t = 3
            else:
                err = np.abs(got[b] - ref[b]).max()
                worst = max(worst, err / po.chain_bound(ref[b], since[b]))
                assert err <= po.chain_bound(ref[b], since[b]), (t, b, err)
    print(f"stream map: largest chain error / bound {worst:.3f}")
    xyz, rgb, index, dropped = m.cloud().trim()
    assert dropped == 0 and len(index) > 200
    assert torch.equal(xyz.view(torch.int32), torch.cat([q[0] for q in parts]).view(torch.int32))
    assert torch.equal(rgb, torch.cat([q[1] for q in parts])) and torch.equal(index, torch.cat([q[2] for q in parts]))
    # the same map from a captured stream and a captured add
    s2 = p.stream(B).capture()
    m2 = s2.map(cap, **dict(KW, stride=4))
    static = {"disp": outs[0]["disp"].clone(), "pose": outs[0]["pose"].clone(), "present": outs[0]["present"].clone()}
    colour = clip[0].clone()
    graph = _capture(lambda: m2.add(static, colour, ik))
    m2.clear()
    torch.cuda.synchronize()

    def replay_add(out, c):
        for k in static:
            static[k].copy_(out[k])
        colour.copy_(c)
        graph.replay()

    _, worlds2 = feed(s2, m2, replay_add)
    for a, b in zip(worlds, worlds2):
        assert torch.equal(a, b)
    xyz2, rgb2, index2, dropped2 = m2.cloud().trim()
    assert dropped2 == 0 and torch.equal(xyz2.view(torch.int32), xyz.view(torch.int32)) and torch.equal(rgb2, rgb)
    assert torch.equal(index2, index)
    m.clear()
    assert m.cloud().cursor.tolist() == [0, 0] and torch.equal(m.world, torch.eye(4, device=device).repeat(B, 1, 1))


def _jpeg_frames(root):
    """Three lines of two frame sizes in KITTI's layout, each with its neighbour -1; -> the split file's lines, the sizes."""
    from PIL import Image
    rng = np.random.default_rng(3)
    drives = {"2011_09_26/drive_a_sync": (100, 300), "2011_09_28/drive_b_sync": (110, 330)}
    for folder, (h, w) in drives.items():
        d = os.path.join(root, folder, "image_02", "data")
        os.makedirs(d)
        for i in range(3):
            y, x = np.mgrid[0:h, 0:w]
            img = np.stack([127 + 100 * np.sin(x / 17.0 + i + c) * np.cos(y / 11.0) for c in range(3)], -1)
            img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, "{:010d}.jpg".format(i)), quality=95)
    a, b = drives
    lines = [f"{a} 1 l", f"{b} 1 l", f"{a} 2 l"]              # the first batch of two mixes the sizes
    sizes = [drives[a], drives[b], drives[a]]
    return lines, sizes


def test_predict_cli_writes_ply(device, tmp_path):
    from ppeadepth import datasets, predict, vis
    from ppeadepth.input_pipeline import DeviceInputPipeline, KITTI_K
    model, opt, tr, eng, p = _setup(device)
    lines, sizes = _jpeg_frames(str(tmp_path / "kitti"))
    split = str(tmp_path / "files.txt")
    with open(split, "w") as f:
        f.write("\n".join(lines) + "\n")
    ckpt = str(tmp_path / "weights")
    tr.save_model_debug(ckpt, eng)
    out = str(tmp_path / "out")
    assert predict.main(["--data_path", str(tmp_path / "kitti"), "--split_file", split, "--load_weights_folder", ckpt,
                         "--out", out, "--batch_size", str(B), "--height", str(H), "--width", str(W), "--adapter",
                         "--weights_init", "scratch", "--ply", "--ply_stride", "2", "--ply_edge", "0.5", "--depth_npy"]) == 0
    import shutil
    shutil.rmtree(ckpt)                              # most of a gigabyte: not kept for pytest's tmp_path retention
    ids = [0] + p.lookup_ids
    data = datasets.KITTIRAWDataset(str(tmp_path / "kitti"), lines, ids)
    pipe = DeviceInputPipeline(None, H, W, device, frame_idxs=tuple(ids), is_train=False)
    mn, mx = tr.depth_bin_tracker.compute()
    n = 0
    for start in range(0, len(lines), B):
        frames = datasets.collate_raw([data[i] for i in range(start, min(start + B, len(lines)))])
        inputs = pipe(frames)
        disp = p.predict(inputs[("color", 0, 0)], inputs[("color", -1, 0)], inputs[("K", 2)], inputs[("inv_K", 2)], mn, mx)["disp"]
        own = sizes[start:start + frames.batch]
        rows = _rows(own)
        for b in range(frames.batch):
            name = "{:010d}".format(n)
            frame = frames.image(b)                                           # frame 0 of item b
            one = p.points(disp[b:b + 1], [own[b]], p.full_inv_K(KITTI_K, [own[b]]), color=frame.reshape(-1).to(device),
                           stride=2, edge=0.5)
            xyz, rgb, index, _ = _host(one)
            got_xyz, got_rgb = vis.read_ply(os.path.join(out, "ply", name + ".ply"))
            assert len(index) > 100 and got_xyz.tobytes() == xyz.tobytes() and np.array_equal(got_rgb, rgb)
            assert np.array_equal(rgb, frame.numpy().reshape(-1, 3)[index])
            depth = np.load(os.path.join(out, "depth", name + ".npy"))
            assert depth.shape == own[b] and np.array_equal(got_xyz[:, 2], depth.reshape(-1)[index])
            n += 1
    assert n == 3 and sorted(os.listdir(os.path.join(out, "ply"))) == ["{:010d}.ply".format(i) for i in range(3)]
