"""Prediction export on the GPU (csrc/depth_export.hip through ops.disp_export / plane_range / colorize, vis.colorize_device,
DepthPredictor.depth / .render, DepthStream.render, python -m ppeadepth.predict) against a float64 restatement written in
tests/export_oracle.py.  Inputs are seeded and synthetic: a smooth depth field with 8 % multiplicative noise, inverted.

Source planes are 24 x 80; targets (47, 157), (24, 80), (12, 41) -- a non-integer enlargement, the identity, a reduction, two
widths with 3 W no multiple of 4 and image offsets that are no multiple of 4 pixels -- as B = 1 and as one ragged batch, a
(1, 1) target, and 192 x 640 -> 375 x 1242 so that an image spans several chunks."""
import os

import numpy as np
import pytest
import torch

from oracle import synth

import export_oracle as eo

pytestmark = pytest.mark.gpu

CASES = {"b1": (eo.SRC, [(47, 157)]), "ragged": (eo.SRC, eo.RAGGED), "one": (eo.SRC, [(1, 1)]), "big": (eo.BIG[0], [eo.BIG[1]])}
# (scale, lo, hi): nothing on a clamp; part of the image on hi (the benchmark writer's numbers); part on lo
RANGES = ((0.5, 1e-3, 80.0), (5.4, 0.0, 80.0), (0.05, 1.0, 80.0))
_scenes = {}


def _planes(case):
    """[B,h,w] fp32 source planes of a case, built once and never modified."""
    if case not in _scenes:
        (h, w), sizes = CASES[case]
        _scenes[case] = np.stack([eo.scene(11 + b, h, w) for b in range(len(sizes))])
    return _scenes[case]


def _split(res, sizes):
    """What an op returned -> list of host arrays, one per image."""
    if isinstance(res, tuple):
        flat, table = res[0].cpu().numpy(), res[1].cpu().tolist()
        off = 0
        for (o, h, w), s in zip(table, sizes):
            assert (o, h, w) == (off,) + tuple(s)
            off += h * w
        return [flat[o:o + h * w].reshape((h, w) + flat.shape[1:]) for o, h, w in table]
    return list(res.cpu().numpy())


@pytest.mark.parametrize("mode", ["disp", "depth"])
@pytest.mark.parametrize("case", list(CASES))
def test_depth_f32_and_u16_against_float64(device, case, mode):
    from ppeadepth import ops
    planes, sizes = _planes(case), CASES[case][1]
    B = len(sizes)
    pred = torch.from_numpy(planes).to(device)
    total = sum(h * w for h, w in sizes)
    for k, (scale, lo, hi) in enumerate(RANGES):
        per_image = [scale * (1 + 0.25 * b) for b in range(B)]
        for scales in ([scale] * B, per_image):
            arg = scale if scales is not per_image else torch.tensor(scales, dtype=torch.float32, device=device)
            out = torch.full((total,), float("nan"), device=device)
            got = _split(ops.disp_export(pred, sizes, arg, lo, hi, mode, out=out), sizes)
            assert not bool(torch.isnan(out).any())                       # every output pixel is written
            q = _split(ops.disp_export(pred, sizes, arg, lo, hi, mode, dtype=torch.uint16), sizes)
            for b, size in enumerate(sizes):
                want = eo.depth_f64(planes[b], size, np.float32(scales[b]), lo, hi, mode)
                r = eo.rel(got[b], want)
                print(f"{case} {mode} scale {scales[b]:.3g} image {b}: rel {r:.2e}")
                assert got[b].dtype == np.float32 and r <= eo.RTOL
                if case != "one" and scales is not per_image:
                    on_hi, on_lo = float((want == hi).mean()), float((want == np.float64(np.float32(lo))).mean())
                    assert (on_hi > 0.02) == (k == 1) and (on_lo > 0.02) == (k == 2), (on_hi, on_lo)
                    if k:
                        assert 0.02 < max(on_hi, on_lo) < 0.98                # part of the image, not all of it
                # link 1: the kernel's quantisation against its definition
                assert q[b].dtype == np.uint16
                assert np.array_equal(q[b].astype(np.int64), (torch.from_numpy(got[b]) * 256).to(torch.int64).numpy())
                # link 2: against the float64 oracle
                v = want * 256
                d = eo.RTOL * v
                assert (q[b] >= np.floor(v - d)).all() and (q[b] <= np.floor(v + d)).all()


def test_export_refusals(device):
    from ppeadepth import _abi, ops
    pred = torch.from_numpy(_planes("b1")).to(device)
    with pytest.raises(_abi.PpeaKernelError):
        ops.disp_export(pred, (47, 157), 1.0, 0.0, 256.0, dtype=torch.uint16)          # hi * 256 > 65535
    assert ops.disp_export(pred, (47, 157), 1.0, 0.0, 255.99, dtype=torch.uint16).dtype == torch.uint16
    ops.disp_export(pred, (47, 157), 1.0, 0.0, 256.0)                                   # fp32 has no such limit
    with pytest.raises(_abi.PpeaKernelError):
        ops.disp_export(pred, (47, 157), mode="inverse")
    with pytest.raises(_abi.PpeaKernelError):
        ops.disp_export(pred, [(47, 157), (24, 80)])                                    # two sizes for one image
    with pytest.raises(_abi.PpeaKernelError):
        ops.disp_export(pred, (47, 157), out=torch.empty(5, device=device))
    with pytest.raises(_abi.PpeaKernelError):
        ops.plane_range(pred, 101.0)
    torch.cuda.synchronize()


# ---- plane_range --------------------------------------------------------------------------------------------------------
def _range_planes():
    """[6,24,80]: a scene, duplicates (quantised), a constant, negative and positive values, NaNs (1901 values left, so that
    q = 50 lands exactly on element 950), -0.0 / tiny values next to a few large ones."""
    a = eo.scene(21, *eo.SRC)
    dup = np.round(a * 64) / 64
    const = np.full(eo.SRC, 0.375, np.float32)
    neg = (eo.scene(22, *eo.SRC) - 0.05).astype(np.float32)
    assert (neg < 0).mean() > 0.2 and (neg > 0).mean() > 0.2
    nan = eo.scene(23, *eo.SRC).copy()
    nan.reshape(-1)[np.random.default_rng(0).choice(nan.size, 19, replace=False)] = np.nan
    assert int((~np.isnan(nan)).sum()) == 1901
    wide = (eo.scene(24, *eo.SRC) * np.float32(1e-3)).astype(np.float32)
    wide[3, 5:9] = [-3e4, 7e8, -1e-30, 2e-38]
    return np.stack([a, dup, const, neg, nan, wide]).astype(np.float32)


@pytest.mark.parametrize("q", [100.0, 95.0, 50.0, 99.9, 0.0])
@pytest.mark.parametrize("which", ["small", "big"])
def test_plane_range(device, which, q):
    from ppeadepth import ops
    if which == "small":
        planes = _range_planes()
    else:
        planes = np.stack([eo.scene(31, *eo.BIG[0]), eo.scene(32, *eo.BIG[0]) - np.float32(0.03)]).astype(np.float32)
        planes[1, 100, 17:40] = np.nan
    x = torch.from_numpy(planes).to(device)
    got = ops.plane_range(x, q)
    again = ops.plane_range(x, q, out=torch.empty(planes.shape[0] * 2, device=device))
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))      # two calls agree bit for bit
    got = got.cpu().numpy()
    for b, p in enumerate(planes):
        ok = p[~np.isnan(p)]
        assert got[b, 0].tobytes() == np.nanmin(p).tobytes(), b
        if q == 100.0:
            assert got[b, 1].tobytes() == np.nanmax(p).tobytes(), b
        want = np.percentile(ok.astype(np.float64), q)
        ulp = np.spacing(np.abs(np.float32(want))).astype(np.float64)
        print(f"{which} plane {b} q {q}: got {got[b, 1]!r} want {want!r}")
        assert abs(np.float64(got[b, 1]) - want) <= ulp, (b, got[b, 1], want)
    if which == "small" and q == 50.0:       # lands exactly on an element: the element itself
        ok = np.sort(planes[4][~np.isnan(planes[4])])
        assert got[4, 1].tobytes() == ok[950].tobytes()
    empty = ops.plane_range(torch.full((1, 3, 5), float("nan"), device=device), q).cpu().numpy()
    assert np.isnan(empty).all()


# ---- colorize -----------------------------------------------------------------------------------------------------------
def _range_of(p, lo_q=0.0, hi_q=95.0):
    ok = p[~np.isnan(p)].astype(np.float64)
    return np.float32(np.percentile(ok, lo_q)), np.float32(np.percentile(ok, hi_q))


@pytest.mark.parametrize("cmap", ["plasma", "viridis"])
@pytest.mark.parametrize("case", list(CASES))
def test_colorize_with_an_explicit_range(device, case, cmap):
    """Every case; in the ragged batch image 0 has values below and above its range, image 1 (the identity) NaN and
    infinite pixels, image 2 a range with vmin == vmax.  The flat output sits inside a larger buffer prefilled with a
    sentinel, twice with different sentinels: a byte the launch did not write differs between the two runs."""
    from ppeadepth import ops, vis
    planes, sizes = _planes(case).copy(), CASES[case][1]
    B = len(sizes)
    ranges = [_range_of(planes[b], 20.0 if b == 0 else 0.0) for b in range(B)]
    if case == "ragged":
        planes[1, 3, 4:7] = np.nan
        planes[1, 23, 79] = np.nan
        planes[1, 0, 0] = np.inf
        planes[1, 5, 5] = -np.inf
        ranges[2] = (planes[2, 0, 0], planes[2, 0, 0])
        planes[2, 4, 4] = np.inf                       # inf * 0: NaN, black
    x = torch.from_numpy(planes).to(device)
    rng = torch.tensor(np.array(ranges, np.float32)).to(device)
    table = vis.lut(cmap)
    total = sum(h * w for h, w in sizes)
    guard = 64
    runs = []
    for sentinel in (0x5A, 0xA5):
        backing = torch.full((guard + total * 3 + guard,), sentinel, dtype=torch.uint8, device=device)
        res = ops.colorize(x, sizes, rng, vis.lut(cmap, device), out=backing[guard:guard + total * 3])
        torch.cuda.synchronize()
        host = backing.cpu().numpy()
        assert (host[:guard] == sentinel).all() and (host[-guard:] == sentinel).all()          # nothing outside the images
        runs.append((host[guard:-guard], _split(res, sizes)))
    assert np.array_equal(runs[0][0], runs[1][0])                                               # every byte inside is written
    for b, size in enumerate(sizes):
        img = runs[0][1][b]
        assert img.dtype == np.uint8 and img.shape == tuple(size) + (3,)
        t = eo.colour_t(planes[b], size, *ranges[b])
        if ranges[b][0] != ranges[b][1]:             # vmin == vmax: t is 0 or NaN, checked exactly below
            eo.check_colours(img, t, table, f"{case} image {b}")
        if case == "ragged" and b == 0:
            assert (t < 0).mean() > 0.1 and (t >= 256).mean() > 0.02
        if case == "ragged" and b == 1:
            assert (img[3, 4:7] == 0).all() and (img[23, 79] == 0).all() and (img[3, 3] != 0).any()
            assert (img[0, 0] == table[255]).all() and (img[5, 5] == table[0]).all()
        if case == "ragged" and b == 2:
            bad = np.isnan(t)
            assert bad.any() and (img[bad] == 0).all() and (img[~bad] == table[0]).all()


def test_colorize_device_is_plane_range_then_colorize(device):
    from ppeadepth import ops, vis
    x = torch.from_numpy(_planes("ragged")).to(device)
    flat, table = vis.colorize_device(x, eo.RAGGED, percentile=95.0, cmap="magma")
    rng = ops.plane_range(x, 95.0)
    want, table2 = ops.colorize(x, eo.RAGGED, rng, vis.lut("magma", device))
    assert torch.equal(flat, want) and torch.equal(table, table2)
    # one bound given: the other still comes from the plane
    half, _ = vis.colorize_device(x, eo.RAGGED, vmin=0.0, percentile=95.0, cmap="magma")
    rng[:, 0] = 0.0
    assert torch.equal(half, ops.colorize(x, eo.RAGGED, rng, vis.lut("magma", device))[0])
    dense = vis.colorize_device(x[:, None], percentile=95.0)                 # [B,1,h,w], own size
    assert tuple(dense.shape) == (3,) + eo.SRC + (3,) and dense.dtype == torch.uint8


def test_device_against_host_without_a_resize(device):
    from ppeadepth import vis
    planes = _planes("ragged").copy()
    planes[0, 2, 2] = np.nan
    got = vis.colorize_device(torch.from_numpy(planes).to(device), None, vmin=0.02, vmax=0.09).cpu().numpy()
    for b, p in enumerate(planes):
        host = vis.colorize(p, np.float32(0.02), np.float32(0.09))
        t = eo.colour_t(p, p.shape, np.float32(0.02), np.float32(0.09))
        eo.check_colours(host, t, vis.lut("plasma"), f"host image {b}")
        eo.check_colours(got[b], t, vis.lut("plasma"), f"device image {b}")
        print(f"image {b}: {(got[b] != host).any(-1).mean():.2%} of the pixels differ between host and device")
    # statistics from the plane itself: the same picture as the host function with vmin = vmax = None
    clean = _planes("ragged")
    auto = vis.colorize_device(torch.from_numpy(clean).to(device)).cpu().numpy()
    for b, p in enumerate(clean):
        t = eo.colour_t(p, p.shape, p.min(), p.max())
        eo.check_colours(auto[b], t, vis.lut("plasma"), f"auto image {b}")
        eo.check_colours(vis.colorize(p, None, None), t, vis.lut("plasma"), f"auto host image {b}")


# ---- predictor, stream, CLI ---------------------------------------------------------------------------------------------
H, W, B = 64, 96, 2
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


def test_render_and_depth_are_captured_after_a_push(device):
    model, opt, tr, eng, p = _setup(device)
    data = {k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W, frame_ids=(0, -1, 1, -2)).items()}
    clip = [data[("color", f, 0)] for f in (-2, -1, 0, 1)]
    K2, inv_K2 = data[("K", 2)], data[("inv_K", 2)]
    s = p.stream(B)
    size = (75, 121)
    outs = [s.push(c, K2, inv_K2, 0.1, 10.0) for c in clip[:3]]
    scale = torch.tensor([1.0, 1.3], device=device)

    def run(r, rgb, lowest, depth):
        s.render(r, "disp", size, percentile=95.0, out=rgb)
        s.render(r, "lowest_cost", size, out=lowest)
        p.depth(r["disp"], size, scale, out=depth)

    def buffers():
        return (torch.zeros(B, *size, 3, dtype=torch.uint8, device=device),
                torch.zeros(B, *size, 3, dtype=torch.uint8, device=device), torch.zeros(B, *size, device=device))

    static = {k: outs[1][k].clone() for k in ("disp", "lowest_cost")}
    captured = buffers()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static, *captured)                       # warm-up: the target table and the LUT reach the device here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                    # one stream, no parallel branches
        run(static, *captured)
    for r in (outs[2], s.push(clip[3], K2, inv_K2, 0.1, 10.0)):        # new input
        for k in static:
            static[k].copy_(r[k])
        graph.replay()
        eager = buffers()
        run(r, *eager)
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
        assert len(torch.unique(eager[0])) > 16 and float(eager[2].std()) > 0        # pictures, not blanks
    # the thin calls are the ops
    from ppeadepth import layers, ops
    scaled, _ = layers.disp_to_depth(outs[2]["disp"], opt.min_depth, opt.max_depth)
    assert torch.equal(p.depth(outs[2]["disp"], size, scale), ops.disp_export(scaled, size, scale))


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


def test_predict_cli_writes_the_three_products(device, tmp_path):
    from PIL import Image
    from ppeadepth import datasets, predict
    from ppeadepth.input_pipeline import DeviceInputPipeline
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
                         "--weights_init", "scratch", "--depth_npy", "--benchmark", "--colour", "--percentile", "95"]) == 0
    import shutil
    shutil.rmtree(ckpt)                              # most of a gigabyte: not kept for pytest's tmp_path retention
    # the same prediction, made here from the model the checkpoint was written from
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
        depth = _split(p.depth(disp, own), own)
        bench = p.depth(disp, (352, 1216), scale=5.4, lo=0.0, hi=80.0).cpu()
        rgb = _split(p.render(disp, own, percentile=95.0), own)
        for b in range(frames.batch):
            name = "{:010d}".format(n)
            got = np.load(os.path.join(out, "depth", name + ".npy"))
            assert got.dtype == np.float32 and got.shape == own[b] and got.tobytes() == depth[b].tobytes()
            assert 1e-3 <= got.min() and got.max() <= 80.0
            with Image.open(os.path.join(out, "benchmark", name + ".png")) as im:
                assert im.mode == "I;16" and im.size == (1216, 352)
                png = np.array(im)
            assert png.dtype == np.uint16 and np.array_equal(png.astype(np.int64), torch.floor(bench[b] * 256).to(torch.int64).numpy())
            with Image.open(os.path.join(out, "colour", name + ".png")) as im:
                assert im.mode == "RGB" and im.size == (own[b][1], own[b][0])
                assert np.array_equal(np.array(im), rgb[b])
            n += 1
    assert n == 3 and sorted(os.listdir(os.path.join(out, "depth"))) == ["{:010d}.npy".format(i) for i in range(3)]
