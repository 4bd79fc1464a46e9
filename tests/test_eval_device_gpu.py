"""Device-side depth metrics (csrc/eval_metrics.hip, ops.depth_errors, evaluate.DeviceGroundTruth, Trainer.val(metrics=
"device")) against the host protocol `evaluate.evaluate_image` and a float64 restatement written below.  Inputs are seeded
and synthetic: a smooth depth field, a noisy prediction of it, sparse LiDAR-like (eigen) or dense (cityscapes) ground truth."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-5              # the bound between two statements of this protocol (tests/test_oracle_golden.py:320)
HOST_OWN = 2.5e-6        # a host path further than this from float64 on a fixture widens the bound there to 4 x its distance
BAND = 1e-5              # a1..a3 may differ only by pixels whose max(gt/pred, pred/gt) lies this close to a threshold
THRESHOLDS = (1.25, 1.5625, 1.953125)


def _scene(seed, h, w, gh, gw, keep, quantise=False):
    """-> (scaled disparity [h,w] fp32, ground truth [gh,gw] fp32 with 0 = no return)."""
    g = torch.Generator().manual_seed(seed)
    def field(H, W):
        y = torch.linspace(0, 1, H)[:, None]
        x = torch.linspace(0, 1, W)[None, :]
        return 6 + 40 * (1 - y) ** 2 + 3 * torch.sin(7 * x + seed) * y + 2 * torch.cos(5 * y * x)      # >= 1
    depth = field(h, w) * (1 + 0.08 * torch.randn(h, w, generator=g)).clamp(0.5, 1.5) * 1.7
    gt = field(gh, gw) * (1 + 0.12 * torch.randn(gh, gw, generator=g)).clamp(0.5, 1.5)
    if quantise:
        depth, gt = torch.round(depth), torch.round(gt * 2) / 2
    gt = gt * (torch.rand(gh, gw, generator=g) < keep)
    return (1 / depth).float().numpy(), gt.float().numpy()


def _host_mask(gt, split):
    from ppeadepth import evaluate
    if split == "cityscapes":
        gt = gt[:int(round(gt.shape[0] * 0.75))][256:, 192:1856]
    if split == "eigen":
        return evaluate.eigen_crop_mask(gt)
    return np.logical_and(gt > evaluate.MIN_VAL, gt < evaluate.MAX_VAL)


def _host(disp, gt, split, median_scaling=True, scale=1.0):
    """The host path: (7 errors fp64 array, ratio, valid count); an empty mask gives NaN without numpy's warnings."""
    from ppeadepth import evaluate
    n = int(_host_mask(gt, split).sum())
    if n == 0:
        return np.full(7, np.nan), np.float32(np.nan), 0
    e, r = evaluate.evaluate_image(disp, gt, split, median_scaling, scale)
    return np.array(e, dtype=np.float64), r, n


def _resize_f64(img, H, W):
    """Bilinear, half-pixel centres, clamped source coordinates, in float64."""
    h, w = img.shape
    def axis(n_in, n_out):
        s = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, s - i0
    y0, y1, ly = axis(h, H)
    x0, x1, lx = axis(w, W)
    img = img.astype(np.float64)
    top = img[y0][:, x0] * (1 - lx) + img[y0][:, x1] * lx
    bot = img[y1][:, x0] * (1 - lx) + img[y1][:, x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def _f64(disp, gt, split, median_scaling=True, scale=1.0):
    """The protocol restated in float64 -> (7 errors, ratio, thresh array)."""
    H, W = gt.shape
    if split == "cityscapes":
        H = int(round(H * 0.75))
        gt = gt[:H]
    pred = 1 / _resize_f64(disp, H, W)
    if split == "cityscapes":
        gt, pred = gt[256:, 192:1856], pred[256:, 192:1856]
    mask = _host_mask(gt, "eigen" if split == "eigen" else "range")
    pred, g = pred[mask] * scale, gt[mask].astype(np.float64)
    ratio = np.median(g) / np.median(pred)
    if median_scaling:
        pred = pred * ratio
    pred = np.clip(pred, np.float64(np.float32(1e-3)), 80.0)
    th = np.maximum(g / pred, pred / g)
    e = [np.mean(np.abs(g - pred) / g), np.mean((g - pred) ** 2 / g), np.sqrt(np.mean((g - pred) ** 2)),
         np.sqrt(np.mean((np.log(g) - np.log(pred)) ** 2))] + [np.mean(th < t) for t in THRESHOLDS]
    return np.array(e), ratio, th


def _device(device, disps, gts, split, median_scaling=True, scale=1.0):
    from ppeadepth import evaluate
    dg = evaluate.DeviceGroundTruth(gts, device)
    pred = torch.from_numpy(np.stack(disps)).to(device)
    e, r, c = dg.score(pred, 0, split, median_scaling, scale)
    torch.cuda.synchronize()
    return e.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy()


def _rel(a, b):
    """max |a - b| / |b|; equal entries count as 0 (also 0 against 0), a difference from 0 as inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(d == 0, 0.0, d / np.abs(b))))


def _flip_parity(gt, split, want_odd):
    """Drops one valid return if the valid count has the wrong parity."""
    gt = gt.copy()
    if (int(_host_mask(gt, split).sum()) % 2 == 1) != want_odd:
        view = gt[:int(round(gt.shape[0] * 0.75))][256:, 192:1856] if split == "cityscapes" else gt
        ys, xs = np.nonzero(_host_mask(gt, split))
        view[ys[0], xs[0]] = 0
    assert (int(_host_mask(gt, split).sum()) % 2 == 1) == want_odd
    return gt


# ---- 1. exact where it can be exact --------------------------------------------------------------------------------
@pytest.mark.parametrize("split,gh,gw", [("eigen", 120, 400), ("cityscapes", 400, 640), ("benchmark", 96, 320)])
@pytest.mark.parametrize("median_scaling,scale", [(True, 1.0), (False, 1.07)])
def test_same_size_prediction_is_exact_against_the_host_path(device, split, gh, gw, median_scaling, scale):
    """Prediction of the ground truth's (resize target) size: the resize is the identity in both implementations and 1 / x
    is IEEE division, so ratio, valid count and a1..a3 must be EQUAL; the continuous errors within 1e-5.  One ragged batch
    holds an odd and an even valid count (middle values differ), heavy ties, and an image with an empty mask."""
    ph = int(round(gh * 0.75)) if split == "cityscapes" else gh
    cases = []
    for seed, (want_odd, quantise) in enumerate([(True, False), (False, False), (True, True), (False, True)]):
        disp, gt = _scene(seed, ph, gw, gh, gw, 0.3, quantise)
        cases.append((disp, _flip_parity(gt, split, want_odd)))
    cases.insert(2, (cases[0][0], np.zeros((gh, gw), np.float32)))          # no valid pixel, in the middle of the batch
    # the even continuous case really has two different middle values
    sel = np.sort(cases[1][1][:ph][256:, 192:1856][_host_mask(cases[1][1], split)] if split == "cityscapes"
                  else cases[1][1][_host_mask(cases[1][1], split)])
    assert len(sel) % 2 == 0 and sel[len(sel) // 2 - 1] != sel[len(sel) // 2]
    e, r, c = _device(device, [d for d, _ in cases], [g for _, g in cases], split, median_scaling, scale)
    for i, (disp, gt) in enumerate(cases):
        he, hr, hn = _host(disp, gt, split, median_scaling, scale)
        print(f"[{split} ms={median_scaling}] image {i}: n {c[i]} / {hn}, ratio {r[i]!r} / {hr!r}, device {e[i]}, host {he}")
        assert c[i] == hn
        if hn == 0:
            assert np.isnan(e[i]).all() and np.isnan(r[i])
            continue
        if median_scaling:
            assert np.float32(r[i]).tobytes() == np.float32(hr).tobytes()
        assert (e[i][4:] == he[4:]).all(), (e[i][4:], he[4:])
        assert _rel(e[i][:4], he[:4]) <= RTOL
    # the images around the empty one are what they are alone
    alone = _device(device, [cases[3][0]], [cases[3][1]], split, median_scaling, scale)
    assert alone[0][0].tobytes() == e[3].tobytes() and alone[1][0] == r[3] and alone[2][0] == c[3]


# ---- 2. real sizes -------------------------------------------------------------------------------------------------
REAL = [("eigen", (48, 160), [(375, 1242), (370, 1226), (375, 1242)], 0.05),
        ("eigen", (192, 640), [(375, 1242), (370, 1226), (375, 1242)], 0.05),
        ("cityscapes", (192, 512), [(1024, 2048), (1024, 2048)], 0.6)]


@pytest.mark.parametrize("split,hw,gt_sizes,keep", REAL)
def test_real_sizes_against_host_and_float64(device, split, hw, gt_sizes, keep):
    """Continuous errors and ratio within rtol 1e-5 of the host path (4 x the host's own distance from float64 where that
    distance exceeds 2.5e-6); a1..a3 differ from the host by at most the number of pixels within relative 1e-5 of the
    threshold in the float64 restatement, and the fixture keeps that number <= 0.1 % of the valid pixels."""
    scenes = [_scene(10 + i, hw[0], hw[1], gh, gw, keep) for i, (gh, gw) in enumerate(gt_sizes)]
    e, r, c = _device(device, [d for d, _ in scenes], [g for _, g in scenes], split)
    worst = {"device_vs_host": 0.0, "host_vs_f64": 0.0, "device_vs_f64": 0.0, "count_delta": 0, "count_allowed": 0}
    for i, (disp, gt) in enumerate(scenes):
        he, hr, hn = _host(disp, gt, split)
        fe, fr, th = _f64(disp, gt, split)
        assert c[i] == hn == len(th)
        host_own = max(_rel(he[:4], fe[:4]), _rel(hr, fr))
        bound = RTOL if host_own <= HOST_OWN else 4 * host_own
        dist = max(_rel(e[i][:4], he[:4]), _rel(r[i], hr))
        near = [int((np.abs(th / t - 1) <= BAND).sum()) for t in THRESHOLDS]
        delta = [abs(int(round(e[i][4 + k] * hn)) - int(round(he[4 + k] * hn))) for k in range(3)]
        print(f"[{split} {hw} vs {gt.shape}] n {hn}: device-host {dist:.3e}, host-f64 {host_own:.3e}, device-f64 "
              f"{max(_rel(e[i][:4], fe[:4]), _rel(r[i], fr)):.3e}, bound {bound:.1e}; a-count delta {delta}, near {near}")
        worst["device_vs_host"] = max(worst["device_vs_host"], dist)
        worst["host_vs_f64"] = max(worst["host_vs_f64"], host_own)
        worst["device_vs_f64"] = max(worst["device_vs_f64"], _rel(e[i][:4], fe[:4]), _rel(r[i], fr))
        worst["count_delta"] = max(worst["count_delta"], *delta)
        worst["count_allowed"] = max(worst["count_allowed"], *near)
        assert max(near) <= 1e-3 * hn, "fixture too loose: too many pixels sit on a threshold"
        assert dist <= bound
        for k in range(3):
            assert delta[k] <= near[k], (k, delta, near)
    # PPEA_PARITY_OUT=profiles pytest tests/test_eval_device_gpu.py -m gpu -k real_sizes   writes profiles/eval_device_parity.json
    out = os.environ.get("PPEA_PARITY_OUT")
    if out and os.path.isdir(out):
        path = os.path.join(out, "eval_device_parity.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.update(command="PPEA_PARITY_OUT=profiles pytest tests/test_eval_device_gpu.py -m gpu -k real_sizes",
                   metric="max over images of the relative distance of abs_rel, sq_rel, rmse, rmse_log and ratio; "
                          "count_delta = |a-count device - host| (pixels), count_allowed = pixels within 1e-5 of a threshold",
                   rule="device_vs_host <= 1e-5 (4 x host_vs_f64 where that exceeds 2.5e-6); count_delta <= count_allowed")
        doc.setdefault("fixtures", {})[f"{split} {hw[0]}x{hw[1]} vs {'/'.join('%dx%d' % s for s in sorted(set(gt_sizes)))}"] = worst
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)


# ---- 3. Trainer.val ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_predictor", [True, False])
def test_val_device_metrics_reproduce_host_metrics(device, golden, tmp_path, with_predictor):
    from ppeadepth import evaluate, networks, options
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.trainer import Trainer
    g = golden("eval")
    n, H, W, seed = [int(v) for v in g["val_meta"]]
    opt = options.default_options(height=H, width=W, batch_size=n, use_checkpoint=False)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model)
    model.to(device).train()
    synth.make_eval_split(str(tmp_path), n=n, height=H, width=W, seed=seed, split="eigen")
    ds = synth.SynthEigenDataset(str(tmp_path), split="eigen", height=H, width=W)
    batch, gt = synth.collate([ds[i] for i in range(n)]), ds.gt_depths()
    tr = Trainer(opt, model, device)
    p = DepthPredictor(model, opt, amp_dtype=None) if with_predictor else None
    host = tr.val([dict(batch)], gt, "eigen", predictor=p, metrics="host")
    assert model.training
    dev = tr.val([dict(batch)], gt, "eigen", predictor=p, metrics="device")
    assert model.training
    for name, d, h, gold in (("multi", dev[0], host[0], g["val_errors"]), ("mono", dev[1], host[1], g["val_errors_mono"])):
        print(f"[predictor={with_predictor}] {name}: device {d}\n    host {h}  rel {_rel(d, h):.3e}")
        assert d.shape == (7,) and d.dtype == np.float64
        assert _rel(d, h) <= RTOL
        assert abs(d[0] - float(gold[0])) <= 1e-3
    again = tr.val([dict(batch)], evaluate.DeviceGroundTruth(gt, device), "eigen", predictor=p, metrics="device")
    assert again[0].tobytes() == dev[0].tobytes() and again[1].tobytes() == dev[1].tobytes()
    # `freeze_tp` / hard_test_mono and `--disable_median_scaling`, `--pred_depth_scale_factor` mean what they meant
    tr.freeze_tp = True
    assert tr.val([dict(batch)], gt, "eigen", predictor=p, metrics="device").shape == (7,)
    tr.opt.disable_median_scaling, tr.opt.pred_depth_scale_factor = True, 1.3
    h2 = tr.val([dict(batch)], gt, "eigen", hard_test_mono=True, predictor=p, metrics="host")
    d2 = tr.val([dict(batch)], gt, "eigen", hard_test_mono=True, predictor=p, metrics="device")
    assert _rel(d2[0], h2[0]) <= RTOL and _rel(d2[1], h2[1]) <= RTOL
    assert _rel(d2[1], dev[1]) <= RTOL and _rel(d2[0][:4], dev[0][:4]) > 1e-3        # the teacher takes neither option


# ---- 4. determinism and launches -----------------------------------------------------------------------------------
LIBRARY = re.compile(r"Cijk_|igemm|ck::|ck_tile|miopen|MIOpen|gemm_|Gemm|rocblas|hipblaslt|rocprim|hipcub|cub::|sort|Sort|"
                     r"at::native|elementwise|reduce_kernel")


def _device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [(e.time_range.start, e.name) for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name]
    return [n for _, n in sorted(ev)]


def test_two_calls_agree_bitwise_and_the_launch_count_does_not_depend_on_the_batch(device):
    from ppeadepth import evaluate
    scenes = [_scene(20 + i, 48, 160, 375 - 5 * (i % 2), 1242 - 16 * (i % 2), 0.05) for i in range(12)]
    dg = evaluate.DeviceGroundTruth([g for _, g in scenes], device)
    pred = torch.from_numpy(np.stack([d for d, _ in scenes])).to(device)
    a = [t.clone() for t in dg.score(pred, 0, "eigen")]
    b = dg.score(pred, 0, "eigen")
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    assert not torch.isnan(a[0]).any() and int(a[2].min()) > 1000
    one = dg.score(pred[5:6], 5, "eigen")                               # an image scores the same alone as in a batch
    assert one[0].cpu().numpy().tobytes() == a[0][5:6].cpu().numpy().tobytes()
    n12 = _device_events(lambda: dg.score(pred, 0, "eigen"))
    n1 = _device_events(lambda: dg.score(pred[:1], 0, "eigen"))
    kernels = [n for n in n12 if "eval_" in n]
    print(f"one scored batch: {len(n12)} device events at B=12, {len(n1)} at B=1; kernels {len(kernels)}: {sorted(set(n12))}")
    assert len(kernels) == 7, "gather + 4 select passes + partial + final"
    assert len(n1) == len(n12) <= 8                                      # + the histogram memset
    assert not [n for n in n12 if LIBRARY.search(n)]


def test_val_copies_to_the_host_once_at_the_end_of_the_split(device, tmp_path):
    from torch.profiler import ProfilerActivity, profile
    from ppeadepth import evaluate, networks, options
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.trainer import Trainer
    n, H, W, B = 6, 64, 96, 2
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model)
    model.to(device).train()
    synth.make_eval_split(str(tmp_path), n=n, height=H, width=W, seed=3, split="eigen")
    ds = synth.SynthEigenDataset(str(tmp_path), split="eigen", height=H, width=W)
    batches = [{k: v.to(device) for k, v in synth.collate([ds[i] for i in range(j, j + B)]).items()} for j in range(0, n, B)]
    tr = Trainer(opt, model, device)
    p = DepthPredictor(model, opt, amp_dtype=None)
    gt = evaluate.DeviceGroundTruth(ds.gt_depths(), device)
    tr.val([dict(b) for b in batches], gt, "eigen", predictor=p, metrics="device")
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        tr.val([dict(b) for b in batches], gt, "eigen", predictor=p, metrics="device")
        torch.cuda.synchronize()
    ev = sorted((e.time_range.start, e.name) for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name)
    scoring = [t for t, name in ev if "eval_gather" in name or "eval_errors_final" in name]
    d2h = [t for t, name in ev if re.search(r"DtoH|Device -> (Pageable|Pinned|Host)", name)]
    print(f"val over {n // B} batches: {len(ev)} device events, {len(scoring)} scoring marks, device-to-host copies {len(d2h)}")
    assert len(scoring) == 2 * 2 * (n // B)                              # two networks, every batch scored as it is produced
    assert len(d2h) >= 1, "the copy of the result was not recognised: the name pattern is stale"
    assert not [t for t in d2h if scoring[0] <= t <= scoring[-1]]
    assert len(d2h) == 1 and d2h[0] > scoring[-1]


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def test_refusals(device):
    from ppeadepth import _abi, evaluate, ops
    scenes = [_scene(30 + i, 48, 160, 100, 300, 0.2) for i in range(3)]
    dg = evaluate.DeviceGroundTruth([g for _, g in scenes], device)
    pred = torch.from_numpy(np.stack([d for d, _ in scenes])).to(device)
    region = dg.max_region("eigen")
    ops.depth_errors(pred, dg.flat, dg.table, region)
    for bad in (pred.cpu(), pred.double(), pred.bfloat16(), pred.transpose(1, 2)):
        with pytest.raises(_abi.PpeaKernelError):
            ops.depth_errors(bad, dg.flat, dg.table, region)
    with pytest.raises(_abi.PpeaKernelError):
        ops.depth_errors(pred, dg.flat.cpu(), dg.table, region)
    with pytest.raises(_abi.PpeaKernelError):
        ops.depth_errors(pred, dg.flat.double(), dg.table, region)
    with pytest.raises(_abi.PpeaKernelError):
        ops.depth_errors(pred, dg.flat, dg.table.cpu(), region)
    with pytest.raises(_abi.PpeaKernelError):
        ops.depth_errors(pred, dg.flat, dg.table.int(), region)
    with pytest.raises(_abi.PpeaKernelError):
        ops.depth_errors(pred, dg.flat, dg.table[:2], region)              # a table for 2 images, a batch of 3
    with pytest.raises(_abi.PpeaKernelError):
        dg.score(pred, 1)                                                   # images 1..3 of a split of 3
    with pytest.raises(_abi.PpeaKernelError):
        evaluate.evaluate_disps_device(pred[:2], dg)
    # a table row that points outside the buffer scores nothing (NaN, count 0) instead of reading there
    table = dg.table.clone()
    table[1, 0] = dg.flat.numel() - 5
    e, _, c = ops.depth_errors(pred, dg.flat, table, region)
    assert int(c[1]) == 0 and torch.isnan(e[1]).all() and int(c[0]) > 0 and int(c[2]) > 0
    mean = evaluate.evaluate_disps_device(pred, dg, "eigen")
    host = evaluate.evaluate_disps(np.stack([d for d, _ in scenes]), [g for _, g in scenes], "eigen")
    assert mean.shape == (7,) and _rel(mean[:4], host[:4]) <= RTOL
