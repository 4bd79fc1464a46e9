"""`Trainer.val_ddad`'s protocol on the device (MODE_DDAD of csrc/eval_metrics.hip through `evaluate.DeviceGroundTruth`,
`evaluate_disps_device(..., "val_ddad")`, `Trainer.val_ddad(metrics="device")`) against the host statement
`evaluate.evaluate_image_ddad` and a float64 restatement written below, and `DDADInputPipeline(backend="hip")` against
backend "torch".  Inputs are seeded and synthetic."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-5              # the bound between two statements of a protocol (tests/test_eval_device_gpu.py:16)
BAND = 1e-5              # a1..a3 may differ only by pixels whose max(gt/pred, pred/gt) lies this close to a threshold
THRESHOLDS = (1.25, 1.5625, 1.953125)
LO, HI = np.float32(1e-3), np.float32(200.0)


def _scene(seed, h, w, gh, gw, keep):
    """-> (scaled disparity [h,w] fp32, ground truth [gh,gw] fp32 with 0 = no return); depths from 8 m to beyond 200 m."""
    g = torch.Generator().manual_seed(seed)
    def field(H, W):
        y = torch.linspace(0, 1, H)[:, None]
        x = torch.linspace(0, 1, W)[None, :]
        return 8 + 230 * (1 - y) ** 2 + 3 * torch.sin(7 * x + seed) * y + 2 * torch.cos(5 * y * x)      # >= 3
    depth = field(h, w) * (1 + 0.08 * torch.randn(h, w, generator=g)).clamp(0.5, 1.5) * 1.7
    gt = field(gh, gw) * (1 + 0.12 * torch.randn(gh, gw, generator=g)).clamp(0.5, 1.5)
    gt = gt * (torch.rand(gh, gw, generator=g) < keep)
    return (1 / depth).float().numpy(), gt.float().numpy()


def _mask(gt):
    return np.logical_and(gt > 1e-3, gt < 200)


def _host(disp, gt, median_scaling=True, scale=1.0):
    """The host path: (7 errors fp64 array, ratio, valid count); an empty mask gives NaN without numpy's warnings."""
    from ppeadepth import evaluate
    n = int(_mask(gt).sum())
    if n == 0:
        return np.full(7, np.nan), np.float32(np.nan), 0
    e, r = evaluate.evaluate_image_ddad(disp, gt, median_scaling, scale)
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


def _f64(disp, gt, median_scaling=True, scale=1.0):
    """The protocol restated in float64 -> (7 errors, ratio, thresh array)."""
    pred = _resize_f64(1 / disp.astype(np.float64), *gt.shape)
    mask = _mask(gt)
    pred, g = pred[mask] * scale, gt[mask].astype(np.float64)
    ratio = np.median(g) / np.median(pred)
    if median_scaling:
        pred = pred * ratio
    pred = np.clip(pred, np.float64(LO), 200.0)
    th = np.maximum(g / pred, pred / g)
    e = [np.mean(np.abs(g - pred) / g), np.mean((g - pred) ** 2 / g), np.sqrt(np.mean((g - pred) ** 2)),
         np.sqrt(np.mean((np.log(g) - np.log(pred)) ** 2))] + [np.mean(th < t) for t in THRESHOLDS]
    return np.array(e), ratio, th


def _score(dg, device, disps, first, median_scaling=True, scale=1.0):
    pred = torch.from_numpy(np.stack(disps)).to(device)
    e, r, c = dg.score(pred, first, "val_ddad", median_scaling, scale)
    torch.cuda.synchronize()
    return e.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy()


def _rel(a, b):
    """max |a - b| / |b|; equal entries count as 0 (also 0 against 0), a difference from 0 as inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(d == 0, 0.0, d / np.abs(b))))


def _with_parity(gt, want_odd):
    gt = gt.copy()
    if (int(_mask(gt).sum()) % 2 == 1) != want_odd:
        ys, xs = np.nonzero(_mask(gt))
        gt[ys[-1], xs[-1]] = 0
    assert (int(_mask(gt).sum()) % 2 == 1) == want_odd
    return gt


# ---- 1. exact where it can be exact --------------------------------------------------------------------------------
SAME_SIZES = [(5, 7), (32, 64), (38, 61)]      # less than one 2048-pixel chunk, exactly one, a partial last chunk


def _same_size_group(k, gh, gw):
    """Four images of one size: odd valid count, no valid pixel, even valid count, one valid pixel.  The two full images
    hold ground truth of exactly 200.0 and exactly float32(1e-3) (both excluded), values in every class, and predictions
    whose scaled depth leaves [1e-3, 200] on either side."""
    out = []
    for j, want_odd in enumerate((True, False)):
        disp, gt = _scene(40 + 10 * k + j, gh, gw, gh, gw, 0.6)
        gt[0, 0], gt[0, 1], gt[1, 0], gt[1, 1] = HI, LO, 150.0, 230.0
        gt[2, 0], gt[2, 1] = 20.0, 60.0
        disp[2, 0], disp[2, 1] = 1e5, 1e-4                     # depth 1e-5 m and 1e4 m at two scored pixels
        out.append((disp, _with_parity(gt, want_odd)))
    one = np.zeros((gh, gw), np.float32)
    one[gh // 2, gw // 2] = 90.0                               # a single return, beyond val's 80 m
    return [out[0], (out[0][0], np.zeros((gh, gw), np.float32)), out[1], (out[1][0], one)]


@pytest.mark.parametrize("median_scaling,scale", [(True, 1.0), (False, 1.07), (True, 1.3)])
def test_same_size_prediction_is_exact_against_the_host_path(device, median_scaling, scale):
    """A prediction of the ground truth's own size: the resize is the identity in both statements and 1 / x is IEEE division,
    so ratio, valid count and a1..a3 are EQUAL and the continuous errors agree within 1e-5.  The ground truth is one ragged
    buffer of 5x7, 32x64 and 38x61 maps; a call takes predictions of ONE size, so the buffer is scored in three calls, each
    over the four consecutive maps of a size (the empty and the one-pixel map among them)."""
    from ppeadepth import evaluate
    groups = [_same_size_group(k, gh, gw) for k, (gh, gw) in enumerate(SAME_SIZES)]
    dg = evaluate.DeviceGroundTruth([g for grp in groups for _, g in grp], device)
    clamped_low = clamped_high = False
    for k, grp in enumerate(groups):
        e, r, c = _score(dg, device, [d for d, _ in grp], 4 * k, median_scaling, scale)
        for i, (disp, gt) in enumerate(grp):
            he, hr, hn = _host(disp, gt, median_scaling, scale)
            print(f"[{SAME_SIZES[k]} ms={median_scaling} x{scale}] image {i}: n {c[i]} / {hn}, ratio {r[i]!r} / {hr!r}, "
                  f"device {e[i]}, host {he}")
            assert c[i] == hn
            if hn == 0:
                assert np.isnan(e[i]).all() and np.isnan(r[i])
                continue
            m = _mask(gt)
            assert not m[0, 0] and not m[0, 1] and (i == 3 or (m[1, 0] and not m[1, 1]))      # 200.0, 1e-3f out; 150 in
            if median_scaling:
                assert np.float32(r[i]).tobytes() == np.float32(hr).tobytes()
            assert (e[i][4:] == he[4:]).all(), (e[i][4:], he[4:])
            assert _rel(e[i][:4], he[:4]) <= RTOL
            p = (1 / disp)[m] * np.float32(scale) * (np.float32(hr) if median_scaling else np.float32(1))
            clamped_low, clamped_high = clamped_low or bool((p < LO).any()), clamped_high or bool((p > HI).any())
        assert [int(v) % 2 for v in c] == [1, 0, 0, 1] and c[3] == 1
        # the images around the empty one are what they are alone
        for i in (0, 2):
            alone = _score(dg, device, [grp[i][0]], 4 * k + i, median_scaling, scale)
            assert alone[0][0].tobytes() == e[i].tobytes() and alone[2][0] == c[i]
            assert np.float32(alone[1][0]).tobytes() == np.float32(r[i]).tobytes()
    assert clamped_low and clamped_high, "the fixture no longer reaches both clamps"


# ---- 2. non-integer size ratios ------------------------------------------------------------------------------------
RATIOS = [((24, 40), (76, 121), 3, 0.3), ((384, 640), (1216, 1936), 2, 0.01)]


@pytest.mark.parametrize("hw,gt_hw,B,keep", RATIOS)
def test_non_integer_ratios_against_host_and_float64(device, hw, gt_hw, B, keep):
    """Continuous errors and ratio within rtol 1e-5 of the host path; a1..a3 differ from the host by at most the number of
    pixels within relative 1e-5 of the threshold in the float64 restatement, and the fixture keeps that number <= 0.1 % of
    the valid pixels."""
    from ppeadepth import evaluate
    scenes = [_scene(60 + i, hw[0], hw[1], gt_hw[0], gt_hw[1], keep) for i in range(B)]
    dg = evaluate.DeviceGroundTruth([g for _, g in scenes], device)
    e, r, c = _score(dg, device, [d for d, _ in scenes], 0)
    worst = {"device_vs_host": 0.0, "host_vs_f64": 0.0, "device_vs_f64": 0.0, "count_delta": 0, "count_allowed": 0}
    for i, (disp, gt) in enumerate(scenes):
        he, hr, hn = _host(disp, gt)
        fe, fr, th = _f64(disp, gt)
        assert c[i] == hn == len(th)
        assert ((gt > 1e-3) & (gt < 80)).any() and ((gt >= 80) & (gt < 200)).any() and (gt >= 200).any()
        host_own = max(_rel(he[:4], fe[:4]), _rel(hr, fr))
        dist = max(_rel(e[i][:4], he[:4]), _rel(r[i], hr))
        dev_f64 = max(_rel(e[i][:4], fe[:4]), _rel(r[i], fr))
        near = [int((np.abs(th / t - 1) <= BAND).sum()) for t in THRESHOLDS]
        delta = [abs(int(round(e[i][4 + k] * hn)) - int(round(he[4 + k] * hn))) for k in range(3)]
        print(f"[{hw} vs {gt.shape}] n {hn}: device-host {dist:.3e}, host-f64 {host_own:.3e}, device-f64 {dev_f64:.3e}; "
              f"a-count delta {delta}, near {near}")
        worst["device_vs_host"] = max(worst["device_vs_host"], dist)
        worst["host_vs_f64"] = max(worst["host_vs_f64"], host_own)
        worst["device_vs_f64"] = max(worst["device_vs_f64"], dev_f64)
        worst["count_delta"] = max(worst["count_delta"], *delta)
        worst["count_allowed"] = max(worst["count_allowed"], *near)
        assert max(near) <= 1e-3 * hn, "fixture too loose: too many pixels sit on a threshold"
        assert dist <= RTOL
        for k in range(3):
            assert delta[k] <= near[k], (k, delta, near)
    # PPEA_PARITY_OUT=profiles pytest tests/test_val_ddad_gpu.py -m gpu -k non_integer   writes profiles/val_ddad_parity.json
    out = os.environ.get("PPEA_PARITY_OUT")
    if out and os.path.isdir(out):
        path = os.path.join(out, "val_ddad_parity.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.update(command="PPEA_PARITY_OUT=profiles pytest tests/test_val_ddad_gpu.py -m gpu -k non_integer",
                   metric="max over images of the relative distance of abs_rel, sq_rel, rmse, rmse_log and ratio; "
                          "count_delta = |a-count device - host| (pixels), count_allowed = pixels within 1e-5 of a threshold",
                   rule="device_vs_host <= 1e-5; count_delta <= count_allowed")
        doc.setdefault("fixtures", {})[f"{hw[0]}x{hw[1]} vs {gt_hw[0]}x{gt_hw[1]} B={B}"] = worst
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)


# ---- 3. determinism, launches, refusal -----------------------------------------------------------------------------
def _device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [(e.time_range.start, e.name) for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name]
    return [n for _, n in sorted(ev)]


def test_two_calls_agree_bitwise_and_an_image_scores_alone_as_in_a_batch(device):
    from ppeadepth import evaluate
    scenes = [_scene(80 + i, 24, 40, 76 - 3 * (i % 2), 121 - 4 * (i % 2), 0.3) for i in range(5)]
    dg = evaluate.DeviceGroundTruth([g for _, g in scenes], device)
    pred = torch.from_numpy(np.stack([d for d, _ in scenes])).to(device)
    a = [t.clone() for t in dg.score(pred, 0, "val_ddad")]
    b = dg.score(pred, 0, "val_ddad")
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    assert not torch.isnan(a[0]).any() and int(a[2].min()) > 1000
    one = dg.score(pred[3:4], 3, "val_ddad")
    assert all(x.cpu().numpy().tobytes() == y[3:4].cpu().numpy().tobytes() for x, y in zip(one, a))
    # not the 80 m range test, which the name "ddad" still selects
    assert int((dg.score(pred, 0, "ddad")[2] < a[2]).sum()) == 5
    n5 = _device_events(lambda: dg.score(pred, 0, "val_ddad"))
    n1 = _device_events(lambda: dg.score(pred[:1], 0, "val_ddad"))
    kernels = [n for n in n5 if "eval_" in n]
    print(f"one scored batch: {len(n5)} device events at B=5, {len(n1)} at B=1; kernels {sorted(set(n5))}")
    assert len(kernels) == 7 and len(n1) == len(n5) <= 8          # gather + 4 select + partial + final, + the memset
    mean = evaluate.evaluate_disps_device(pred, dg, "val_ddad", batch=2)
    host = evaluate.evaluate_disps_ddad(pred.cpu().numpy(), [g for _, g in scenes])
    assert mean.shape == (7,) and _rel(mean[:4], host[:4]) <= RTOL


def test_mode_4_is_refused_through_the_c_abi(device):
    from ppeadepth import _abi, evaluate
    disp, gt = _scene(90, 24, 40, 76, 121, 0.3)
    dg = evaluate.DeviceGroundTruth([gt], device)
    pred = torch.from_numpy(disp[None]).to(device)
    region = dg.max_region("val_ddad")
    assert region == 76 * 121
    errors = torch.zeros(1, 7, device=device, dtype=torch.float64)
    ratio = torch.zeros(1, device=device)
    count = torch.zeros(1, device=device, dtype=torch.int32)
    ws = torch.empty(_abi.lib.ppea_depth_errors_workspace_bytes(1, region), device=device, dtype=torch.uint8)

    def run(mode):
        return _abi.lib.ppea_depth_errors_f32(_abi.ptr(pred), _abi.ptr(dg.flat), dg.flat.numel(), _abi.ptr(dg.table),
                                              _abi.ptr(ws), _abi.ptr(errors), _abi.ptr(ratio), _abi.ptr(count), 1, 24, 40,
                                              region, mode, 1, ctypes.c_float(1.0), _abi.stream_ptr())
    for mode in (4, 5, 1 << 20, -1):
        assert run(mode) == -1                                  # PPEA_ERR_UNSUPPORTED, nothing launched
    torch.cuda.synchronize()
    assert int(count[0]) == 0 and float(errors.abs().sum()) == 0
    assert run(3) == 0
    torch.cuda.synchronize()
    assert int(count[0]) == int(_mask(gt).sum())


# ---- 4. Trainer.val_ddad -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ddad_val(device):
    """A small synthetic DDAD validation set through the pipeline: model, trainer, two batches of two."""
    from ppeadepth import networks, options
    from ppeadepth.input_pipeline import DDADInputPipeline
    from ppeadepth.trainer import Trainer
    H, W, raw_hw, B = 64, 96, (203, 305), 2
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, frame_ids=[0, -1])
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model)
    model.to(device).train()
    items = synth.make_ddad_val(4, raw_hw, seed=3, valid=0.05)
    pipe = DDADInputPipeline(device, H, W, raw_hw)
    batches = []
    for j in range(0, 4, B):
        raw, intr, depth = synth.collate_ddad(items[j:j + B])
        data = pipe(raw, intr)
        data["depth"] = depth
        batches.append(data)
    for it in items:
        d = it["depth"]
        assert ((d > 1e-3) & (d < 80)).any() and ((d >= 80) & (d < 200)).any() and (d >= 200).any() and (d == 0).mean() > 0.9
    return opt, model, Trainer(opt, model, device), batches, items


@pytest.mark.parametrize("with_predictor", [True, False])
def test_val_ddad_device_metrics_reproduce_host_metrics(device, ddad_val, with_predictor):
    from ppeadepth import evaluate
    from ppeadepth.inference import DepthPredictor
    opt, model, tr, batches, items = ddad_val
    p = DepthPredictor(model, opt, amp_dtype=None) if with_predictor else None
    fresh = lambda on_device=False: [{k: (v.to(device) if on_device else v) for k, v in b.items()} for b in batches]  # noqa: E731
    tr.freeze_tp = False
    tr.opt.disable_median_scaling, tr.opt.pred_depth_scale_factor = False, 1.0
    host = tr.val_ddad(fresh(), predictor=p, metrics="host")
    assert model.training
    dev = tr.val_ddad(fresh(), predictor=p, metrics="device")
    assert model.training
    for name, d, h in (("multi", dev[0], host[0]), ("mono", dev[1], host[1])):
        print(f"[predictor={with_predictor}] {name}: device {d}\n    host {h}  rel {_rel(d, h):.3e}")
        assert d.shape == (7,) and d.dtype == np.float64 and np.isfinite(d).all()
        assert _rel(d, h) <= RTOL
    # the ground truth on the device already, or given for the whole set: the same bits
    gts = [it["depth"] for it in items]
    for again in (tr.val_ddad(fresh(True), predictor=p, metrics="device"),
                  tr.val_ddad(fresh(), gts, predictor=p, metrics="device"),
                  tr.val_ddad(fresh(), evaluate.DeviceGroundTruth(gts, device), predictor=p, metrics="device")):
        assert again[0].tobytes() == dev[0].tobytes() and again[1].tobytes() == dev[1].tobytes()
    assert _rel(tr.val_ddad(fresh(), gts, predictor=p)[0], host[0]) == 0
    # not `val`'s protocol under the name "ddad"
    other = tr.val(fresh(), gts, "ddad", predictor=p, metrics="device")
    assert _rel(other[0][:4], dev[0][:4]) > 1e-3
    # `freeze_tp` / hard_test_mono, `--disable_median_scaling`, `--pred_depth_scale_factor`; the teacher takes neither
    tr.freeze_tp = True
    assert tr.val_ddad(fresh(), predictor=p, metrics="device").shape == (7,)
    tr.opt.disable_median_scaling, tr.opt.pred_depth_scale_factor = True, 1.3
    try:
        h2 = tr.val_ddad(fresh(), hard_test_mono=True, predictor=p, metrics="host")
        d2 = tr.val_ddad(fresh(), hard_test_mono=True, predictor=p, metrics="device")
    finally:
        tr.freeze_tp = False
        tr.opt.disable_median_scaling, tr.opt.pred_depth_scale_factor = False, 1.0
    assert _rel(d2[0], h2[0]) <= RTOL and _rel(d2[1], h2[1]) <= RTOL
    assert d2[1].tobytes() == dev[1].tobytes() and _rel(d2[0][:4], dev[0][:4]) > 1e-3


def test_val_ddad_copies_to_the_host_once_at_the_end(device, ddad_val):
    from torch.profiler import ProfilerActivity, profile
    from ppeadepth.inference import DepthPredictor
    opt, model, tr, batches, _ = ddad_val
    p = DepthPredictor(model, opt, amp_dtype=None)
    fresh = lambda: [{k: v.to(device) for k, v in b.items()} for b in batches]      # noqa: E731  (depth on the device too)
    tr.val_ddad(fresh(), predictor=p, metrics="device")
    torch.cuda.synchronize()
    data = fresh()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        tr.val_ddad(data, predictor=p, metrics="device")
        torch.cuda.synchronize()
    ev = sorted((e.time_range.start, e.name) for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name)
    scoring = [t for t, name in ev if "eval_gather" in name or "eval_errors_final" in name]
    d2h = [t for t, name in ev if re.search(r"DtoH|Device -> (Pageable|Pinned|Host)", name)]
    h2d = [t for t, name in ev if re.search(r"HtoD|(Pageable|Pinned|Host) -> Device", name)]
    print(f"val_ddad over {len(batches)} batches: {len(ev)} device events, {len(scoring)} scoring marks, "
          f"device-to-host copies {len(d2h)}, host-to-device copies {len(h2d)}")
    assert len(scoring) == 2 * 2 * len(batches)                         # two networks, every batch scored as it is produced
    assert len(d2h) >= 1, "the copy of the result was not recognised: the name pattern is stale"
    assert not [t for t in d2h if scoring[0] <= t <= scoring[-1]]
    assert len(d2h) == 1 and d2h[0] > scoring[-1]


# ---- 5. the loader's image path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw_hw,hw,B", [((50, 77), (16, 24), 3), ((1216, 1936), (384, 640), 2)])
def test_ddad_pipeline_backends_return_the_same_bytes(device, raw_hw, hw, B):
    from ppeadepth.input_pipeline import DDADInputPipeline
    items = synth.make_ddad_val(B, raw_hw, seed=5)
    raw, intr, _ = synth.collate_ddad(items)
    raw[-1][0, :, : raw_hw[0] // 3] = 255
    raw[0][-1] = torch.randint(0, 256, raw[0][-1].shape, generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    hip = DDADInputPipeline(device, hw[0], hw[1], raw_hw)
    assert hip.backend == "hip"
    a = hip(raw, intr)
    b = DDADInputPipeline(device, hw[0], hw[1], raw_hw, backend="torch")(raw, intr)
    c = DDADInputPipeline("cpu", hw[0], hw[1], raw_hw)(raw, intr)
    assert set(a) == set(b) == set(c) and len(a) == 2 * 2 * 4 + 2 * 4
    for k in a:
        assert a[k].dtype == torch.float32 and a[k].device.type == "cuda"
        assert torch.equal(a[k], b[k]) and torch.equal(a[k].cpu(), c[k]), k
    assert tuple(a[("color", -1, 3)].shape) == (B, 3, hw[0] // 8, hw[1] // 8)
    assert torch.equal(a[("K", 0)], a[("K", 3)]) and not torch.equal(a[("K", 0)][0], a[("K", 0)][1])
