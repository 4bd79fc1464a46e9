"""The seeded inputs and references of tests/test_pose_trunk_gpu.py are fit to judge a kernel: the cases take the code
paths their comments name (plans restated from conv_image.hip / nhwc_bn.hip), planted kinds and ratios are present,
the fp32 and fp64 CPU references agree to 1e-5, the isolated-trunk oracle is RefRepDepth.pose_net itself, and the
bf16 floor file reproduces and stays under the caps.  No GPU needed."""
import math

import pytest
import torch

from conftest import rel_err
from oracle import pose_inputs as PI
from oracle import ref_model

REF_AGREE = 1e-5


# ---- A. image-fed convolution -------------------------------------------------------------------------------------------
def test_image_conv_cases_take_the_planned_paths():
    cases = PI.IMAGE_CONV_CASES
    # the weights the product passes, both output layouts for K = 3, an fp32 and a bf16 parameter per K
    assert {(K, Cout) for K, Cout, *_ in cases} == {(7, 64), (3, 128), (3, 64), (3, 72)}
    assert {nchw for K, _, _, nchw, _ in cases if K == 3} == {False, True}
    for K in (7, 3):
        assert {wdt for k, _, _, _, wdt in cases if k == K} == {"f32", "bf16"}
        assert {(1, 16, 32), (2, 18, 34), (3, 33, 47), (1, 2, 2)} <= {nhw for k, _, nhw, _, _ in cases if k == K}
    # img_plan as the issue reads it
    assert PI.img_plan(5, 64, 7, 48, 96) == (180, 146, 146)
    assert PI.img_plan(6, 128, 3, 48, 96) == (216, 170, 170)
    plans = {(K, Cout, nhw): PI.img_plan(nhw[0], Cout, K, PI.conv_out(nhw[1], K), PI.conv_out(nhw[2], K))
             for K, Cout, nhw, _, _ in cases}
    for K in (7, 3):
        assert any(n > s for (k, _, _), (n, _, s) in plans.items() if k == K)          # second trip of the patch loop
        assert any(n < want and s == n for (k, _, _), (n, want, s) in plans.items() if k == K)    # splits capped by n_patches
    assert plans[(7, 64, (1, 16, 32))][0] == 1 and plans[(7, 64, (2, 18, 34))][0] == 8 and plans[(7, 64, (3, 33, 47))][0] == 18
    # geometry: one exact tile; ragged row and column; odd sizes; one output pixel
    assert (PI.conv_out(16, 7), PI.conv_out(32, 7)) == (PI.TILE_H, PI.TILE_W) == (PI.conv_out(16, 3), PI.conv_out(32, 3))
    assert (PI.conv_out(18, 7), PI.conv_out(34, 7)) == (9, 17) and (PI.conv_out(33, 3), PI.conv_out(47, 3)) == (17, 24)
    assert PI.conv_out(2, 7) == 1 and PI.conv_out(2, 3) == 1
    assert 72 % 64 != 0 and 72 % 8 == 0


@pytest.mark.parametrize("case", PI.IMAGE_CONV_CASES, ids=[PI.case_id(c) for c in PI.IMAGE_CONV_CASES])
def test_image_conv_reference_fp32_agrees_with_fp64(case):
    K, Cout, nhw, _, _ = case
    img, w, go = PI.image_conv_case(K, Cout, nhw)
    assert float(img.min()) >= 0 and float(img.max()) <= 1 and w.shape == (Cout, 6 if K == 7 else 3, K, K)
    assert torch.equal(go, go.bfloat16().float()) and not torch.equal(w, w.bfloat16().float())
    y64, dw64 = PI.image_conv_reference(img, w, go)
    y32, dw32 = PI.image_conv_reference(img, w, go, torch.float32)
    assert y64.shape == go.shape and dw64.shape == w.shape
    assert rel_err(y32, y64) < REF_AGREE and rel_err(dw32, dw64) < REF_AGREE
    assert torch.equal(img, PI.image_conv_case(K, Cout, nhw)[0])                      # seeded


# ---- B. nhwc_bn_act -----------------------------------------------------------------------------------------------------
def test_bn_shapes_take_the_planned_paths():
    plan = {s: PI.bn_plan((s[0] // s[4]) * s[2] * s[3], s[1]) for s in PI.BN_SHAPES}
    rl, want, rows, slabs = plan[(2, 8, 3, 5, 1, False)]
    assert rl == 256 and 30 < rl and slabs == 1
    assert plan[(2, 2048, 1, 1, 1, False)][0] == 1                                   # one row lane
    assert plan[(1, 2048, 47, 45, 1, False)] == (1, 265, 9, 235)                     # cap taken; launched count re-derived
    rl, want, rows, slabs = plan[(1, 2048, 47, 46, 1, False)]
    assert want > PI.BN_MAX_SLABS and slabs == 241 and 47 * 46 - (slabs - 1) * rows == 2        # ... last slab ragged
    rl, want, rows, slabs = plan[(2, 64, 130, 257, 1, False)]
    assert (rl, want, rows, slabs) == (32, 262, 262, 256) and 66820 - 255 * rows == 10
    assert {s[1] for s in PI.BN_SHAPES} >= {8, 64, 128, 512, 2048} and {s[4] for s in PI.BN_SHAPES} == {1, 2, 3}
    assert any(s[5] for s in PI.BN_SHAPES)
    for s in PI.BN_SHAPES:
        assert s[0] % s[4] == 0 and 256 % (s[1] // 8) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PI.BN_SHAPES, ids=[PI.case_id(s) for s in PI.BN_SHAPES])
def test_bn_reference_fp32_agrees_with_fp64(shape, dtype):
    groups = shape[4]
    c = PI.bn_case(shape, dtype)
    if dtype == torch.bfloat16:
        for k in ("x", "res", "go"):
            assert c[k] is None or torch.equal(c[k], c[k].bfloat16().float())
    r64 = PI.bn_reference(c, groups)
    r32 = PI.bn_reference(c, groups, dtype=torch.float32)
    for k in ("y", "running_mean", "running_var", "dres", "dweight", "dbias"):
        if r64[k] is not None:
            assert rel_err(r32[k], r64[k]) < REF_AGREE, k
    P = (shape[0] // groups) * shape[2] * shape[3]
    assert PI.dx_err(r32["dx"], r64, REF_AGREE, cancelling=P <= 4) < 1        # P = 2: dx vanishes but for eps
    assert [sh for sh in PI.BN_SHAPES if (sh[0] // sh[4]) * sh[2] * sh[3] <= 4] == [(2, 2048, 1, 1, 1, False)]
    # the ReLU works on both sides, and the cotangent was cleared on few elements
    open_share = float((r64["y"] > 0).double().mean())
    assert 0.2 < open_share < 0.8
    assert float(c["near_zero"].double().mean()) < 0.01
    assert float((c["go"] == 0)[~c["near_zero"]].double().mean()) < 0.01
    if groups > 1:                      # the sub-batches differ, so the order of the running-statistics updates shows
        m = c["x"].double().view(groups, -1, *c["x"].shape[1:]).mean((1, 3, 4))
        assert float((m[0] - m[-1]).abs().max()) > 1e-2


@pytest.mark.parametrize("case", PI.LARGE_MEAN_CASES, ids=[PI.case_id(c) for c in PI.LARGE_MEAN_CASES])
def test_bn_large_mean_case_holds_the_planted_ratios(case):
    C, N, H, W = case
    c = PI.bn_large_mean_case(case)
    rl, want, rows, slabs = PI.bn_plan(N * H * W, C)
    assert rl == {16: 128, 64: 32}[C]                                                # row lanes: above / at the fp32 chain limit
    assert (N * H * W, slabs, rows) in ((6000, 6, 1000), (6000, 24, 250), (66820, 256, 262))
    x = c["x"].double()
    assert x.shape == (N, C, H, W)
    mean, std = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False).sqrt()
    ratio = mean.abs() / std
    want = torch.tensor(PI.LARGE_MEAN_RATIOS, dtype=torch.float64).repeat(C // 4)
    assert bool(((ratio - want).abs() <= 0.05 * want + 0.05).all()), ratio
    assert bool((mean > 0).any()) and bool((mean < 0).any())
    r64 = PI.bn_reference(c, 1, act=0)
    r32 = PI.bn_reference(c, 1, act=0, dtype=torch.float32)
    assert rel_err(r32["y"], r64["y"]) < REF_AGREE
    assert float(PI.large_mean_bound(mean, std ** 2).max()) < 4e-3


# ---- C. maxpool3x3s2 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PI.POOL_SHAPES, ids=[PI.case_id(s) for s in PI.POOL_SHAPES])
def test_pool_cases_hold_the_planted_kinds(shape, dtype):
    N, C, H, W = shape
    x, _ = PI.pool_case(shape, "negative", dtype)
    assert bool((x < 0).all())
    x, _ = PI.pool_case(shape, "constant", dtype)
    assert bool((x == x[:, :, :1, :1]).all()) and (N * C == 1 or x[:, :, 0, 0].unique().numel() > 1)
    x, _ = PI.pool_case(shape, "signed_zero", dtype)
    assert bool((x == 0).all())
    neg = torch.signbit(x)
    assert bool(neg.any()) and bool((~neg).any())
    if W > 1:
        assert bool((neg[..., :, 1:] != neg[..., :, :-1]).all())
    if H > 1:
        assert bool((neg[..., 1:, :] != neg[..., :-1, :]).all())
    x, _ = PI.pool_case(shape, "neg_inf", dtype)
    assert bool(torch.isinf(x[0, 0]).all()) and bool((x[torch.isinf(x)] < 0).all()) and not bool(torch.isnan(x).any())
    if x.numel() > 64:
        assert bool(torch.isfinite(x).any())
    x, _ = PI.pool_case(shape, "nan", dtype)
    assert torch.isnan(x).flatten(1).sum(1).tolist() == [1] * N


@pytest.mark.parametrize("kind", PI.POOL_KINDS)
def test_pool_reference_fp32_agrees_with_fp64(kind):
    for shape in PI.POOL_SHAPES:
        x, go = PI.pool_case(shape, kind, torch.float32)
        y32, dx32 = PI.pool_reference(x, go)
        y64, dx64 = PI.pool_reference(x.double(), go.double())
        assert y32.shape == go.shape
        assert torch.allclose(y32.double(), y64, rtol=0, atol=0, equal_nan=(kind == "nan"))
        assert torch.equal(torch.signbit(y32), torch.signbit(y64))
        assert rel_err(dx32, dx64) < REF_AGREE and bool(torch.isfinite(dx32).all())          # up to four windows: fp32 sum
        assert torch.equal(dx32 != 0, dx64 != 0)
        if kind == "constant":          # every window a tie: the first element in scan order takes the gradient
            took = dx32 != 0
            assert bool(took[:, :, 0, 0].all()) and not bool(took[:, :, 2::2, :].any()) and not bool(took[:, :, :, 2::2].any())


# ---- D. the trunk in isolation ------------------------------------------------------------------------------------------
def test_trunk_inputs_are_what_they_claim():
    sd = PI.trunk_state()
    bn_w = torch.cat([v for k, v in sd.items() if ".bn" in k and k.endswith(".weight") and v.dim() == 1])
    assert 0.05 < float(bn_w.std()) < 0.2 and abs(float(bn_w.mean()) - 1) < 0.05
    rm = torch.cat([v for k, v in sd.items() if k.endswith("running_mean")])
    rv = torch.cat([v for k, v in sd.items() if k.endswith("running_var")])
    assert float(rm.std()) > 0.02 and float(rv.min()) >= 1.0 and float(rv.std()) > 0.01
    enc, dec = PI.split_state(sd)
    assert "encoder.conv1.weight" in enc and enc["encoder.conv1.weight"].shape == (64, 6, 7, 7)
    assert dec["net.3.weight"].shape == (12, 256, 1, 1) and len(enc) + len(dec) == len(sd)
    for H, W, _ in PI.TRUNK_CONFIGS[::2]:
        p = PI.trunk_pairs(H, W)
        assert p.shape == (PI.TRUNK_PAIRS, 6, H, W) and float(p.min()) >= 0 and float(p.max()) <= 1
        assert torch.equal(p, PI.trunk_pairs(H, W))
        d = p - p.mean((2, 3), keepdim=True)
        corr = (d[..., :, 1:] * d[..., :, :-1]).mean() / (d * d).mean()
        assert float(corr) > 0.8                                                     # image-like: neighbours alike
        assert float((p[:, :3] - p[:, 3:]).abs().mean()) > 0.01                      # two different frames
    ca, ct = PI.trunk_cotangent()
    assert ca.shape == ct.shape == (PI.TRUNK_PAIRS, 2, 1, 3)
    assert [(h // 32, w // 32) for h, w, _ in PI.TRUNK_CONFIGS] == [(2, 3), (2, 3), (2, 3), (2, 3)]


def test_trunk_oracle_is_ref_pose_net():
    """PoseRef.pose_net_feats without rounding == RefRepDepth.pose_net, bit for bit in fp64: outputs, every gradient, every
    running statistic and counter; the ragged size has the deep maps 9x13, 5x7, 3x4."""
    H, W, groups = 72, 104, 2
    a = PI.trunk_reference(H, W, groups)
    b = PI.trunk_reference(H, W, groups, plain=True)
    assert isinstance(PI.PoseRef({}, PI.TRUNK_OPT), ref_model.RefRepDepth)
    assert set(a) - set(b) == set(PI.FEATURE_KEYS)
    for k, v in b.items():
        assert torch.equal(a[k], v), k
    assert [tuple(a[k].shape[2:]) for k in PI.FEATURE_KEYS] == [(36, 52), (18, 26), (9, 13), (5, 7), (3, 4)]
    assert all(int(v) == groups for k, v in a.items() if k.endswith("num_batches_tracked"))
    n = sum(a[k].numel() for k in a if k.startswith("grad."))
    assert 12.4e6 < n < 12.7e6
    assert all(float(a[k].abs().max()) > 0 for k in a if k.startswith("grad."))
    # one pass over the whole batch is a different computation: the reference really is per sub-batch
    c = PI.trunk_reference(H, W, 1)
    assert rel_err(c["axisangle"], a["axisangle"]) > 1e-3


@pytest.mark.parametrize("cfg", PI.TRUNK_CONFIGS, ids=[PI.config_name(c) for c in PI.TRUNK_CONFIGS])
def test_trunk_has_no_gate_near_a_tie_and_fp32_agrees_with_fp64(cfg):
    """With the stored nudges no ReLU input of the fp64 oracle lies within MARGIN of zero and no max-pool window has its two
    largest values within MARGIN of each other (one flipped gate moves a gradient entry by 100 %); the nudges are small;
    and the same oracle in fp32 then agrees with fp64 on every compared tensor -- without them it does not."""
    probes = PI.trunk_probes(cfg)
    assert len(probes) == 1 + 1 + 16 + 3 and [s for s, _ in probes].count("pool") == 1
    for site, t in probes:
        assert float(PI.site_margins(site, t).min()) >= PI.MARGIN, site
        if site != "pool":
            assert 0.02 < float((t > 0).double().mean()) < 0.98, site                # the gate opens and closes
    nudges = PI.load_floor()["nudges"][PI.config_name(cfg)]
    assert 0 < len(nudges) < 200 and all(abs(d) <= 1e-2 for _, _, d in nudges)
    r64 = PI.trunk_reference(*cfg)
    r32 = PI.trunk_reference(*cfg, dtype=torch.float32)
    for k, v in r64.items():
        if v.is_floating_point():
            assert rel_err(r32[k], v) < 1e-4, k
    if cfg == (64, 96, 2):              # the same inputs without the nudges: two gates within fp32 rounding of zero
        a, b = PI.trunk_reference(*cfg, nudges=()), PI.trunk_reference(*cfg, dtype=torch.float32, nudges=())
        assert max(rel_err(b[k], a[k]) for k in a if a[k].is_floating_point()) > 1e-3


@pytest.mark.parametrize("cfg", PI.TRUNK_CONFIGS, ids=[PI.config_name(c) for c in PI.TRUNK_CONFIGS])
def test_bf16_floor_file_reproduces_and_is_under_the_caps(cfg):
    """tests/golden/pose_trunk_bf16_floor.json is what oracle.pose_inputs.generate_floor writes, for every compared key.
    The outputs, the five features and the running statistics are conditioned well enough to judge a kernel tightly:
    1 - cos <= 0.02 and rel_err <= 0.2 between the bf16-rounded and the fp64 oracle.  The 68 parameter gradients
    mostly are not (see the next test); their stored floors stay below 0.25 in 1 - cos, so band() holds every one of
    them below the 0.5 the e2e test allows."""
    stored = PI.load_floor()["floor"][PI.config_name(cfg)]
    now = PI.bf16_floor(cfg)
    assert set(stored) == set(now) and {"axisangle", "translation", *PI.FEATURE_KEYS} <= set(now)
    assert sum("running_" in k for k in now) == 40 and sum(k.startswith("grad.") for k in now) == 68
    for k, (rel, cos) in now.items():
        assert math.isclose(rel, stored[k][0], rel_tol=1e-3, abs_tol=1e-12), k
        assert math.isclose(cos, stored[k][1], rel_tol=1e-3, abs_tol=1e-12), k
        assert rel > 0                                                               # the rounding reached every key
        if k.startswith("grad."):
            assert cos <= 0.25 and PI.band(rel, cos)[1] <= PI.COS_CEILING, (k, rel, cos)
        else:
            assert PI.well_conditioned(rel, cos), (k, rel, cos)
    assert PI.band(0.1, 0.01) == (0.2 + 1e-6, 0.04 + 1e-6) and PI.band(0.7, 0.2)[1] == 0.5


@pytest.mark.parametrize("n,H,W", [(16, 64, 96), (4, 128, 192)], ids=["16_pairs", "128x192"])
def test_bf16_gradient_floor_does_not_come_under_the_caps_with_more_pairs_or_a_larger_map(n, H, W):
    """Why most gradient keys carry band() of their own floor and not the caps: four times the pairs, or four times the map,
    leave the bf16-rounded oracle's gradients where they are (median 1 - cos 0.07-0.09; at most 10 of 68 keys under the
    caps).  The cotangent's scale cannot matter: every gradient is linear in it, rel_err and 1 - cos are ratios."""
    fl = PI.bf16_floor((H, W, 1), nudges=(), n=n)
    g = sorted(v[1] for k, v in fl.items() if k.startswith("grad."))
    assert len(g) == 68 and g[34] > 2 * PI.CAP_COS
    assert sum(PI.well_conditioned(*v) for k, v in fl.items() if k.startswith("grad.")) <= 12
    assert all(PI.well_conditioned(*v) for k, v in fl.items() if not k.startswith("grad."))
