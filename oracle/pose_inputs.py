"""TEST INFRASTRUCTURE ONLY -- seeded inputs, cases and fp64 references for the pose network's kernels (conv_image.hip,
nhwc_bn.hip, nhwc_pool.hip) and for the trunk in isolation (ResNet-18 + PoseDecoder against RefRepDepth.pose_net).
Pure torch on the CPU; everything is a function of its arguments and the seed.  tests/test_pose_trunk_cpu.py proves
the properties the GPU test (tests/test_pose_trunk_gpu.py) relies on."""
import functools
import json
import os
import types

import torch
import torch.nn.functional as F

from . import model_spec, ref_model, synth

FLOOR_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                          "pose_trunk_bf16_floor.json")


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def bf16_round(t):
    return t.float().bfloat16().to(t.dtype)


# ---------------------------------------------------------------------------------------------
# A. image-fed convolution (conv_image.hip), forward and weight gradient
# ---------------------------------------------------------------------------------------------
TILE_H, TILE_W = 8, 16          # conv_image.hip TH, TW


def img_plan(N, Cout, K, Ho, Wo):
    """conv_image.hip img_plan(): (n_patches, uncapped splits, splits) of the weight-gradient launch."""
    n_patches = -(-Wo // TILE_W) * -(-Ho // TILE_H) * N
    coutp = -(-Cout // 64) * 64
    kp = (K * 8 + 31) // 32 * 32
    wk = 4 // (2 * (kp // 32))
    per_slab = K * coutp * kp * 4
    want = min(512 // (coutp // 64), (16 << 20) // (per_slab * wk))
    return n_patches, want, max(1, min(want, n_patches))


def img_ws_bytes(N, Cout, K, Ho, Wo):
    """conv_image.hip img_plan().ws_bytes: [splits * WK][K][CoutP][KP] fp32."""
    kp = (K * 8 + 31) // 32 * 32
    return K * (-(-Cout // 64) * 64) * kp * 4 * img_plan(N, Cout, K, Ho, Wo)[2] * (4 // (2 * (kp // 32)))


def case_id(case):
    return "-".join("x".join(str(v) for v in f) if isinstance(f, tuple) else str(f) for f in case)


def conv_out(n, K):
    return (n + 2 * (K // 2) - K) // 2 + 1


# (K, Cout, (N, H, W), out_nchw, weight dtype).  Cin = 6 for K = 7 (pose conv1), 3 for K = 3 (stem[0]); pad = K // 2.
# img_plan: K = 7, Cout 64 -> at most 146 splits; K = 3, Cout 128 or 72 -> 170; K = 3, Cout 64 -> 341.
IMAGE_CONV_CASES = [
    (7, 64, (1, 16, 32), False, "f32"),      # exactly one 8x16 output tile; 1 patch: splits capped 146 -> 1
    (7, 64, (2, 18, 34), False, "bf16"),     # one ragged output row and column; 8 patches: splits 146 -> 8
    (7, 64, (3, 33, 47), False, "f32"),      # odd sizes; 18 patches: splits 146 -> 18
    (7, 64, (1, 2, 2), False, "f32"),        # one output pixel, all-padding halo; splits 1
    (7, 64, (5, 96, 192), False, "f32"),     # 180 patches > 146 splits: second trip of the patch loop for 34 blocks
    (3, 128, (2, 18, 34), True, "f32"),      # 8 patches: splits 170 -> 8
    (3, 128, (3, 33, 47), False, "bf16"),    # 18 patches: splits 18
    (3, 128, (1, 2, 2), False, "f32"),       # splits 1
    (3, 128, (6, 96, 192), True, "f32"),     # 216 patches > 170 splits: second trip for 46 blocks
    (3, 64, (1, 16, 32), False, "f32"),      # the 64-column forward tile; splits 341 -> 1
    (3, 64, (3, 33, 47), True, "bf16"),      # splits 341 -> 18
    (3, 72, (2, 18, 34), False, "f32"),      # Cout no multiple of the 128-column tile nor of 64; splits 170 -> 8
    (3, 72, (3, 33, 47), True, "f32"),       # splits 170 -> 18
]


def image_conv_case(K, Cout, nhw, seed=0):
    """-> img [N,Cin,H,W] in [0,1] fp32, w [Cout,Cin,K,K] fp32 (not pre-rounded), go [N,Cout,Ho,Wo] on the bf16 grid."""
    N, H, W = nhw
    Cin = 6 if K == 7 else 3
    g = _gen(seed + 1000 * K + Cout + 7 * N + H * W)
    img = torch.rand(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) / (Cin * K * K) ** 0.5
    go = bf16_round(torch.randn(N, Cout, conv_out(H, K), conv_out(W, K), generator=g))
    return img, w, go


def image_conv_reference(img, w, go, dtype=torch.float64):
    """F.conv2d on the operands the kernel sees: ((img - 0.45) / 0.225) and w rounded to bf16 -> (y, dw)."""
    K = w.shape[-1]
    x = ((img - 0.45) / 0.225).bfloat16().to(dtype)
    wr = w.bfloat16().to(dtype).requires_grad_(True)
    y = F.conv2d(x, wr, None, 2, K // 2)
    y.backward(go.to(dtype))
    return y.detach(), wr.grad


# ---------------------------------------------------------------------------------------------
# B. nhwc_bn_act edges (nhwc_bn.hip)
# ---------------------------------------------------------------------------------------------
BN_TPB, BN_V, BN_MAX_SLABS = 256, 8, 256


def bn_plan(P, C):
    """nhwc_bn.hip plan_slabs(): (row lanes, slabs before the cap, rows per slab, slabs launched)."""
    rl = BN_TPB // (C // BN_V)
    want = max(1, -(-P // (rl * 8)))
    slabs = min(want, BN_MAX_SLABS)
    rows = -(-P // slabs)
    return rl, want, rows, -(-P // rows)


# (N, C, H, W, groups, residual)
BN_SHAPES = [
    (2, 8, 3, 5, 1, False),          # 1 channel thread, 256 row lanes, P = 30 < RL
    (4, 128, 5, 7, 2, False),        # layer2 width
    (6, 512, 2, 3, 3, False),        # layer4 width, three sub-batches: running-statistics order
    (2, 2048, 1, 1, 1, False),       # P = 2, one row lane
    (1, 2048, 47, 45, 1, False),     # P = 2115: 265 slabs wanted, cap taken, rows 9 -> 235 slabs launched (9 * 235 = P)
    (1, 2048, 47, 46, 1, False),     # P = 2162: cap taken, rows 9 -> 241 slabs, the last one ragged (2 rows)
    (2, 64, 130, 257, 1, False),     # P = 66820: the cap at the real conv1 width, rows 262 -> 256 slabs, last one ragged
    (4, 64, 9, 13, 2, True),         # with residual
]
RELU_MARGIN = 1e-3                   # the cotangent is zero where |u| is below this: the ReLU mask cannot differ there


def bn_case(shape, dtype, seed=0):
    """-> dict x, res (or None), weight, bias, running_mean, running_var, go; x / res / go on the grid of `dtype`."""
    N, C, H, W, groups, has_res = shape
    g = _gen(seed + C + 31 * groups + H * W)
    cast = (lambda t: t) if dtype == torch.float32 else bf16_round
    z = torch.randn(N, C, H, W, generator=g)
    P = (N // groups) * H * W
    if P <= 4:      # a handful of samples: spread them (two nearly equal ones leave x - mean to fp32 cancellation, eps to rule)
        lad = (torch.arange(P, dtype=torch.float32) - (P - 1) / 2).view(1, N // groups, 1, H, W).expand(groups, -1, C, -1, -1)
        sign = torch.where(torch.rand(groups, 1, C, 1, 1, generator=g) < 0.5, -1.0, 1.0)
        z = (lad * sign * (1 + torch.rand(groups, 1, C, 1, 1, generator=g))).reshape(N, C, H, W)
    x = cast(z * (0.5 + torch.rand(1, C, 1, 1, generator=g)) + 0.5 * torch.randn(1, C, 1, 1, generator=g))
    res = cast(torch.randn(N, C, H, W, generator=g)) if has_res else None
    go = cast(torch.randn(N, C, H, W, generator=g))
    c = dict(x=x, res=res, weight=torch.rand(C, generator=g) + 0.5, bias=torch.randn(C, generator=g) * 0.2,
             running_mean=0.3 * torch.randn(C, generator=g), running_var=0.5 + torch.rand(C, generator=g), go=go)
    u = bn_reference(c, groups, act=0, dtype=torch.float64)["y"]
    c["go"] = torch.where(u.abs() < RELU_MARGIN, torch.zeros(()), go)
    c["near_zero"] = u.abs() < RELU_MARGIN
    return c


def bn_reference(c, groups, act=1, dtype=torch.float64, eps=1e-5, momentum=0.1):
    """F.batch_norm per sub-batch in order (+ residual, ReLU) under autograd -> y, running_mean, running_var, dx, dres,
    dweight, dbias, var [groups, C] (biased batch variance of every sub-batch)."""
    leaf = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)
    x, res, w, b = leaf(c["x"]), leaf(c["res"]), leaf(c["weight"]), leaf(c["bias"])
    rm, rv = c["running_mean"].to(dtype).clone(), c["running_var"].to(dtype).clone()
    outs, var = [], []
    for i, xc in enumerate(x.chunk(groups, 0)):
        u = F.batch_norm(xc, rm, rv, w, b, True, momentum, eps)
        if res is not None:
            u = u + res.chunk(groups, 0)[i]
        outs.append(F.relu(u) if act == 1 else u)
        var.append(xc.detach().var((0, 2, 3), unbiased=False))
    y = torch.cat(outs, 0)
    (y * c["go"].to(dtype)).sum().backward()
    var = torch.stack(var)
    # dx = a (g - mean g - xhat mean(g xhat)) is a difference of terms of size a |g|, which fp32 carries to 2^-24 each:
    # where it cancels (P = 2: dx vanishes but for eps) a comparison has to allow DX_SLACK of that size
    terms = float((c["weight"].to(dtype).abs() / (var + eps).sqrt()).max() * c["go"].abs().max())
    return dict(y=y.detach(), running_mean=rm, running_var=rv, dx=x.grad, dres=None if res is None else res.grad,
                dweight=w.grad, dbias=b.grad, var=var, dx_terms=terms)


DX_SLACK = 1e-6         # x dx_terms, absolute


def dx_err(dx, ref, tol, cancelling=False):
    """max |dx - ref| over its allowance tol * max |ref| (<= 1: within tolerance); cancelling (P <= 4): the allowance
    also holds DX_SLACK * dx_terms."""
    r = ref["dx"].double()
    return float((dx.double() - r).abs().max() / (tol * r.abs().max() + (DX_SLACK * ref["dx_terms"] if cancelling else 0.0)))


LARGE_MEAN_RATIOS = (1.0, 10.0, 30.0, 100.0)
# (C, N, H, W): P = 6000 with 128 row lanes (their sum taken in double) and with the 32 of the conv1 width (fp32);
# the conv1 width at the MAX_SLABS cap (P = 66820: 256 slabs of 262 rows)
LARGE_MEAN_CASES = [(16, 2, 50, 60), (64, 2, 50, 60), (64, 2, 130, 257)]


def bn_large_mean_case(case, seed=0):
    """fp32 x [N,C,H,W] whose channel c has |mean| / std close to LARGE_MEAN_RATIOS[c % 4] (sign alternating)."""
    C, N, H, W = case
    g = _gen(seed + 77 + C - 16 + (H * W - 3000))
    std = 0.5 + torch.rand(1, C, 1, 1, generator=g)
    ratio = torch.tensor(LARGE_MEAN_RATIOS).repeat(C // 4).view(1, C, 1, 1)
    sign = torch.where(torch.arange(C) % 8 < 4, 1.0, -1.0).view(1, C, 1, 1)
    x = (torch.randn(N, C, H, W, generator=g) + sign * ratio) * std
    return dict(x=x, res=None, weight=torch.rand(C, generator=g) + 0.5, bias=torch.randn(C, generator=g) * 0.2,
                running_mean=torch.zeros(C), running_var=torch.ones(C), go=torch.randn(N, C, H, W, generator=g))


def large_mean_bound(mean, var):
    """Bound on the relative variance error of E[x^2] - mean^2 from fp32 partials combined in fp64."""
    return 3e-7 * (1 + mean ** 2 / var) + 1e-6


# ---------------------------------------------------------------------------------------------
# C. maxpool3x3s2 edges (nhwc_pool.hip)
# ---------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 8, 1, 1), (2, 8, 1, 7), (2, 8, 7, 1), (1, 16, 2, 2), (3, 24, 5, 6)]      # (N, C, H, W)
POOL_KINDS = ("negative", "constant", "signed_zero", "neg_inf", "nan")


def pool_case(shape, kind, dtype, seed=0):
    """-> (x [N,C,H,W], go [N,C,Ho,Wo]) of `dtype`.  negative: every value < 0; constant: one value per (n, c) plane;
    signed_zero: +0 / -0 checkerboard (its phase alternating with the channel); neg_inf: random values with about half
    the entries -inf, item 0 / channel 0 entirely -inf; nan: random values and one NaN per image."""
    N, C, H, W = shape
    g = _gen(seed + 13 * POOL_KINDS.index(kind) + C * H * W + N)
    x = torch.randn(N, C, H, W, generator=g)
    if kind == "negative":
        x = -0.1 - x.abs()
    elif kind == "constant":
        x = torch.randn(N, C, 1, 1, generator=g).expand(N, C, H, W).clone()
    elif kind == "signed_zero":
        par = (torch.arange(H).view(1, 1, H, 1) + torch.arange(W).view(1, 1, 1, W) + torch.arange(C).view(1, C, 1, 1)) % 2
        x = torch.where(par.expand(N, C, H, W) == 0, torch.tensor(0.0), torch.tensor(-0.0))
    elif kind == "neg_inf":
        x = torch.where(torch.rand(N, C, H, W, generator=g) < 0.5, torch.tensor(float("-inf")), x)
        x[0, 0] = float("-inf")
    elif kind == "nan":
        flat = x.view(N, -1)
        pos = torch.randint(0, flat.shape[1], (N,), generator=g)
        flat[torch.arange(N), pos] = float("nan")
    go = torch.randn(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=g)
    return x.to(dtype).contiguous(), go.to(dtype)


def pool_reference(x, go):
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    y.backward(go.to(x.dtype))
    return y.detach(), xr.grad


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


# ---------------------------------------------------------------------------------------------
# D. the trunk in isolation: ResnetEncoder(18, False, num_input_images=2) + PoseDecoder(num_ch_enc, 1, 2)
# ---------------------------------------------------------------------------------------------
TRUNK_PAIRS = 4
TRUNK_CONFIGS = [(64, 96, 1), (64, 96, 2), (72, 104, 1), (72, 104, 2)]       # (H, W, groups); 72x104: every stride-2 layer ragged
TRUNK_OPT = types.SimpleNamespace(rep_size="b", use_checkpoint=False)
FEATURE_KEYS = tuple(f"feature.{i}" for i in range(5))
COTANGENT_SCALE = 100.0              # outputs carry the decoder's 0.01


def config_name(cfg):
    return "%dx%d_g%d" % cfg


MARGIN = 5e-5               # no ReLU input of the fp64 oracle is closer to zero, no max-pool window's two largest are closer
NUDGE_FILTER_SEED = 97


def trunk_state(cfg=None, nudges=None):
    """state_dict (reference keys: pose_encoder.encoder.*, pose.net.*) from oracle.synth's filler: BN weights 1 +- 0.1,
    biases and running means +-0.05, running variances in [1, 1.1].  With a TRUNK_CONFIGS entry: plus that
    configuration's nudges (find_nudges; stored in the floor file), which keep every ReLU and max-pool decision of the
    oracle MARGIN away from a tie -- one flipped gate moves a gradient entry by 100 %, so without them two fp32
    evaluations of this very oracle disagree by 5 % on a tensor or two in every other configuration."""
    sd = {k: synth.synth_tensor(k, torch.empty(shape, dtype=dt))
          for k, (shape, dt) in model_spec.state_spec("b").items() if k.startswith(("pose_encoder.", "pose."))}
    if cfg is not None and nudges is None:
        nudges = load_floor()["nudges"][config_name(cfg)]
    for key, c, delta in nudges or ():
        if sd[key].dim() == 1:
            sd[key][c] += delta
        else:                           # a conv1 filter: moved along a fixed random direction
            sd[key][c] += delta * torch.randn(sd[key][c].shape, generator=_gen(NUDGE_FILTER_SEED + c))
    return sd


def split_state(sd):
    """-> (ResnetEncoder state_dict, PoseDecoder state_dict)"""
    enc = {k[len("pose_encoder."):]: v for k, v in sd.items() if k.startswith("pose_encoder.")}
    dec = {k[len("pose."):]: v for k, v in sd.items() if k.startswith("pose.")}
    return enc, dec


def trunk_pairs(H, W, n=TRUNK_PAIRS, seed=0):
    """[n, 6, H, W] in [0, 1]: a smooth texture and the same texture shifted by a few pixels with a little
    noise (two neighbouring frames), per pair."""
    g = _gen(seed + H * W)
    k = torch.ones(3, 1, 7, 7) / 49.0
    tex = F.conv2d(torch.rand(n, 3, H + 14, W + 14, generator=g), k, groups=3)          # [B,3,H+8,W+8]
    tex = (tex - tex.amin((1, 2, 3), keepdim=True)) / (tex.amax((1, 2, 3), keepdim=True) - tex.amin((1, 2, 3), keepdim=True))
    a = tex[:, :, 4:4 + H, 4:4 + W]
    shifts = ((0, 3), (1, -2), (-2, 1), (2, 4))
    b = torch.stack([tex[i, :, 4 + dy:4 + dy + H, 4 + dx:4 + dx + W] for i, (dy, dx) in enumerate(shifts[j % 4] for j in range(n))])
    b = (b + 0.02 * torch.randn(b.shape, generator=g)).clamp(0, 1)
    return torch.cat([a, b], 1).contiguous()


def trunk_cotangent(n=TRUNK_PAIRS, seed=0):
    """Fixed cotangent on (axisangle, translation), both [n, 2, 1, 3]."""
    g = _gen(seed + 5)
    return (COTANGENT_SCALE * torch.randn(n, 2, 1, 3, generator=g),
            COTANGENT_SCALE * torch.randn(n, 2, 1, 3, generator=g))


class _RoundBoth(torch.autograd.Function):
    """bf16 rounding of an activation and, on the way back, of its gradient (both are bf16 tensors in the product)."""

    @staticmethod
    def forward(ctx, x):
        return bf16_round(x)

    @staticmethod
    def backward(ctx, g):
        return bf16_round(g)


class _RoundFwd(torch.autograd.Function):
    """bf16 rounding of a weight as a conv reads it; its gradient goes to the fp32 parameter unrounded."""

    @staticmethod
    def forward(ctx, x):
        return bf16_round(x)

    @staticmethod
    def backward(ctx, g):
        return g


class PoseRef(ref_model.RefRepDepth):
    """RefRepDepth.pose_net that also returns the five encoder features and, with `bf16`, rounds to bf16 where the
    product's bf16 step does: the normalised frame pair, conv weights, conv outputs, the output of every fused
    BatchNorm (+ residual + ReLU) launch, the two spatial means and the 0.01 scaling.  Without `bf16` it is
    RefRepDepth.pose_net operation for operation (the CPU test compares the two bit for bit)."""
    bf16 = False
    probe = None            # or a list that receives (bias key | "pool", tensor) at every ReLU input and at the max-pool input

    def _r(self, x):
        return _RoundBoth.apply(x) if self.bf16 else x

    def _w(self, key):
        return _RoundFwd.apply(self.sd[key]) if self.bf16 else self.sd[key]

    def _relu(self, u, bias_key):
        if self.probe is not None:
            self.probe.append((bias_key, u.detach()))
        return F.relu(u)

    def _block(self, x, p, stride, down):
        out = self._r(F.conv2d(x, self._w(p + ".conv1.weight"), None, stride, 1))
        out = self._r(self._relu(self._rbn(out, p + ".bn1"), p + ".bn1.bias"))
        out = self._rbn(self._r(F.conv2d(out, self._w(p + ".conv2.weight"), None, 1, 1)), p + ".bn2")
        if down:
            x = self._r(F.conv2d(x, self._w(p + ".downsample.0.weight"), None, stride))
            x = self._r(self._rbn(x, p + ".downsample.1"))
        return self._r(self._relu(out + x, p + ".bn2.bias"))

    def pose_net_feats(self, pair):
        sd, p = self.sd, "pose_encoder.encoder"
        x = self._r((pair - 0.45) / 0.225)
        x = self._r(F.conv2d(x, self._w(p + ".conv1.weight"), None, 2, 3))
        x = self._r(self._relu(self._rbn(x, p + ".bn1"), p + ".bn1.bias"))
        feats = [x]
        if self.probe is not None:
            self.probe.append(("pool", x.detach()))
        x = F.max_pool2d(x, 3, 2, 1)
        for li, stride in ((1, 1), (2, 2), (3, 2), (4, 2)):
            x = self._block(x, f"{p}.layer{li}.0", stride, li > 1)
            x = self._block(x, f"{p}.layer{li}.1", 1, False)
            feats.append(x)
        for i in range(3):
            x = self._r(self._relu(F.conv2d(x, self._w(f"pose.net.{i}.weight"), sd[f"pose.net.{i}.bias"], 1, min(i, 1)),
                                   f"pose.net.{i}.bias"))
        x = self._r(F.conv2d(x, self._w("pose.net.3.weight"), sd["pose.net.3.bias"]))
        out = self._r(0.01 * self._r(self._r(x.mean(3)).mean(2)).reshape(-1, 2, 1, 6))
        return out[..., :3], out[..., 3:], feats


def grad_keys(sd):
    return [k for k, v in sd.items() if v.is_floating_point() and "running_" not in k and ".fc." not in k]


def trunk_probes(cfg, nudges=None):
    """[(site, tensor)] of the fp64 oracle's ReLU inputs and max-pool input, the sub-batches concatenated."""
    H, W, groups = cfg
    ref = PoseRef({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in trunk_state(cfg, nudges).items()}, TRUNK_OPT)
    runs = []
    with torch.no_grad():
        for chunk in trunk_pairs(H, W).double().chunk(groups, 0):
            ref.probe = []
            ref.pose_net_feats(chunk)
            runs.append(ref.probe)
    return [(site, torch.cat([r[i][1] for r in runs])) for i, (site, _) in enumerate(runs[0])]


def site_margins(site, t):
    """Per channel: the smallest |u| of a ReLU input; for the max-pool input the smallest gap between the two largest
    values of a window whose maximum is positive (below it the ReLU before the pool has zeroed the gradient)."""
    if site != "pool":
        return t.abs().transpose(0, 1).flatten(1).min(1)[0]
    N, C, H, W = t.shape
    win = F.unfold(F.pad(t, (1, 1, 1, 1), value=-1.0).reshape(N * C, 1, H + 2, W + 2), 3, stride=2)     # [N*C, 9, L]
    top = win.topk(2, dim=1)[0]
    gap = torch.where(top[:, 0] > 0, top[:, 0] - top[:, 1], torch.ones(()).double())
    return gap.reshape(N, C, -1).transpose(0, 1).flatten(1).min(1)[0]


def find_nudges(cfg, max_sweeps=200):
    """Front to back: at the first site with a channel inside MARGIN, move that channel's bias (a uniform shift of its
    ReLU inputs; training-mode BN statistics do not see it) by the smallest multiple of 3 MARGIN that clears it, or for
    the max-pool move the conv1 filter; later sites are looked at again after every change."""
    nudges = []
    for _ in range(max_sweeps):
        for site, t in trunk_probes(cfg, nudges):
            m = site_margins(site, t)
            bad = (m < MARGIN).nonzero().flatten().tolist()
            if not bad:
                continue
            for c in bad:
                if site == "pool":
                    nudges.append(["pose_encoder.encoder.conv1.weight", c, 1e-3])
                    continue
                u = t[:, c].flatten()
                for k in range(1, 1000):
                    delta = 3 * MARGIN * ((k + 1) // 2) * (1 if k % 2 else -1)
                    if float((u + delta).abs().min()) >= 2 * MARGIN:
                        break
                nudges.append([site, c, delta])
            break
        else:
            return nudges
    raise RuntimeError("no margin found")


def trunk_reference(H, W, groups, bf16=False, dtype=torch.float64, plain=False, nudges=None, n=TRUNK_PAIRS):
    """The oracle on a `dtype` copy of trunk_state(), once per sub-batch in order (the running statistics see the
    sub-batches one after the other) -> dict: axisangle, translation, feature.0-4, grad.<key>, <key> for every running
    statistic and num_batches_tracked.  plain: through RefRepDepth.pose_net itself (no features); nudges: instead of the
    stored ones (() for none); n: pairs in the batch."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in trunk_state((H, W, groups), nudges).items()}
    keys = grad_keys(sd)
    for k in keys:
        sd[k].requires_grad_(True)
    ref = PoseRef(sd, TRUNK_OPT)
    ref.bf16 = bf16
    pairs = trunk_pairs(H, W, n).to(dtype)
    ca, ct = (t.to(dtype) for t in trunk_cotangent(n))
    aas, tts, feats = [], [], []
    for chunk in pairs.chunk(groups, 0):
        if plain:
            aa, tt = ref.pose_net(chunk)
        else:
            aa, tt, f = ref.pose_net_feats(chunk)
            feats.append(f)
        aas.append(aa)
        tts.append(tt)
    aa, tt = torch.cat(aas), torch.cat(tts)
    ((aa * ca).sum() + (tt * ct).sum()).backward()
    out = {"axisangle": aa.detach(), "translation": tt.detach()}
    for i in range(5 if feats else 0):
        out[f"feature.{i}"] = torch.cat([f[i] for f in feats]).detach()
    for k in keys:
        out["grad." + k] = sd[k].grad
    for k, v in sd.items():
        if "running_" in k or k.endswith("num_batches_tracked"):
            if ".fc." not in k:
                out[k] = v.detach()
    return out


CAP_REL, CAP_COS = 0.2, 0.02         # floors up to these: the key is conditioned well enough for the tight band to mean much
COS_CEILING = 0.5                    # what tests/test_e2e_gpu.py allows the pose gradients; no band here is looser


def band(floor_rel, floor_cos):
    """(rel_err, 1 - cos) a bf16 execution may show on a key whose bf16-rounded oracle shows (floor_rel, floor_cos): the
    kernels' accumulation order is an independent second noise of the emulation's size (2x), 1 - cos goes with its
    square (4x), + 1e-6; 1 - cos never above COS_CEILING."""
    return 2 * floor_rel + 1e-6, min(4 * floor_cos + 1e-6, COS_CEILING)


def well_conditioned(floor_rel, floor_cos):
    return floor_rel <= CAP_REL and floor_cos <= CAP_COS


def forward_keys(ref):
    """The outputs, the five features and the running statistics of a trunk_reference() result."""
    return [k for k, v in ref.items() if v.is_floating_point() and not k.startswith("grad.")]


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def one_minus_cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(1 - (a @ b) / (a.norm() * b.norm() + 1e-300))


def bf16_floor(cfg, nudges=None, n=TRUNK_PAIRS):
    """{key: [rel_err, 1 - cos]} of the bf16-rounded oracle against the fp64 oracle for one TRUNK_CONFIGS entry, every
    compared key.  The outputs, features and running statistics are well_conditioned(); most parameter gradients are
    not (ReLU and max-pool decisions that flip under the forward rounding put them at 1 - cos of 0.05 to 0.15), with
    more pairs or a larger map as with these (tests/test_pose_trunk_cpu.py), so they are held to band() of their own floor."""
    H, W, groups = cfg
    ref = trunk_reference(H, W, groups, nudges=nudges, n=n)
    emu = trunk_reference(H, W, groups, bf16=True, nudges=nudges, n=n)
    return {k: [rel_err(emu[k], ref[k]), one_minus_cos(emu[k], ref[k])] for k in ref if ref[k].is_floating_point()}


def generate_floor(path=FLOOR_PATH):
    """Writes tests/golden/pose_trunk_bf16_floor.json: {"nudges": {config: [[key, channel, delta], ...]},
    "floor": {config: {key: [rel_err, 1 - cos]}}}; the nudges first, the floor is measured on the nudged state."""
    data = {"nudges": {config_name(cfg): find_nudges(cfg) for cfg in TRUNK_CONFIGS}, "floor": {}}
    _write(path, data)
    data["floor"] = {config_name(cfg): bf16_floor(cfg) for cfg in TRUNK_CONFIGS}
    _write(path, data)
    return data


def _write(path, data):
    load_floor.cache_clear()
    with open(path, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)
        f.write("\n")


@functools.lru_cache(maxsize=None)
def load_floor(path=FLOOR_PATH):
    with open(path) as f:
        return json.load(f)


if __name__ == "__main__":
    generate_floor()
