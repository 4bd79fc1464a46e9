"""TEST INFRASTRUCTURE ONLY -- case tables, seeded inputs, float64 references and per-element error bounds for the dense
convolution kernels (csrc/conv_nhwc.hip, csrc/conv_wgrad.hip) behind ops.conv2d_nhwc / conv_module / conv_transpose_module.
Pure torch on the CPU; everything is a function of its arguments and the seed.  Which kernel a row reaches is NOT restated
here: the rows name the arm they claim and tests/test_conv_arms_cpu.py asks the library's own plan queries
(ops.conv_nhwc_plan / ops.conv_wgrad_plan, the functions the launches go by) whether they do.  That file also proves
the other properties the GPU test (tests/test_conv_arms_gpu.py) relies on.

THE BOUND (derived, not tuned).  The kernels multiply bf16 operands exactly (8 x 8 bit significands fit fp32), add the
products in fp32 in some order, and round the sum once to the output type.  For a sum of n terms with magnitude sum
A = sum |a_i b_i|, any order of fp32 additions, rounding or truncating, is within n * 2^-23 * A of the exact sum (2^-23: the
unit error of a truncating adder; the guides document the fp32 MFMA as an fmaf chain and say nothing of the bf16 one).  One
round-to-nearest to bf16 adds at most 2^-8 of the value (half an ulp of an 8-bit significand, reached just above a power of
two: the bound is sharp, and correct kernels come close to it), so

    bf16 output:  |got - ref| <= 2^-8 |ref| + (1 + 2^-8) * n * 2^-23 * A
    fp32 output:  |got - ref| <=              (1 + 2^-8) * n * 2^-23 * A

n = Cin k k (forward), Cout k k (data gradient), N Ho Wo (weight and bias gradient).  Every element is held to its own bound.
"""
import collections

import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8          # one round-to-nearest to bf16, relative
U_ACC = 2.0 ** -23          # one fp32 addition, rounding or truncating, relative
ACTS = ("none", "relu", "elu", "sigmoid")
# activated outputs: the band tests/test_pose_trunk_gpu.py holds such layers to (the fast exponential of the epilogue)
ACT_REL, ACT_ABS = 2.0 ** -7, 1e-3

Case = collections.namedtuple("Case", "name N Cin H W Cout k stride pad reflect act bias nchw wdtype arm")
# bias: None | "f32" | "bf16"; wdtype: dtype of the weight parameter and so of its gradient ("f32" | "bf16")
# arm: what the row claims (see each table)


def _c(name, shape, k, stride=1, pad=None, reflect=False, act="none", bias=None, nchw=False, wdtype="bf16", arm=None):
    N, Cin, H, W, Cout = shape
    return Case(name, N, Cin, H, W, Cout, k, stride, k // 2 if pad is None else pad, reflect, act, bias, nchw, wdtype, arm)


def tile(BN, stride, k, nchw=False, rps=1):
    """conv_nhwc_kernel<BN, ., ., stride, nchw, k, rps>"""
    return ("tile", BN, stride, k, int(nchw), rps)


def resident(NTC):
    """conv3x3_resident_kernel<NTC, 1>"""
    return ("resident", NTC)


def arm_of_plan(plan, stride, k, nchw):
    """The arm tuple of an ops.conv_nhwc_plan result."""
    if plan["NTC"]:
        return resident(plan["NTC"])
    return tile(plan["BN"], stride, k, nchw, plan["RPS"])


# every arm ppea_conv_nhwc_bf16 can launch: 40 per-tile instantiations + 3 persistent ones
ALL_FWD_ARMS = frozenset(
    [tile(BN, s, k, nchw, rps) for BN in (32, 64, 128) for s in (1, 2) for k in (1, 3, 7) for nchw in (0, 1)
     for rps in (1, 3) if not (BN == 128 and k == 7) and (rps == 1 or (k == 3 and BN <= 64))]
    + [resident(n) for n in (1, 2, 4)])
# conv_wgrad_kernel<stride, k, BM, BN>
ALL_WGRAD_ARMS = frozenset((s, k, bm, bn) for s in (1, 2) for k in (1, 3, 7) for bm in (32, 64) for bn in (32, 64))
SPLIT_RULES = ("want", "cap", "floor", "fill", "patches")


# ---------------------------------------------------------------------------------------------
# what ops passes to the entry points (ops._ConvNhwc / ops._ConvTransposeNhwc); the GPU test checks these against the
# recorded calls
# ---------------------------------------------------------------------------------------------
def out_hw(c):
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def cout8(c):
    """conv2d_nhwc runs a layer whose output channel count is no multiple of 8 zero-padded to the next one."""
    return (c.Cout + 7) // 8 * 8


def launch_args(c):
    """-> dict(fwd, dgrad: argument tuples of ops.conv_nhwc_plan; wgrad: of ops.conv_wgrad_plan) of a conv2d_nhwc row."""
    Ho, Wo = out_hw(c)
    Co = cout8(c)
    fwd = (c.N, c.H, c.W, c.Cin, Co, c.k, c.stride, c.pad, int(c.reflect), 1, Ho, Wo, int(c.nchw))
    if c.reflect:       # full correlation onto the padded domain, folded back by ppea_nhwc_reflect_pad1_bwd_bf16
        dgrad = (c.N, Ho, Wo, Co, c.Cin, c.k, 1, c.k - 1, 0, c.stride, Ho + c.k - 1, Wo + c.k - 1, 0)
    else:
        dgrad = (c.N, Ho, Wo, Co, c.Cin, c.k, 1, c.k - 1 - c.pad, 0, c.stride, c.H, c.W, 0)
    return dict(fwd=fwd, dgrad=dgrad, wgrad=(c.N, c.Cin, Co, c.k, c.stride, Ho, Wo))


def transpose_out_hw(c):
    return (c.H - 1) * 2 - 2 + 3 + 1, (c.W - 1) * 2 - 2 + 3 + 1


def transpose_launch_args(c):
    """ConvTranspose2d(Cin, Cout, 3, 2, 1, output_padding=1): its forward is the dilated data-gradient form, its data
    gradient a stride-2 forward, its weight gradient that conv's with the two activations exchanged."""
    Ho, Wo = transpose_out_hw(c)
    return dict(fwd=(c.N, c.H, c.W, c.Cin, c.Cout, 3, 1, 1, 0, 2, Ho, Wo, 0),
                dgrad=(c.N, Ho, Wo, c.Cout, c.Cin, 3, 2, 1, 0, 1, c.H, c.W, 0),
                wgrad=(c.N, c.Cout, c.Cin, 3, 2, c.H, c.W))


# ---------------------------------------------------------------------------------------------
# case tables.  Shapes are (N, Cin, H, W, Cout).
# ---------------------------------------------------------------------------------------------
# per-tile rows: (BN, rps) -> stride -> shape.  BN = 64 needs Cout > 32 and >= 256 workgroups of 64 channels, BN = 128 Cout > 64,
# >= 512 workgroups of 128 channels and (3 x 3) fewer than 256 input channels; the whole 3 x 3 weight slice per step
# (rps 3) needs >= 256 input channels.  Odd extents: Ho % TR, Wo % TC, Cout % BN, Cin % 32 all non-zero, N > 1 where it is cheap.
_FWD_SHAPES = {
    (32, 1): {1: (2, 40, 5, 7, 24), 2: (2, 40, 9, 13, 24)},
    (32, 3): {1: (1, 264, 5, 7, 24), 2: (1, 264, 9, 13, 24)},
    (64, 1): {1: (1, 8, 63, 255, 72), 2: (2, 8, 61, 253, 200)},
    (64, 3): {1: (1, 264, 63, 255, 72), 2: (3, 264, 93, 93, 264)},
    (128, 1): {1: (2, 8, 63, 255, 136), 2: (3, 8, 93, 253, 392)},
}
# filter sizes whose NCHW row gets Wo % 4 == 0 (8-byte stores of 4 pixels; else the scalar store on the forced 8 x 16 tile):
# both stores under every KS, every BN and under RPS 3
_NCHW_VECTOR = {(32, 1): (3,), (32, 3): (), (64, 1): (1, 7), (64, 3): (3,), (128, 1): (1,)}
_FWD_SHAPES_K7 = {(64, 1): {1: (1, 8, 63, 255, 72), 2: (2, 8, 125, 509, 72)}}


def _fwd_cases():
    rows = []
    for s in (1, 2):
        for k in (1, 3, 7):
            for nchw in (False, True):
                for (BN, rps) in _FWD_SHAPES:
                    if (BN == 128 and k == 7) or (rps == 3 and k != 3):
                        continue
                    N, Cin, H, W, Cout = (_FWD_SHAPES_K7 if k == 7 else {}).get((BN, rps), _FWD_SHAPES[(BN, rps)])[s]
                    if nchw and k in _NCHW_VECTOR[(BN, rps)]:
                        W += s                       # Wo % 4 == 0: the vector NCHW store (the other NCHW rows: the scalar one)
                    name = f"bn{BN}{'_rps3' if rps == 3 else ''}_s{s}k{k}{'nchw' if nchw else 'nhwc'}"
                    rows.append(_c(name, (N, Cin, H, W, Cout), k, s, nchw=nchw, wdtype=("bf16", "f32")[len(rows) % 2],
                                   arm=tile(BN, s, k, nchw, rps)))
    # the persistent kernel: 3 x 3, stride 1, <= 32 input channels, <= 64 output channels, >= 2048 tiles of 8 x 16
    rows.append(_c("resident1", (1, 24, 509, 510, 8), 3, reflect=True, arm=resident(1)))
    rows.append(_c("resident2", (2, 32, 253, 510, 24), 3, arm=resident(2)))
    rows.append(_c("resident4", (1, 32, 510, 509, 40), 3, reflect=True, arm=resident(4)))
    return tuple(rows)


FWD_CASES = _fwd_cases()

# (case, what pick_tile does, (TR, TC)).  arm = the outcome's tag.
TILE_CASES = (
    (_c("t8x16_s1", (1, 8, 16, 80, 8), 3), "default", (8, 16)),
    (_c("t8x16_s2", (1, 8, 31, 159, 8), 3, 2), "default", (8, 16)),
    (_c("t4x32_s1", (1, 8, 4, 96, 8), 3), "4x32", (4, 32)),
    (_c("t4x32_s2", (1, 8, 7, 191, 8), 3, 2), "4x32", (4, 32)),
    (_c("t2x64_s1", (1, 8, 2, 128, 8), 3), "2x64", (2, 64)),
    (_c("t2x64_s2", (1, 8, 3, 255, 8), 1, 2), "2x64", (2, 64)),
    (_c("tfull_s1", (1, 8, 9, 20, 8), 3), "full_width", (6, 20)),
    (_c("tfull_s2", (2, 8, 17, 47, 8), 3, 2), "full_width", (5, 24)),
    (_c("tfull_clamp_s1", (1, 8, 5, 20, 8), 3), "full_width_clamped", (5, 20)),
    (_c("tfull_clamp_s2", (1, 8, 9, 39, 8), 3, 2), "full_width_clamped", (5, 20)),
    (_c("thalo_s1", (1, 8, 4, 32, 8), 7), "halo_rejected", (8, 16)),
    (_c("thalo_s2", (1, 8, 3, 127, 8), 3, 2), "halo_rejected", (2, 32)),
    (_c("tnchw_skip_s1", (1, 8, 9, 18, 8), 3, nchw=True), "nchw_skipped", (4, 32)),
    (_c("tnchw_skip_s2", (1, 8, 17, 35, 8), 3, 2, nchw=True), "nchw_skipped", (4, 32)),
)

# dil = 2 (the backward of a stride-2 layer; odd H and W) and the reflection fold.  arm = the arm of the DATA-GRADIENT launch.
DGRAD_CASES = (
    _c("dil2_k1_bn32", (2, 24, 9, 13, 40), 1, 2, arm=tile(32, 1, 1)),
    _c("dil2_k3_bn32", (2, 24, 9, 13, 40), 3, 2, arm=tile(32, 1, 3)),
    _c("dil2_k7_bn32", (2, 24, 9, 13, 40), 7, 2, arm=tile(32, 1, 7)),
    _c("dil2_k1_bn64", (1, 72, 127, 129, 16), 1, 2, arm=tile(64, 1, 1)),
    _c("dil2_k3_bn64", (1, 72, 127, 129, 16), 3, 2, arm=tile(64, 1, 3)),
    _c("dil2_k7_bn64", (1, 72, 127, 129, 16), 7, 2, arm=tile(64, 1, 7)),
    _c("dil2_k3_bn64_rps3", (1, 72, 127, 129, 264), 3, 2, arm=tile(64, 1, 3, rps=3)),
    _c("dil2_k3_bn32_rps3", (2, 24, 9, 13, 264), 3, 2, arm=tile(32, 1, 3, rps=3)),
    _c("reflect_3x3", (2, 8, 3, 3, 8), 3, reflect=True, bias="f32", arm=tile(32, 1, 3)),
    _c("reflect_ragged", (3, 40, 11, 21, 24), 3, reflect=True, bias="bf16", arm=tile(32, 1, 3)),
)

def _wgrad_cases():
    """(case, claims): case.arm = (stride, k, BM, BN) of conv_wgrad_kernel; claims = dict(rule: what set `splits`
    [, slabs, tree: the reducer, ppw: at least so many patches per workgroup (the prefetch under the MFMAs runs ppw - 1 times)])."""
    rows = []
    # the 24 instantiations on a ragged map (BM = 64: Cout > 32, BN = 64: Cin > 32); 7 x 7: one filter row per workgroup
    for s in (1, 2):
        for k in (1, 3, 7):
            for Cout in (24, 40):
                for Cin in (24, 40):
                    H, W = (11, 21) if s == 1 else (21, 41)
                    i = len(rows)
                    rows.append((_c(f"wg_s{s}k{k}_co{Cout}_ci{Cin}", (2, Cin, H, W, Cout), k, s, reflect=(k == 3 and s == 1 and Cin == 40),
                                    wdtype=("f32", "bf16")[i % 2], arm=(s, k, 64 if Cout > 32 else 32, 64 if Cin > 32 else 32)),
                                 dict(rule="patches", rgroups=7 if k == 7 else 1)))
    # the reducers' boundary: 16 patches -> 16 slabs (flat), 17 patches -> 17 slabs (tree)
    rows.append((_c("wg_slabs16", (1, 40, 8, 256, 40), 3, arm=(1, 3, 64, 64)), dict(rule="patches", slabs=16, tree=0)))
    rows.append((_c("wg_slabs17", (1, 40, 8, 260, 40), 3, wdtype="f32", arm=(1, 3, 64, 64)), dict(rule="patches", slabs=17, tree=1)))
    # two waves of workgroups with room in the workspace: 32 tiles x 16 splits, 3 patches each; 16 slabs
    rows.append((_c("wg_want", (3, 512, 32, 64, 256), 1, wdtype="f32", arm=(1, 1, 64, 64)), dict(rule="want", slabs=16, tree=0, ppw=3)))
    # the workspace cap: 7 x 7, 56 tiles x 5 splits over 18 patches
    rows.append((_c("wg_cap_7x7", (1, 512, 144, 7, 8), 7, arm=(1, 7, 32, 64)), dict(rule="cap", rgroups=7, ppw=3)))
    # the floor of 4 under a cap of 3: 64 tiles x 4 splits over 12 patches, at both strides
    rows.append((_c("wg_floor", (3, 512, 24, 20, 512), 3, reflect=True, arm=(1, 3, 64, 64)), dict(rule="floor", slabs=4, tree=0, ppw=3)))
    rows.append((_c("wg_floor_s2", (3, 512, 47, 39, 512), 3, 2, wdtype="f32", arm=(2, 3, 64, 64)),
                 dict(rule="floor", slabs=4, tree=0, ppw=3)))
    # one workgroup per CU beyond the cap: 1 tile x 256 splits over 768 patches
    rows.append((_c("wg_fill", (3, 40, 128, 256, 40), 3, arm=(1, 3, 64, 64)), dict(rule="fill", slabs=256, tree=1, ppw=3)))
    return tuple(rows)


WGRAD_CASES = _wgrad_cases()

# the scalar store paths, launched into a guarded buffer: channels-last with Cout % 4 != 0, NCHW with Wo % 4 != 0
SENTINEL_CASES = (
    _c("sentinel_nhwc_cout14", (2, 24, 5, 7, 14), 3),
    _c("sentinel_nchw_wo7", (2, 24, 5, 7, 16), 3, nchw=True),
)

TRANSPOSE_CASES = (
    _c("tr_8_nobias", (1, 8, 3, 5, 8), 3, 2, 1, wdtype="f32"),
    _c("tr_8_bias", (1, 8, 3, 5, 8), 3, 2, 1, bias="f32", wdtype="f32"),
    _c("tr_40_nobias", (2, 40, 7, 9, 40), 3, 2, 1, wdtype="bf16"),
    _c("tr_40_bias", (2, 40, 7, 9, 40), 3, 2, 1, bias="bf16", wdtype="bf16"),
)

# act x bias x layout x Cout in {1, 12, 24} (the zero-pad wrapper and the non-vector store) on two small shapes
_E1, _E2 = (2, 24, 6, 9), (1, 40, 11, 18)


def _epilogue_cases():
    rows, i = [], 0
    for act in ACTS:
        for bias in (None, "f32", "bf16"):
            for nchw in (False, True):
                N, Cin, H, W = (_E1, _E2)[i % 2]
                Cout = (1, 12, 24)[i % 3]
                k, s, reflect = ((3, 1, True), (3, 1, False), (1, 1, False), (3, 2, False))[(i // 2) % 4]
                rows.append(_c(f"{act}_{bias or 'nobias'}_{'nchw' if nchw else 'nhwc'}_co{Cout}", (N, Cin, H, W, Cout), k, s,
                               reflect=reflect, act=act, bias=bias, nchw=nchw, wdtype=("f32", "bf16")[i % 2]))
                i += 1
    return tuple(rows)


EPILOGUE_CASES = _epilogue_cases()


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _seed(c):
    s = 29
    for v in (c.N, c.Cin, c.H, c.W, c.Cout, c.k, c.stride, c.pad, int(c.reflect), ACTS.index(c.act), int(c.nchw),
              sum(ord(ch) for ch in c.name)):
        s = (s * 1000003 + v) % (2 ** 31 - 1)
    return s


def contraction(c, what):
    Ho, Wo = out_hw(c)
    return {"y": c.Cin * c.k * c.k, "dx": c.Cout * c.k * c.k, "dw": c.N * Ho * Wo, "db": c.N * Ho * Wo}[what]


def elements(c, transposed=False):
    """Elements of the largest tensor of the row (x, y, w)."""
    Ho, Wo = transpose_out_hw(c) if transposed else out_hw(c)
    return max(c.N * c.Cin * c.H * c.W, c.N * c.Cout * Ho * Wo, c.Cin * c.Cout * c.k * c.k)


def _conv64(x, w, b, c):
    xp = F.pad(x, (c.pad,) * 4, mode="reflect") if c.reflect else x
    return F.conv2d(xp, w, b, c.stride, 0 if c.reflect else c.pad), xp


def _act64(z, act):
    return {"none": z, "relu": torch.relu(z), "elu": F.elu(z), "sigmoid": torch.sigmoid(z)}[act]


KINK_FACTOR = 4.0        # x the accumulation bound n * 2^-23 * A: no kernel's sum can land on the other side of zero


def kink_margin(c, A):
    return KINK_FACTOR * contraction(c, "y") * U_ACC * A


def kink_count(c, inp):
    """Pre-activations of the float64 reference within the margin of zero (a kernel's ReLU could cut them the other way)."""
    z, A = _z_and_mag(c, inp)
    return int((z.abs() < kink_margin(c, A)).sum())


def _z_and_mag(c, inp):
    x, w = inp["x"].double(), inp["w"].double()
    b = None if inp["b"] is None else inp["b"].double()
    z, _ = _conv64(x, w, b, c)
    A, _ = _conv64(x.abs(), w.abs(), None if b is None else b.abs(), c)
    return z, A


def settle_kinks(c, inp, rounds=32):
    """Moves the centre tap of w[co, 0] by whole bf16 ulps for every output channel that has a pre-activation within the
    margin of zero, recomputes and repeats until there is none.  In place; -> rounds taken."""
    for it in range(rounds):
        z, A = _z_and_mag(c, inp)
        bad = (z.abs() < kink_margin(c, A)).flatten(2).any(2).any(0)
        if not bool(bad.any()):
            return it
        w = inp["w"]
        tap = w[:, 0, c.k // 2, c.k // 2].double()
        # the bf16 ulp of the largest weight: a whole number of ulps of every smaller one (a tap near zero has ulps too
        # small to move anything)
        ulp = torch.exp2(torch.floor(torch.log2(w.double().abs().max())) - 7)
        w[:, 0, c.k // 2, c.k // 2] = torch.where(bad, tap + (it + 1) * ulp, tap).to(w.dtype)
        assert torch.equal(w.float(), w.float().bfloat16().float())
    raise RuntimeError("kinks did not settle")


def make_inputs(c, transposed=False):
    """-> dict(x bf16 [N,Cin,H,W], w [Cout,Cin,k,k] ([Cin,Cout,3,3] transposed) of the parameter's dtype with values on the
    bf16 grid, b None | [Cout] fp32 / bf16 on the bf16 grid, go bf16 [N,Cout,Ho,Wo]).  ReLU rows are settled."""
    g = _gen(_seed(c))
    Ho, Wo = transpose_out_hw(c) if transposed else out_hw(c)
    x = torch.randn(c.N, c.Cin, c.H, c.W, generator=g).bfloat16()
    wshape = (c.Cin, c.Cout, c.k, c.k) if transposed else (c.Cout, c.Cin, c.k, c.k)
    w = (torch.randn(wshape, generator=g) / (c.Cin * c.k * c.k) ** 0.5).bfloat16()
    if c.wdtype == "f32":
        w = w.float()
    b = None
    if c.bias is not None:
        b = (0.2 * torch.randn(c.Cout, generator=g)).bfloat16()
        if c.bias == "f32":
            b = b.float()
    go = torch.randn(c.N, c.Cout, Ho, Wo, generator=g).bfloat16()
    inp = dict(x=x, w=w, b=b, go=go)
    if c.act == "relu" and not transposed:
        settle_kinks(c, inp)
    return inp


# ---------------------------------------------------------------------------------------------
# float64 reference with magnitude maps
# ---------------------------------------------------------------------------------------------
def act_grad64(y, act):
    """act'(z) written in the saved output y, as the backward forms it (ops._ConvNhwc.backward)."""
    if act == "relu":
        return (y > 0).double()
    if act == "elu":
        return torch.where(y > 0, torch.ones_like(y), y + 1)
    if act == "sigmoid":
        return y * (1 - y)
    return torch.ones_like(y)


def elu_fused(c):
    """The backward of this row forms dz and the bias sums in ppea_nhwc_bias_elu_bwd_bf16 (ops._ConvNhwc.backward: ELU,
    channels-last output, a channel count the kernel's thread layout divides); the GPU test checks this against the
    recorded launches."""
    ct = cout8(c) // 8
    return c.act == "elu" and not c.nchw and ct <= 256 and 256 % ct == 0


def stored_dz(c, go, y, fused):
    """dz = go * act'(y) bit for bit as the backward stores it from the device's own bf16 y, so that the data and weight
    gradient are referenced on the very operand their kernels read (no allowance for its roundings is needed then).
    Elementwise bf16 arithmetic rounds each operation once to nearest, on the host as on the device:
      ReLU     go * (y > 0)                          exact
      ELU      go * where(y > 0, 1, y + 1)           y + 1 rounds, the product rounds
      sigmoid  go * (y * (1 - y))                    three roundings
      ELU, fused kernel (`fused`)  fp32 go * (y > 0 ? 1 : y + 1), rounded once to bf16; its bias sums add the fp32 products
    -> (dz as stored, the values whose per-channel sum is the bias gradient), both float64."""
    gb, yb = go.bfloat16(), y.bfloat16()
    if c.act == "relu":
        dz = gb * (yb > 0)
    elif c.act == "elu" and fused:
        prod = gb.float() * torch.where(yb.float() > 0, torch.ones_like(yb.float()), yb.float() + 1.0)
        return prod.bfloat16().double(), prod.double()
    elif c.act == "elu":
        dz = gb * torch.where(yb > 0, torch.ones_like(yb), yb + 1)
    elif c.act == "sigmoid":
        dz = gb * (yb * (1 - yb))
    else:
        dz = gb
    return dz.double(), dz.double()


def _grads(x, w, go, c):
    """Gradients of sum(conv(x, w) * go) by autograd in double -> (dx, dw, dpad: the gradient on the reflection-padded
    domain or None)."""
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    z, xp = _conv64(x, w, None, c)
    if c.reflect:
        xp.retain_grad()
    (z * go).sum().backward()
    return x.grad, w.grad, (xp.grad if c.reflect else None)


def fold64(dpad, c):
    """The adjoint of the reflection pad: the padded-domain gradient folded back onto [H, W]."""
    t = torch.zeros(dpad.shape[0], dpad.shape[1], c.H, c.W, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(F.pad(t, (c.pad,) * 4, mode="reflect"), t, grad_outputs=dpad)[0]


def reference(c, inp, y_saved=None, fused=None):
    """float64 forward and gradients of one conv2d_nhwc row on the operands AS GIVEN (the bf16-rounded x, w, b, go).
    `y_saved`: the device's own stored output -- the backward forms dz = go * act'(y) from it in bf16, so the reference
    does too (`stored_dz`; `fused`: by the fused ELU kernel, default elu_fused(c)).  Without `y_saved` the gradients are
    those of the float64 forward.  -> dict of name -> (ref, bound) for y, dx, dw, db (db only with a bias), every bound a
    tensor of the reference's shape, plus z and the raw magnitude maps."""
    x, w, go = inp["x"].double(), inp["w"].double(), inp["go"].double()
    b = None if inp["b"] is None else inp["b"].double()
    z, A = _z_and_mag(c, inp)
    y = _act64(z, c.act)
    out = dict(z=z, A_y=A)
    if c.act == "none":
        out["y"] = (y, U_BF16 * y.abs() + (1 + U_BF16) * contraction(c, "y") * U_ACC * A)
    else:
        out["y"] = (y, ACT_REL * y.abs() + ACT_ABS * float(y.abs().max()))
    if y_saved is None:
        dz = dz_b = go * act_grad64(y, c.act)
    else:
        dz, dz_b = stored_dz(c, inp["go"], y_saved, elu_fused(c) if fused is None else fused)
    dx, dw, dpad = _grads(x, w, dz, c)
    A_dx, A_dw, A_dpad = _grads(x.abs(), w.abs(), dz.abs(), c)
    acc_x = (1 + U_BF16) * contraction(c, "dx") * U_ACC
    if c.reflect:
        # dpad is rounded to bf16 before the fold and the fold rounds again
        out["dx"] = (dx, U_BF16 * (dx.abs() + fold64(dpad.abs(), c)) + acc_x * A_dx)
        out["dpad"] = dpad
    else:
        out["dx"] = (dx, U_BF16 * dx.abs() + acc_x * A_dx)
    n_w = contraction(c, "dw")
    acc_w = (1 + U_BF16) * n_w * U_ACC * A_dw
    out["dw"] = (dw, acc_w + (U_BF16 * dw.abs() if c.wdtype == "bf16" else 0.0))
    if b is not None:
        db, A_db = dz_b.sum((0, 2, 3)), dz_b.abs().sum((0, 2, 3))
        out["db"] = (db, (1 + U_BF16) * n_w * U_ACC * A_db + (U_BF16 * db.abs() if c.bias == "bf16" else 0.0))
    return out


def reference_transposed(c, inp):
    """float64 F.conv_transpose2d(x, w, b, 2, 1, output_padding=1) with its gradients and bounds, as `reference`."""
    x = inp["x"].double().requires_grad_(True)
    w = inp["w"].double().requires_grad_(True)
    b = None if inp["b"] is None else inp["b"].double().requires_grad_(True)
    go = inp["go"].double()
    y = F.conv_transpose2d(x, w, b, 2, 1, output_padding=1)
    (y * go).sum().backward()
    xa = inp["x"].double().abs().requires_grad_(True)
    wa = inp["w"].double().abs().requires_grad_(True)
    A = F.conv_transpose2d(xa, wa, None if b is None else b.detach().abs(), 2, 1, output_padding=1)
    (A * go.abs()).sum().backward()
    n_y, n_x, n_w = c.Cin * 9, c.Cout * 9, c.N * c.H * c.W
    out = dict(y=(y.detach(), U_BF16 * y.detach().abs() + (1 + U_BF16) * n_y * U_ACC * A.detach()),
               dx=(x.grad, U_BF16 * x.grad.abs() + (1 + U_BF16) * n_x * U_ACC * xa.grad),
               dw=(w.grad, (1 + U_BF16) * n_w * U_ACC * wa.grad + (U_BF16 * w.grad.abs() if c.wdtype == "bf16" else 0.0)))
    if b is not None:
        Ho, Wo = transpose_out_hw(c)
        n_b = c.N * Ho * Wo
        out["db"] = (b.grad, (1 + U_BF16) * n_b * U_ACC * go.abs().sum((0, 2, 3))
                     + (U_BF16 * b.grad.abs() if c.bias == "bf16" else 0.0))
    return out


def worst(got, ref, bound):
    """-> (max over elements of err / bound, elements outside their bound).  A zero bound admits only an exact match; a
    NaN or an infinite element is outside its bound (counted as NOT err <= bound; its ratio reads inf)."""
    err = (got.double() - ref).abs()
    inside = err <= bound
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max()) if ratio.numel() else 0.0, int((~inside).sum())


def all_cases():
    """Every conv2d_nhwc row of every table (the transposed rows are apart: their shapes read differently)."""
    return (FWD_CASES + tuple(t[0] for t in TILE_CASES) + DGRAD_CASES + tuple(w[0] for w in WGRAD_CASES) + EPILOGUE_CASES)


