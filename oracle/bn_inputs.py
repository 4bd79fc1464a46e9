"""TEST INFRASTRUCTURE ONLY -- case tables, seeded inputs and a float64 reference for the training-mode BatchNorm
kernels (csrc/bn_fused.hip):  y = act(BN1(z1) [+ BN2(z2)]) * mask[n] + r1 + s * r2  and the end-of-block + next-block form
y2 = BN_B(y).  Pure torch on the CPU; everything is a function of its arguments and the seed.
tests/test_bn_arms_cpu.py proves the properties the GPU test (tests/test_bn_arms_gpu.py) relies on."""
import math

import torch

EPS, MOMENTUM = 1e-5, 0.1
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2

# ---------------------------------------------------------------------------------------------
# host-side dispatch, restated (csrc/bn_common.h, csrc/bn_fused.hip, ops.bn_channel_ok)
# ---------------------------------------------------------------------------------------------
TPB, VEC = 256, 8                     # threads per workgroup, elements per 16-byte step
CHANNEL_ELEMS = 16384                 # N * HW a channel-owning workgroup holds in registers
SMALL_PLANE = 4096                    # HW up to which one wave takes a plane's statistics
NV_INSTANCES = (1, 2, 3, 4, 8)


def bn_nv(N, HW):
    """16-byte vectors per thread of a channel-owning workgroup (bn_common.h bn_nv)."""
    return (N * (HW // VEC) + TPB - 1) // TPB


def nv_instance(N, HW):
    """The register-tile instantiation PPEA_BN_NV launches for bn_nv(N, HW): 5..7 run on the 8."""
    nv = bn_nv(N, HW)
    return 1 if nv <= 1 else (nv if nv <= 4 else 8)


def channel_ok(N, C, HW):
    """ops.bn_channel_ok / the guards of the ppea_bn_*_channel_* entry points."""
    return C >= 64 and HW % VEC == 0 and N * HW <= CHANNEL_ELEMS


def plane_chunks(planes, HW):
    """Pieces bn_apply / bn_bwd_apply cut a plane into (bn_fused.hip plane_chunks); only HW % 8 != 0 gets there."""
    chunks = 1
    while planes * chunks < 2048 and HW // (chunks * 2) >= 1024:
        chunks *= 2
    return chunks


def wave_kernel(HW):
    """bn_stats_wave / bn_bwd_reduce_wave (one wave per plane) rather than bn_stats / bn_bwd_reduce (one workgroup)."""
    return HW % VEC == 0 and HW <= SMALL_PLANE


def apply_kernel(N, C, HW):
    """'flat' (bn_apply_flat, HW % 8 == 0) or the number of chunks of the per-plane bn_apply."""
    return "flat" if HW % VEC == 0 else plane_chunks(N * C, HW)


# (shape, instantiation, bn_nv)
CHANNEL_CASES = (
    ((1, 64, 1, 8), 1, 1),            # one vector: 255 idle threads
    ((12, 64, 2, 4), 1, 1),           # hv = 1: every vector its own plane and its own DropPath mask entry
    ((2, 64, 32, 32), 1, 1),          # 256 vectors: exactly full
    ((1, 64, 8, 257), 2, 2),          # 257: one thread holds two
    ((4, 64, 32, 32), 2, 2),          # 512: full
    ((3, 64, 8, 171), 3, 3),          # 513
    ((1, 64, 8, 769), 4, 4),          # 769
    ((8, 64, 32, 32), 4, 4),          # 1024: full
    ((5, 64, 8, 205), 8, 5),          # 1025: bn_nv = 5 runs on the 8 instantiation with idle register slots
    ((11, 64, 8, 163), 8, 8),         # 1793
    ((1, 64, 128, 128), 8, 8),        # 2048 vectors: exactly the 16384-element cap
    ((3, 65, 4, 8), 1, 1),            # odd channel count
)
# refused by channel_ok; the general path must serve them
REFUSED_CASES = (
    (1, 64, 8, 2049),                 # 16392 elements
    (2, 63, 4, 8),                    # C < 64
)
# (shape, statistics kernel, apply_kernel)
GENERAL_CASES = (
    ((1, 5, 2, 4), "wave", "flat"),           # 5 planes: the last block has one live wave
    ((1, 3, 64, 64), "wave", "flat"),         # HW = 4096: the last plane size the wave kernels take
    ((1, 3, 8, 513), "block", "flat"),        # HW = 4104: just over the switch
    ((2, 5, 1, 1), "block", 1),               # count 2, HW = 1
    ((2, 3, 1, 7), "block", 1),               # scalar tails around the block size
    ((1, 4, 3, 3), "block", 1),
    ((1, 2, 1, 257), "block", 1),
    ((1, 3, 33, 63), "block", 2),             # HW = 2079: 2 chunks
    ((1, 3, 5, 821), "block", 4),             # HW = 4105: 4 uneven chunks
)
# one channel case per instantiation for the skip / dup / next forms
PER_NV = {1: (2, 64, 32, 32), 2: (1, 64, 8, 257), 3: (3, 64, 8, 171), 4: (1, 64, 8, 769), 8: (5, 64, 8, 205)}
# count 2: xhat = +-1 up to eps, so dz = a * (g0 - g1) / 2 * eps / (var + eps) -- with var of order 1 a 1e-5 residue of a
# cancellation that no fp32 evaluation resolves to 2e-4.  The case draws z with var of order eps, where dz is of order a * g.
INPUT_SCALE = {(2, 5, 1, 1): (0.0, 3e-3)}

# (two BNs, activation, mask + r1 + r2): every value of every factor, and the heaviest combination
COMBOS = ((False, 0, False), (False, 1, False), (True, 1, False), (False, 2, False), (False, 0, True), (True, 1, True),
          (True, 2, True))


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def storage(dtype):
    return {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]


def _seed(shape, *extra):
    s = 17
    for v in tuple(shape) + tuple(int(e) for e in extra):
        s = (s * 1000003 + v) % (2 ** 31 - 1)
    return s


def grid_grad(shape, g, scale=1.0):
    """A gradient on the 2^-4 grid with |value| < 4 (times `scale`, a power of two): exact in bf16, and so is the sum of
    two of them -- the kernels' round(dy + dyb) merge is then the identity and the fp64 sum is the reference as it stands."""
    return (torch.randn(shape, generator=g) * 16).round().clamp(-63, 63) / 16 * scale


def sample_mask(N):
    """DropPath scale per sample: zeros in it, every live entry different (a vector reading its neighbour's entry shows).
    N = 1 keeps its one sample: a zero there would blank the whole case."""
    if N == 1:
        return torch.tensor([1.4])
    return torch.tensor([0.0 if n % 3 == 0 else 1.0 + 0.125 * (n % 5) for n in range(N)])


# ---------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------
def _d(t, grad=False):
    return None if t is None else t.detach().double().clone().requires_grad_(grad)


def _bn64(z, gamma, beta, rm0, rv0):
    n = z.numel() // z.shape[1]
    mean = z.mean((0, 2, 3))
    var = ((z - mean[None, :, None, None]) ** 2).mean((0, 2, 3))
    invstd = (var + EPS).rsqrt()
    a = gamma * invstd
    o = beta - mean * a
    out = (z - mean[None, :, None, None]) * a[None, :, None, None] + beta[None, :, None, None]
    unbiased = var * n / max(n - 1, 1)
    st = dict(mean=mean.detach(), var=var.detach(), invstd=invstd.detach(),
              running_mean=((1 - MOMENTUM) * rm0 + MOMENTUM * mean).detach(),
              running_var=((1 - MOMENTUM) * rv0 + MOMENTUM * unbiased).detach())
    # |a x| + |o|: the magnitude whose fp32 rounding the kernels' a * x + o form carries
    mag = ((a[None, :, None, None] * z).abs() + o.abs()[None, :, None, None]).detach()
    return out, st, mag


def _act64(u, act):
    if act == ACT_RELU:
        return torch.relu(u)
    if act == ACT_GELU:
        return 0.5 * u * (1 + torch.erf(u / math.sqrt(2.0)))
    return u


def reference(z1, g1, b1, z2=None, g2=None, b2=None, act=ACT_NONE, mask=None, r1=None, r2=None, r2_scale=1.0, go=None,
              go_b=None, g_skip=None, rm0=0.0, rv0=1.0):
    """float64 y = act(BN1(z1) [+ BN2(z2)]) * mask[n] + r1 + r2_scale * r2 of the values AS GIVEN (pass the stored, e.g.
    bf16-rounded, tensors), batch statistics, running statistics from (rm0, rv0) and -- with `go`, the gradient arriving
    at y -- every gradient by autograd.  `go_b`: a second gradient arriving at y (the `dup` form); `g_skip`: a gradient
    arriving at z1 through its other use (the `skip` form).  -> dict."""
    grad = go is not None
    a, w1, c1 = _d(z1, grad), _d(g1, grad), _d(b1, grad)
    bb, w2, c2 = _d(z2, grad), _d(g2, grad), _d(b2, grad)
    q1, q2 = _d(r1, grad), _d(r2, grad)
    u, st1, mag = _bn64(a, w1, c1, rm0, rv0)
    out = {k + "1": v for k, v in st1.items()}
    if bb is not None:
        u2, st2, mag2 = _bn64(bb, w2, c2, rm0, rv0)
        u, mag = u + u2, mag + mag2
        out.update({k + "2": v for k, v in st2.items()})
    y = _act64(u, act)
    if mask is not None:
        y = y * mask.double().view(-1, 1, 1, 1)
    if q1 is not None:
        y = y + q1
    if q2 is not None:
        y = y + r2_scale * q2
    out.update(y=y.detach(), u=u.detach(), mag=mag)
    if grad:
        loss = (y * go.double()).sum()
        if go_b is not None:
            loss = loss + (y * go_b.double()).sum()
        if g_skip is not None:
            loss = loss + (a * g_skip.double()).sum()
        loss.backward()
        for name, leaf in (("dz1", a), ("dg1", w1), ("db1", c1), ("dz2", bb), ("dg2", w2), ("db2", c2), ("dr1", q1),
                           ("dr2", q2)):
            if leaf is not None:
                out[name] = leaf.grad
    return out


def reference_next(z, gA, bA, gB, bB, y_in, mask=None, r1=None, r2=None, r2_scale=1.0, go2=None, go2_b=None, go_y=None,
                   dy_in=None):
    """The end-of-block + next-block form.  Stage A: y = mask * BN_A(z) + r1 + r2_scale * r2 as `reference`.  Stage B:
    y2 = BN_B(y_in) on the y the caller passes in (the stored y: the kernel takes BN_B's statistics of the rounded values).
    Gradients: `go2` (+ `go2_b`) arrive at y2 and `go_y` at y through its other use; dy = BN_B-backward + go_y is the total
    gradient of y, and stage A's backward runs on `dy_in` where given (the stored dy, as stage B's forward runs on the stored
    y), else on that dy.  -> (A, B) dicts; B["dy"] is the total gradient of y."""
    B = reference(y_in, gB, bB, go=go2, go_b=go2_b, g_skip=go_y)
    dy = None
    if go2 is not None:
        dy = B["dy"] = B.pop("dz1")
    A = reference(z, gA, bA, mask=mask, r1=r1, r2=r2, r2_scale=r2_scale, go=dy if dy_in is None else dy_in)
    return A, B


# ---------------------------------------------------------------------------------------------
# ReLU kink
# ---------------------------------------------------------------------------------------------
KINK_FACTOR = 64 * 2.0 ** -24         # 64 x the rounding of the kernels' a * x + o form


def _ulp(z, dt):
    bits = 23 if dt == torch.float32 else 7
    e = torch.floor(torch.log2(z.double().abs().clamp_min(1e-30)))
    return torch.exp2(e - bits)


def kink_count(ref):
    """Elements whose pre-activation lies within the margin of 0 (their ReLU gradient could flip)."""
    return int((ref["u"].abs() < KINK_FACTOR * ref["mag"]).sum())


def settle_kinks(inp, rounds=32):
    """Moves every element of z1 whose float64 pre-activation lies within KINK_FACTOR * (|a x| + |o|) of zero away from
    it, in whole ulps of the storage type, recomputes (the statistics move with z1) and repeats until there is none.
    In place; -> rounds taken."""
    dt = inp["z1"].dtype
    for it in range(rounds):
        ref = reference(inp["z1"], inp["g1"], inp["b1"], inp.get("z2"), inp.get("g2"), inp.get("b2"), act=ACT_RELU)
        u, margin = ref["u"], KINK_FACTOR * ref["mag"]
        bad = u.abs() < margin
        if not bool(bad.any()):
            return it
        a1 = (inp["g1"].double() * ref["invstd1"])[None, :, None, None].expand_as(u)
        if bool((a1[bad] == 0).any()):
            raise ValueError("an element at the kink of a channel with gamma = 0 cannot be moved")
        z = inp["z1"].double()
        ulp = _ulp(z, dt)
        side = torch.where(u >= 0, 1.0, -1.0) * torch.sign(a1)
        steps = torch.ceil((2 * margin - u.abs()) / (a1.abs() * ulp)).clamp_min(1.0)
        inp["z1"] = torch.where(bad, z + side * steps * ulp, z).to(dt)
    raise RuntimeError("kinks did not settle")


# ---------------------------------------------------------------------------------------------
# benign inputs (mean 0.5, std 2 -- the data of the existing kernel tests)
# ---------------------------------------------------------------------------------------------
def make_inputs(shape, dtype, two=False, act=ACT_NONE, res=False, extra=False):
    """Stored-type inputs of one case: z1 [z2], gamma / beta per BN, [mask, r1, r2], the gradient `go` arriving at y and, with
    `extra`, a second gradient of y (`go_b`) and a gradient of z1 from its other use (`g_skip`, 4 x the scale: the residual
    gradient is the larger one in the network, and a bf16 kernel rounds dz before it adds).  ReLU cases are settled."""
    N, C = shape[0], shape[1]
    dt = storage(dtype)
    g = _gen(_seed(shape, two, act, res))
    mean, std = INPUT_SCALE.get(tuple(shape), (0.5, 2.0))
    inp = dict(z1=(torch.randn(shape, generator=g) * std + mean).to(dt),
               g1=torch.rand(C, generator=g) + 0.5, b1=torch.randn(C, generator=g) * 0.2)
    z2 = (torch.randn(shape, generator=g) * 0.35 * std - 0.4 * mean).to(dt)
    g2, b2 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    if two:
        inp.update(z2=z2, g2=g2, b2=b2)
    r1, r2 = torch.randn(shape, generator=g).to(dt), torch.randn(shape, generator=g).to(dt)
    if res:
        inp.update(mask=sample_mask(N), r1=r1, r2=r2)
    inp["go"] = grid_grad(shape, g).to(dt)
    if extra:
        inp["go_b"] = grid_grad(shape, g).to(dt)
        inp["g_skip"] = grid_grad(shape, g, 4.0).to(dt)
    if act == ACT_RELU:
        settle_kinks(inp)
    return inp


def reference_of(inp, act=ACT_NONE, r2_scale=0.5, dup=False, skip=False, **kw):
    return reference(inp["z1"], inp["g1"], inp["b1"], inp.get("z2"), inp.get("g2"), inp.get("b2"), act=act,
                     mask=inp.get("mask"), r1=inp.get("r1"), r2=inp.get("r2"), r2_scale=r2_scale, go=inp["go"],
                     go_b=inp["go_b"] if dup else None, g_skip=inp["g_skip"] if skip else None, **kw)


# ---------------------------------------------------------------------------------------------
# ill-conditioned channels
# ---------------------------------------------------------------------------------------------
# name -> |mean| / std the channel claims (None: not a ratio recipe)
VALUE_CASES = {
    "f32": (("ratio0", 0.0), ("ratio1", 1.0), ("ratio30", 30.0), ("ratio300", 300.0), ("constant", None),
            ("tiny_std", None), ("outlier", None), ("gamma0", None), ("neg_gamma", None)),
    # bf16: above 30 the grid spacing (2^-7 relative) exceeds the std
    "bf16": (("ratio0", 0.0), ("ratio1", 1.0), ("ratio30", 30.0), ("constant", None), ("tiny_std", None),
             ("outlier", None), ("gamma0", None), ("neg_gamma", None)),
}
CONSTANT_VALUE, TINY_STD, OUTLIER_VALUE = 3.0, 1e-4, 100.0


def value_recipes(C, dtype):
    """Recipe name per channel: the recipes laid across the C channels in turn, so one launch covers them all."""
    names = [n for n, _ in VALUE_CASES[dtype]]
    return [names[c % len(names)] for c in range(C)]


def value_inputs(shape, dtype):
    """-> dict(z1, g1, b1, go, recipes): per-channel recipes of VALUE_CASES[dtype]; signs of the mean alternate."""
    N, C, H, W = shape
    dt = storage(dtype)
    g = _gen(_seed(shape, 99))
    ratios = dict(VALUE_CASES[dtype])
    recipes = value_recipes(C, dtype)
    z = torch.randn(shape, generator=g)
    g1, b1 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    for c, name in enumerate(recipes):
        sign = -1.0 if (c // len(ratios)) % 2 else 1.0
        if ratios[name] is not None:
            z[:, c] += sign * ratios[name]
        elif name == "constant":
            z[:, c] = sign * CONSTANT_VALUE
        elif name == "tiny_std":
            z[:, c] *= TINY_STD
        elif name == "outlier":
            z[:, c] = 0.0
            z[N // 2, c, H // 2, W // 3] = sign * OUTLIER_VALUE
        elif name == "gamma0":
            g1[c] = 0.0
        elif name == "neg_gamma":
            g1[c] = -1.3
    return dict(z1=z.to(dt), g1=g1, b1=b1, go=grid_grad(shape, g).to(dt), recipes=recipes)
