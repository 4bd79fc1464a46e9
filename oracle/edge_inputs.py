"""TEST INFRASTRUCTURE ONLY -- seeded edge-case inputs for the warp, loss and cost-reduce kernels
(grid_sample, smooth_loss, loss_select, loss_tail, cost_volume_reduce).  Pure torch on the CPU; everything
is a function of its arguments and the seed.  tests/test_loss_warp_edges_cpu.py proves the properties the
GPU test (tests/test_loss_warp_edges_gpu.py) relies on."""
import torch

# ---------------------------------------------------------------------------------------------
# grid_sample
# ---------------------------------------------------------------------------------------------
GRID_BLOCKS = ("lattice", "rim", "far", "random")
# 1e-3 is taken on the 2^-22 grid (4194 * 2^-22 = 0.99993e-3): then (g + 1) is exact in fp32 for every rim coordinate, as
# it is in fp64, and with Wi-1 a power of two so is ix.  With the decimal 1e-3 the fp32 sum 1.001 + 1 rounds by up to 2^-23,
# which Wi-1 = 16 turns into 1e-6 of a pixel: as large as the agreement the CPU test demands of the two precisions.
RIM_OFFSETS = (0.0, 2.0 ** -20, 4194 * 2.0 ** -22)
FAR_VALUES = (3.0, 1e6, 1e30)          # 3e38 overflows ix: fp32 ATen itself returns NaN there (zeros mode)
NEAR_INT = 1e-4                        # |ix - round(ix)| below this: fp32 and fp64 may pick different cells


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def grid_blocks(Hi, Wi):
    """Names of the blocks grid_cases stacks, in order.  The lattice needs two pixels on both axes."""
    return GRID_BLOCKS if (Hi >= 2 and Wi >= 2) else GRID_BLOCKS[1:]


def _fill(points, Ho, Wo, g):
    """[N,2] points -> [Ho,Wo,2]: a seeded shuffle of the points, repeated until the output is full."""
    n = points.shape[0]
    order = torch.randperm(n, generator=g)
    idx = order[torch.arange(Ho * Wo) % n]
    return points[idx].reshape(Ho, Wo, 2)


def _cross(xs, ys):
    xs, ys = torch.as_tensor(xs, dtype=torch.float32), torch.as_tensor(ys, dtype=torch.float32)
    return torch.stack([xs[None, :].expand(len(ys), len(xs)), ys[:, None].expand(len(ys), len(xs))], -1).reshape(-1, 2)


def _is_pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def lattice_points(Hi, Wi):
    """Every pixel centre, rims included; the four corners first (they survive any cropping).  With Wi-1 and
    Hi-1 powers of two the coordinates, and ix / iy computed from them, are exact in fp32 and in fp64."""
    if not (_is_pow2(Wi - 1) and _is_pow2(Hi - 1)):
        raise ValueError("lattice block: Wi-1 and Hi-1 must be powers of two")
    xs = -1 + 2 * torch.arange(Wi, dtype=torch.float32) / (Wi - 1)
    ys = -1 + 2 * torch.arange(Hi, dtype=torch.float32) / (Hi - 1)
    return _cross(xs, ys)


def rim_points():
    v = [s + o for s in (-1.0, 1.0) for d in RIM_OFFSETS for o in ((d,) if d == 0 else (-d, d))]
    return _cross(v, v)


def far_points():
    v = [s * f for f in FAR_VALUES for s in (-1.0, 1.0)]
    return _cross(v, v)


def grid_cases(Hi, Wi, Ho, Wo, seed):
    """[B,Ho,Wo,2] fp32 sampling grid for an Hi x Wi source; B = len(grid_blocks(Hi, Wi)), one block per item."""
    g = _gen(seed)
    out = []
    for name in grid_blocks(Hi, Wi):
        if name == "lattice":
            pts = lattice_points(Hi, Wi)
            corners = torch.tensor([0, Wi - 1, (Hi - 1) * Wi, Hi * Wi - 1])
            rest = torch.tensor([i for i in range(Hi * Wi) if i not in set(corners.tolist())], dtype=torch.long)
            rest = rest[torch.randperm(rest.numel(), generator=g)]
            idx = torch.cat([corners, rest])[torch.arange(Ho * Wo) % (Hi * Wi)]
            out.append(pts[idx].reshape(Ho, Wo, 2))
        elif name == "rim":
            out.append(_fill(rim_points(), Ho, Wo, g))
        elif name == "far":
            out.append(_fill(far_points(), Ho, Wo, g))
        else:
            out.append((torch.rand(Ho, Wo, 2, generator=g) * 2 - 1) * 1.3)
    return torch.stack(out).float().contiguous()


def grid_source(B, C, Hi, Wi, seed):
    return torch.rand(B, C, Hi, Wi, generator=_gen(seed + 7919))


def near_integer(grid, Hi, Wi):
    """[B,Ho,Wo] bool: the un-normalised coordinate (fp64) lies within NEAR_INT of an integer on an axis that has
    more than one pixel.  (On a one-pixel axis ix == 0 exactly in every precision.)"""
    gd = grid.double()
    bad = torch.zeros(grid.shape[:-1], dtype=torch.bool)
    for k, n in ((0, Wi), (1, Hi)):
        if n > 1:
            c = (gd[..., k] + 1) / 2 * (n - 1)
            bad |= (c - c.round()).abs() < NEAR_INT
    return bad


# ---------------------------------------------------------------------------------------------
# smooth_loss
# ---------------------------------------------------------------------------------------------
def smooth_cases(B, C, H, W, seed):
    """-> (disp [B,1,H,W], img [B,C,H,W]).  The disparity is cut into 3x3 tiles (offset by one pixel, so even a
    2x2 map spans four tiles); a tile is a plateau (one value), coarse noise (four levels: equal neighbours by
    chance) or continuous noise."""
    g = _gen(seed)
    th, tw = (H + 2) // 3 + 1, (W + 2) // 3 + 1
    ty = (torch.arange(H) + 2) // 3
    tx = (torch.arange(W) + 2) // 3
    kind = torch.randint(0, 3, (B, 1, th, tw), generator=g)[:, :, ty][:, :, :, tx]
    level = (0.1 + 0.8 * torch.rand(B, 1, th, tw, generator=g))[:, :, ty][:, :, :, tx]
    noise = 0.1 + 0.8 * torch.rand(B, 1, H, W, generator=g)
    coarse = 0.25 * (1 + torch.randint(0, 4, (B, 1, H, W), generator=g).float())
    disp = torch.where(kind == 0, level, torch.where(kind == 1, coarse, noise))
    disp[0, 0, 0, 1] = disp[0, 0, 0, 0]                          # one equal pair even in a 2x2 map
    img = torch.rand(B, C, H, W, generator=g)
    return disp.contiguous(), img


def flat_pixels(disp):
    """[B,1,H,W] bool: every neighbour the pixel has (left, right, up, down) equals it."""
    eq = torch.ones_like(disp, dtype=torch.bool)
    ex = disp[..., :, 1:] == disp[..., :, :-1]
    ey = disp[..., 1:, :] == disp[..., :-1, :]
    eq[..., :, 1:] &= ex
    eq[..., :, :-1] &= ex
    eq[..., 1:, :] &= ey
    eq[..., :-1, :] &= ey
    return eq


# ---------------------------------------------------------------------------------------------
# loss_select
# ---------------------------------------------------------------------------------------------
def select_cases(B, C, H, W, seed, nan_layer=False):
    """dict: reproj, identity [B,2,H,W]; warped_m1, warped_p1 [B,C,H,W]; noise [B,1,H,W]; tie_reproj, tie_identity,
    tie_auto [B,1,H,W] bool (where ties were planted).  Warped frames: 12 % of pixels near-black in frame -1 only,
    12 % in frame +1 only, 16 % in both; a near-black pixel's channel sum is 0.1 * f with f in [0.2, 0.999] (four
    in five) or [1.001, 1.5], so the `sum_C < 0.1` test falls on both sides and never within rounding of 0.1."""
    g = _gen(seed)
    reproj = torch.rand(B, 2, H, W, generator=g)
    identity = torch.rand(B, 2, H, W, generator=g)
    u = torch.rand(3, B, 1, H, W, generator=g)
    tie_r, tie_i, tie_a = u[0] < 0.15, u[1] < 0.15, u[2] < 0.15
    reproj[:, 1:] = torch.where(tie_r, reproj[:, :1], reproj[:, 1:])
    identity[:, 1:] = torch.where(tie_i, identity[:, :1], identity[:, 1:])
    # identity minimum == reprojection minimum (a tie in the automask argmin when no frame is black and no noise is added)
    rmin = reproj.min(1, keepdim=True)[0]
    identity[:, :1] = torch.where(tie_a, rmin, identity[:, :1])
    identity[:, 1:] = torch.where(tie_a, rmin + 0.25 * torch.rand(B, 1, H, W, generator=g), identity[:, 1:])
    tie_i = tie_i & ~tie_a

    def frame(dark):
        col = 0.2 + 0.8 * torch.rand(B, C, H, W, generator=g)
        below = torch.rand(B, 1, H, W, generator=g) < 0.8
        f = torch.where(below, 0.2 + 0.799 * torch.rand(B, 1, H, W, generator=g),
                        1.001 + 0.499 * torch.rand(B, 1, H, W, generator=g))
        wgt = 0.5 + torch.rand(B, C, H, W, generator=g)
        black = 0.1 * f * wgt / wgt.sum(1, keepdim=True)
        return torch.where(dark, black, col)

    cls = torch.rand(B, 1, H, W, generator=g)
    wm1 = frame((cls < 0.12) | ((cls >= 0.24) & (cls < 0.40)))
    wp1 = frame((cls >= 0.12) & (cls < 0.40))
    noise = torch.randn(B, 1, H, W, generator=g) * 1e-5
    if nan_layer:
        nan = float("nan")
        n = B * H * W
        pos = torch.randperm(n, generator=g)[:min(n, 24)]

        def plant(t, which):        # which: a cycle of channel sets
            flat = t.permute(1, 0, 2, 3).reshape(2, n)
            for j, p in enumerate(pos.tolist()):
                for c in which[j % len(which)]:
                    flat[c, p] = nan
            return flat.reshape(2, B, H, W).permute(1, 0, 2, 3).contiguous()

        reproj = plant(reproj, [(0,), (1,), (0, 1), (), (), ()])
        identity = plant(identity, [(), (), (), (0,), (1,), (0, 1)])
    return dict(reproj=reproj.contiguous(), identity=identity.contiguous(), warped_m1=wm1, warped_p1=wp1, noise=noise,
                tie_reproj=tie_r, tie_identity=tie_i, tie_auto=tie_a)


def select_source_code(frame_idx, warped_m1, warped_p1, selec):
    """uint8 [B,1,H,W]: 2 where both warped frames are near-black, otherwise the frame whose loss was taken."""
    code = frame_idx.clone()
    if selec:
        m1 = warped_m1.sum(1, keepdim=True) < 0.1
        p1 = warped_p1.sum(1, keepdim=True) < 0.1
        code = torch.where(m1, torch.ones_like(code), code)
        code = torch.where(p1, torch.zeros_like(code), code)
        code = torch.where(m1 & p1, torch.full_like(code, 2), code)
    return code.to(torch.uint8)


# ---------------------------------------------------------------------------------------------
# loss_tail
# ---------------------------------------------------------------------------------------------
def tail_cases(B, H, W, seed, is_multi, all_masked=False):
    """The construction of test_loss_tail_equals_the_elementwise_composite at any shape: reproj [B,2,H,W], src code
    (0 / 1 / 2) and the selected loss, auto_idx, cons [B,H,W], aug [B,1,1,1] (every second item augmented), multi and
    mono depth (equal on a few pixels: |.| at 0).  all_masked: auto_idx all 1 (single-frame pass), aug all 1 (multi)."""
    g = _gen(seed + int(is_multi))
    reproj = torch.rand(B, 2, H, W, generator=g)
    src = torch.randint(0, 3, (B, 1, H, W), generator=g).to(torch.uint8)
    sel = torch.where(src == 0, reproj[:, :1], torch.where(src == 1, reproj[:, 1:], torch.zeros(B, 1, H, W)))
    auto_idx = torch.randint(0, 2, (B, 1, H, W), generator=g)
    cons = (torch.rand(B, H, W, generator=g) > 0.4).float()
    aug = (torch.arange(B) % 2 == 1).float().view(B, 1, 1, 1)
    multi = 1 + torch.rand(B, 1, H, W, generator=g)
    mono = 1 + torch.rand(B, 1, H, W, generator=g)
    multi[0, 0, 0, :5] = mono[0, 0, 0, :5]
    if all_masked:
        auto_idx = torch.ones_like(auto_idx)
        aug = torch.ones_like(aug)
    return dict(reproj=reproj, src=src, sel=sel, auto_idx=auto_idx, cons=cons, aug=aug, multi=multi, mono=mono)


def tail_reference(c, is_multi, use_cons=True, use_aug=True, w_rl=0.7, w_cl=1.3):
    """fp64 element-wise formulation under autograd -> dict(rl, cl, mask, target, d_reproj, d_multi)."""
    B, _, H, W = c["reproj"].shape
    r = c["reproj"].double().requires_grad_(True)
    m64 = c["multi"].double().requires_grad_(True)
    src = c["src"]
    selr = torch.where(src == 0, r[:, :1], torch.where(src == 1, r[:, 1:], torch.zeros(B, 1, H, W, dtype=torch.float64)))
    if is_multi:
        mask = torch.ones(B, 1, H, W, dtype=torch.float64)
        if use_cons:
            mask = mask * c["cons"].double().unsqueeze(1)
        if use_aug:
            mask = mask * (1 - c["aug"].double())
    else:
        mask = (c["auto_idx"] == 0).double()
    rl = (selr * mask).sum() / (mask.sum() + 1e-7)
    cm = 1 - mask
    cl = (torch.abs(m64 - c["mono"].double()) * cm).mean() if is_multi else None
    tgt = 1 / (c["mono"].double() * cm + m64.detach() * (1 - cm)) if is_multi else None
    (rl * w_rl + (cl * w_cl if is_multi else 0)).backward()
    return dict(rl=rl.detach(), cl=None if cl is None else cl.detach(), mask=mask, target=tgt, d_reproj=r.grad,
                d_multi=m64.grad if is_multi else None)


# ---------------------------------------------------------------------------------------------
# cost_volume_reduce
# ---------------------------------------------------------------------------------------------
def reduce_cases(B, D, h, w, seed=0):
    """Raw cost volume [B,D,h,w] >= 0 (0 = bin not observed) with four kinds of pixel, a quarter each: all bins
    positive; some bins exactly 0; all bins exactly 0; the minimum repeated in two or three bins (and, for every
    second such pixel, one other bin exactly 0)."""
    g = _gen(seed + 31 * D + h * w)
    raw = 0.05 + torch.rand(B, D, h, w, generator=g)
    kind = torch.randint(0, 4, (B, h, w), generator=g)
    n = B * h * w
    if n >= 4:                          # each kind at least once wherever there is room
        first = torch.randperm(n, generator=g)[:4]
        kind.view(-1)[first] = torch.arange(4)
    drop = torch.rand(B, D, h, w, generator=g) < 0.3
    drop[:, 0] |= ~drop.any(1)                                   # "some": at least one
    if D > 1:
        full = drop.all(1)
        drop[:, D - 1] &= ~full                                  # ... and not all
    raw = torch.where((kind == 1)[:, None] & drop, torch.zeros(()), raw)
    raw = torch.where((kind == 2)[:, None], torch.zeros(()), raw)
    if D >= 2:
        lo = 0.01 + 0.03 * torch.rand(B, h, w, generator=g)      # below every other bin
        reps = torch.randint(2, 4, (B, h, w), generator=g).clamp(max=D)
        order = torch.rand(B, D, h, w, generator=g).argsort(1)   # a random permutation of the bins per pixel
        rank = order.argsort(1)
        tie = (kind == 3)[:, None] & (rank < reps[:, None])
        raw = torch.where(tie, lo[:, None].expand_as(raw), raw)
        if D >= 4:
            zero = (kind == 3)[:, None] & (rank == D - 1) & (torch.rand(B, 1, h, w, generator=g) < 0.5)
            raw = torch.where(zero, torch.zeros(()), raw)
    return raw.contiguous()


def reduce_pixel_kinds(raw):
    """dict of [B,h,w] bool maps computed from the volume itself."""
    D = raw.shape[1]
    nz = (raw == 0).sum(1)
    pos_min = torch.where(raw > 0, raw, torch.full_like(raw, float("inf"))).min(1, keepdim=True)[0]
    ties = ((raw == pos_min) & (raw > 0)).sum(1)
    return dict(all_positive=nz == 0, some_zero=(nz > 0) & (nz < D), all_zero=nz == D, tie=ties >= 2,
                tie_with_zero=(ties >= 2) & (nz > 0))


def reduce_reference(raw, bins, R):
    """set_missing_to_max as in R.cost_volume, then R.cost_volume_reduce, fp32 -> (masked, conf, argmin, lowest)."""
    miss = (raw == 0).float()
    filled = raw * (1 - miss) + raw.max(1)[0][:, None] * miss
    conf, idx, lowest, masked = R.cost_volume_reduce(filled, miss, bins)
    return masked, conf, idx, lowest


# ---------------------------------------------------------------------------------------------
# the cases both test files run (shape -> seed where a property of the seeded input is asserted on the CPU)
# ---------------------------------------------------------------------------------------------
GRID_SHAPES = [(5, 9, 5, 9, 3), (9, 17, 6, 11, 1), (5, 5, 13, 21, 4), (17, 9, 3, 3, 16),      # (Hi, Wi, Ho, Wo, C)
               (1, 9, 4, 6, 3), (5, 1, 4, 6, 3)]                                             # one-pixel axis
GRID_SEEDS = {s: 100 + i for i, s in enumerate(GRID_SHAPES)}
SMOOTH_SHAPES = [(1, 3, 2, 2), (2, 1, 2, 7), (2, 3, 7, 2), (3, 3, 17, 63), (3, 3, 96, 457)]   # (B, C, H, W)
SELECT_SHAPES = [(1, 3, 1, 1), (2, 1, 5, 7), (3, 3, 9, 29)]                                   # (B, C, H, W)
SELECT_SEEDS = {s: 200 + i for i, s in enumerate(SELECT_SHAPES)}
TAIL_SHAPES = [(3, 3, 5), (1, 1, 1), (2, 7, 73), (2, 192, 684)]                               # (B, H, W)
REDUCE_SHAPES = [(1, 1, 1, 1), (2, 7, 5, 9), (2, 96, 16, 17)]                                 # (B, D, h, w)
