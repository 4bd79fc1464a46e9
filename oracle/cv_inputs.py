"""TEST INFRASTRUCTURE ONLY -- the row table, seeded inputs, float64 reference, per-element error bound and fp32 emulation of
the plane-sweep cost volume, csrc/cost_volume.hip: cost_volume_fwd<F, DB, PK, RING>, F = 1 .. 4 lookup frames (DB = 4, 2, 1, 1
bins per thread), fp32 features or bf16 channel pairs, frames in [B][F] order or in a ring.  Pure torch on the CPU; everything
is a function of the row and its seed.

THE OPERATION (the reference's replk_matching_adapter.py:261-340, written here from its definition, in double).  Per item b,
lookup frame f, bin d and pixel (px, py):  ray = inv_K[:3, :3] (px, py, 1);  X = depth_d ray;  cam = P X + P[:, 3] with
P = (K @ T_f)[:3] (formed in double and rounded once to the fp32 operand the entry points take: the kernel never sees K or T);
iz = cam_z + eps;  gx = ((cam_x / iz) / (w - 1) - 0.5) 2;  xv = (gx / 2 + 0.5)(w - 1) (the edge-mask position);
ix = ((gx + 1) / 2)(w - 1) (grid_sample's, align_corners) -- likewise in y;  warped = bilinear sample of lookup_f at (ix, iy),
zero outside the map;  diff_f = mean_c |warped - cur| * [2 <= xv <= w - 2][2 <= yv <= h - 2] * [2 <= px < w - 2][2 <= py < h - 2];
cost = (sum_f diff_f) / (#{f: diff_f > 0} + 1e-7) over the frames that are not skipped.

THE BOUND, per element.  u = 2^-24 (fp32, round to nearest), g_k = k u / (1 - k u).
(a) Position.  Every fp32 operation of the chain from (px, py) to xv, yv, ix, iy is followed with a running error: a quantity
    with double value v carries e >= |fp32 value - v|;  sum: e = ea + eb, product: e = |a| eb + |b| ea + ea eb,
    quotient: e = (ea + |q| eb) / (|b| - eb) (infinite where |b| <= eb: cam_z + eps cancels), each followed by
    e += u (|v| + e) for the rounding of the result; scalings by 2 and 1/2 round nothing.  A fused multiply-add rounds once
    where the unfused pair rounds twice, so the bound holds for either (the library is built without contraction).
(b) |bilinear(p) - bilinear(p')| <= Sx |dx| + Sy |dy| for a continuous piecewise-bilinear surface, Sx (Sy) the largest
    horizontal (vertical) difference of neighbouring texels over the cells the segment p p' can touch: the sample's own cell and
    its eight neighbours (|dx|, |dy| << 1).  ||a - c| - |b - c|| <= |a - b|, so diff_f moves by at most
    mean_c(Sx) ex + mean_c(Sy) ey, (ex, ey) the bound of (a) on (ix, iy).
(c) fp32 rounding at the fp32 position: tx = ix - floor(ix) is exact; a weight is up to two rounded factors and a rounded
    product (3 roundings), a term one more product (1), the four-term sum three additions (3): the warped value is within
    g_7 * bilinear(|lookup|) of the exact bilinear value;  the subtraction of cur adds u |warped - cur|, |.| nothing, the
    channel sum is in double (2^-53: nothing visible), the conversion of the mean to float adds u diff_f:
    e_f = mean_c(Sx) ex + mean_c(Sy) ey + g_7 bilinear(mean_c |lookup|) + 2 u diff_f.
    The epilogue adds F - 1 fp32 sums, `count + 1e-7f` and one division, F + 1 roundings:
    |got - cost| <= (1 + g_(F+1)) (sum_f e_f) / (n + 1e-7) + g_(F+1) cost,  n the number of contributing frames.
    Where no frame contributes the kernel stores 0.0f: bound 0.
On the EXACT rows every operation of (a) is exact: (w - 1, h - 1) = (32, 16), focal length 16, principal point (16, 8), bins
powers of two, translations multiples of 1 / 16 of a bin: `exact_positions_hold` asserts that every intermediate of the fp32
chain equals the double chain bit for bit (a 24-bit result that both precisions agree on is the exact one: a product of two
fp32 has 48 bits, a quotient that is not representable differs from every 24-bit number by more than 2^-53 of itself), so (a)
is 0 there, fused or not, and no mask decision is open.

UNDECIDED FRAMES.  A frame of an entry whose double xv (yv) lies within its own bound of 2, w - 2 (h - 2), the bound not
being 0, may be inside or outside the edge mask: the entry passes if it is within the bound of one of the <= 2^F values the
open decisions allow.  An entry whose bound is above VACUOUS = 5 % of the row's mean non-zero cost says nothing and is left out.
CAP: undecided + left-out entries are at most 2 % of a row (a condition on the table, asserted from the reference alone).
NaN and Inf are outside every bound.  Not in scope: the value where cam_z + eps == 0 exactly (`no_degenerate_depth`).

INPUTS THAT MAKE INDEX ERRORS VISIBLE.  Features are randn with planes alternating in scale by 4 over (item, frame) and over
channel parity (a neighbouring plane, a swapped channel pair, a frame read from another slot land far outside the bound); the
lookup map of every skipped frame is NaN (a skipped frame that is read shows).  `evaluate` is the kernel's arithmetic in
vectorised fp32 torch (same expression trees, channel sum in double, frames in order) and takes a `fault` of FAULTS:
tests/test_cv_arms_cpu.py shows that each fault leaves the bound on every row where it applies."""
import collections
import itertools
import math

import torch
import torch.nn.functional as F_

from oracle.dwconv_inputs import guarded, guards_intact, worst  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
EPS7 = float(torch.tensor(1e-7, dtype=torch.float32))        # 1e-7f, the kernel's and the default eps
VACUOUS = 0.05
CAP = 0.02
DB_OF = {1: 4, 2: 2, 3: 1, 4: 1}
INT32_MAX = 2 ** 31 - 1


def gamma(k):
    return k * U / (1 - k * U)


Row = collections.namedtuple("Row", "name B F C h w D dtype form eps what opts")


def instantiation(r):
    """cost_volume_fwd<F, DB, PK, RING>"""
    return (r.F, DB_OF[r.F], r.dtype == "bf16", r.form == "ring")


ALL_INSTANTIATIONS = frozenset((F, DB_OF[F], pk, ring) for F in (1, 2, 3, 4) for pk in (False, True) for ring in (False, True))
# D every DB has to see: nd = min(DB, D - d0) of the last group
REQUIRED_TAILS = {1: (1, 2, 3, 5, 6, 7), 2: (1, 3), 3: (1,), 4: (1,)}


def _r(name, B, F, C, h, w, D, dtype="f32", form="multi", eps=EPS7, what="", **opts):
    return Row(name, B, F, C, h, w, D, dtype, form, eps, what, opts)


# opts: t0 / dt: translation of frame f = t0 + f dt (+ 0.02 b in x);  rot: rotation about y and z of frame f (radians, x (f+1));
#       bins: (lo, hi) log-spaced, or a tuple of D values;  centre: principal point ((w-1)/2, (h-1)/2), focal (0.58 w, 0.96 h);
#       skip: ((b, f), ..) flagged frames;  off: ((b, f), ..) frames that project off the map;  equal: item 0's frames are one
#       frame;  exact: "int" | "half";  head, seen, skipnull: the ring's state words and a NULL skip
_GEN = dict(t0=(0.30, 0.04, 0.30), dt=(-0.25, 0.03, -0.15), rot=(0.010, 0.006), bins=(0.5, 10.0))
_SMALL = dict(t0=(0.10, 0.05, 0.10), dt=(0.03, 0.02, 0.05), rot=(0.0, 0.0), bins=(0.5, 10.0), centre=True)


def _generic_rows():
    rows = []
    for F in (1, 2, 3, 4):
        for dtype in ("f32", "bf16"):
            for form in ("multi", "ring"):
                o = dict(_GEN, skip=((1, 0),) if F > 1 else ())
                if form == "ring":
                    o.update(head=F - 1, seen=(F, F, max(F - 1, 1)))
                rows.append(_r(f"gen_f{F}_{dtype}_{form}", 3, F, 8 if dtype == "f32" else 6, 21, 37, 13, dtype, form,
                               what="one generic row per instantiation: ragged map, three blocks, D = 13", **o))
    return rows


def _tail_rows():
    rows = []
    for F, Ds in REQUIRED_TAILS.items():
        for i, D in enumerate(Ds):
            dtype = ("f32", "bf16")[(i + F) % 2]
            rows.append(_r(f"tail_f{F}_d{D}", 2, F, 4, 9, 31, D, dtype, "multi",
                           what=f"bin tail: D = {D} against DB = {DB_OF[F]}", **_GEN))
    return rows


def _exact(name, B, F, D, bins, trans, what, dtype="f32", form="multi", **o):
    return _r(name, B, F, 4, 17, 33, D, dtype, form, eps=0.0, what=what, exact=True, bins=bins, trans=trans, **o)


ROWS = tuple(
    _generic_rows() + _tail_rows() + [
        # maps
        _r("map_5x5", 2, 2, 4, 5, 5, 5, "f32", "multi", what="smallest map: one interior pixel", **_SMALL),
        _r("map_5x5_bf16_ring", 2, 1, 4, 5, 5, 3, "bf16", "ring", what="smallest map, pairs, ring", head=0, seen=(1, 1), **_SMALL),
        _r("map_5x37", 2, 3, 4, 5, 37, 4, "f32", "multi", what="h = 5: one interior row", **_SMALL),
        _r("map_21x5", 2, 1, 6, 21, 5, 6, "bf16", "multi", what="w = 5: one interior column", **_SMALL),
        _r("map_hw_below_block", 2, 2, 4, 11, 23, 5, "f32", "multi", what="hw = 253 < 256: one partial block", **_GEN),
        _r("map_hw_over_block", 2, 4, 4, 13, 20, 3, "bf16", "multi", what="hw = 260: a second block of 4 threads", **_GEN),
        # channels
        _r("ch_f32_c1", 2, 1, 1, 9, 31, 5, "f32", "multi", what="fp32, C = 1", **_GEN),
        _r("ch_f32_c3", 2, 2, 3, 9, 31, 5, "f32", "multi", what="fp32, odd C", **_GEN),
        _r("ch_f32_c3_ring", 2, 3, 3, 9, 31, 5, "f32", "ring", what="fp32 ring, odd C", head=1, seen=(3, 3), **_GEN),
        _r("ch_pairs_c2", 2, 2, 2, 9, 31, 5, "bf16", "multi", what="pairs, C = 2: one dword per position", **_GEN),
        _r("ch_pairs_c30", 2, 1, 30, 21, 37, 13, "bf16", "multi", what="pairs, C = 30: odd pair count", **_GEN),
        _r("ch_f32_c32", 3, 2, 32, 21, 37, 13, "f32", "multi", what="the largest row: B = 3, C = 32", **_GEN),
        # skip patterns
        _r("skip_all_frames", 3, 3, 4, 9, 31, 5, "f32", "multi", what="every frame of item 1 skipped: zeros",
           **dict(_GEN, skip=((1, 0), (1, 1), (1, 2)))),
        _r("skip_each_in_turn", 3, 3, 4, 9, 31, 5, "bf16", "multi", what="F = 3: item b skips frame b",
           **dict(_GEN, skip=((0, 0), (1, 1), (2, 2)))),
        _r("skip_off_the_map", 2, 3, 4, 9, 31, 5, "f32", "multi",
           what="frames that project off the map count 0: the divisor is the others'", **dict(_GEN, off=((0, 1), (1, 0), (1, 2)))),
        _r("equal_frames", 2, 2, 4, 9, 31, 5, "f32", "multi",
           what="item 0: both frames the same map and pose -> the single-frame cost (the count divisor)", **dict(_GEN, equal=True)),
        _r("behind_camera", 2, 2, 4, 13, 29, 6, "f32", "multi", what="t_z = -1 with bins below 1: cam z < 0 for the near bins",
           t0=(0.2, 0.05, -1.0), dt=(-0.3, 0.02, -0.1), rot=(0.0, 0.0), bins=(0.30, 4.5)),
        # exact rows: every mask boundary hit exactly, eps = 0
        _exact("exact_f1", 2, 1, 4, (2.0, 4.0, 8.0, 16.0), (((2.0, 1.0),), ((-2.0, -1.0),)),
               "F = 1: item 0 on the upper, item 1 on the lower mask boundaries"),
        _exact("exact_f2", 1, 2, 4, (2.0, 4.0, 8.0, 16.0), (((2.0, 1.0), (-2.0, -1.0)),),
               "F = 2: the two opposite translations in one item"),
        _exact("exact_f2_bf16_ring", 1, 2, 4, (2.0, 4.0, 8.0, 16.0), (((2.0, 1.0), (-2.0, -1.0)),),
               "the same through the pair ring", "bf16", "ring", head=1, seen=(2,)),
        _exact("exact_half", 2, 2, 1, (16.0,), (((0.5, 0.5), (-1.5, -0.5)), ((0.5, 1.0), (1.0, -1.5))),
               "half-pixel shifts (16 t / depth = k + 0.5): weights 0.25 (item 0) and 0.5 (item 1) exactly"),
        # ring state words
        _r("ring_head_minus1", 2, 3, 4, 9, 31, 5, "f32", "ring", what="head word -1", head=-1, seen=(3, 3), **_GEN),
        _r("ring_head_F", 2, 2, 4, 9, 31, 5, "bf16", "ring", what="head word F", head=2, seen=(2, 2), **_GEN),
        _r("ring_head_F_plus2", 2, 4, 4, 9, 31, 5, "f32", "ring", what="head word F + 2", head=6, seen=(4, 4), **_GEN),
        _r("ring_head_int_max", 2, 3, 4, 9, 31, 5, "bf16", "ring", what="head word 2^31 - 1", head=INT32_MAX, seen=(3, 3), **_GEN),
        _r("ring_seen_edges", 4, 3, 4, 9, 31, 5, "f32", "ring", what="seen 0, negative, above F, and 1 of 3",
           head=2, seen=(0, -3, 8, 1), **_GEN),
        _r("ring_seen_edges_bf16", 4, 2, 4, 9, 31, 5, "bf16", "ring", what="seen 0, INT_MIN, INT_MAX, 1 of 2",
           head=1, seen=(0, -INT32_MAX - 1, INT32_MAX, 1), **_GEN),
        _r("ring_skip_null", 2, 2, 4, 9, 31, 5, "f32", "ring", what="skip == NULL", head=0, seen=(2, 1), skipnull=True, **_GEN),
        _r("ring_skip_array", 2, 2, 4, 9, 31, 5, "f32", "ring", what="the same with a skip array that flags (0, 1)",
           head=0, seen=(2, 1), **dict(_GEN, skip=((0, 1),))),
    ])
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _seed(r):
    s = 17
    for v in (r.B, r.F, r.C, r.h, r.w, r.D, sum(ord(ch) for ch in r.name)):
        s = (s * 1000003 + v) % (2 ** 31 - 1)
    return s


def bins_of(r):
    b = r.opts["bins"]
    if len(b) == r.D and r.opts.get("exact"):
        return torch.tensor(b, dtype=torch.float32)
    return torch.exp(torch.linspace(math.log(b[0]), math.log(b[1]), r.D)).float() if r.D > 1 else torch.tensor([b[0]])


def _rot(ay, az):
    cy, sy, cz, sz = math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    return Ry @ Rz


def camera(r):
    """-> K, inv_K [B,4,4] fp32 (inv_K: the double inverse rounded once), T [B,F,4,4] float64."""
    h, w, o = r.h, r.w, r.opts
    K = torch.eye(4, dtype=torch.float64)
    if o.get("exact"):
        K[0, 0] = K[1, 1] = 16.0
        K[0, 2], K[1, 2] = 16.0, 8.0
    else:
        K[0, 0], K[1, 1] = 0.58 * w, 0.96 * h
        K[0, 2], K[1, 2] = ((w - 1) / 2, (h - 1) / 2) if o.get("centre") else (0.5 * w, 0.5 * h)
    K = K.float()
    inv_K = torch.linalg.inv(K.double()).float()
    T = torch.eye(4, dtype=torch.float64).repeat(r.B, r.F, 1, 1)
    for b in range(r.B):
        for f in range(r.F):
            if o.get("exact"):
                T[b, f, 0, 3], T[b, f, 1, 3] = o["trans"][b][f]
                continue
            g = 0 if (o.get("equal") and b == 0) else f
            T[b, f, :3, :3] = _rot(o["rot"][0] * (g + 1), o["rot"][1] * (g + 1))
            for q in range(3):
                T[b, f, q, 3] = o["t0"][q] + g * o["dt"][q] + (0.02 * b if q == 0 else 0.0)
            if (b, f) in o.get("off", ()):
                T[b, f, 0, 3] = 50.0
    return K[None].repeat(r.B, 1, 1), inv_K[None].repeat(r.B, 1, 1), T


def make_inputs(r):
    """-> dict: cur [B,C,h,w], look [B,F,C,h,w] (fp32, or bf16 for the pair rows; NaN maps where the frame is skipped), K, inv_K
    [B,4,4], T [B,F,4,4] double, P [B,F,3,4] fp32, bins [D], skip [B,F] int32 (the effective one: flags or-ed with the seen
    counts), and for ring rows ring [F,B,C,h,w], state [1+B] int32, skip_arg (the skip array the entry gets, or None)."""
    g = torch.Generator().manual_seed(_seed(r))
    B, F, C, h, w, o = r.B, r.F, r.C, r.h, r.w, r.opts
    dt = torch.bfloat16 if r.dtype == "bf16" else torch.float32
    par = torch.where(torch.arange(C) % 2 == 1, 4.0, 1.0)[:, None, None]
    cur = torch.randn(B, C, h, w, generator=g) * par
    look = torch.randn(B, F, C, h, w, generator=g) * par
    bf = torch.arange(B)[:, None] + torch.arange(F)[None, :]
    look = look * torch.where(bf % 2 == 1, 0.25, 1.0)[:, :, None, None, None]
    if o.get("equal"):
        look[0, 1] = look[0, 0]
    K, inv_K, T = camera(r)
    P = torch.matmul(K.double()[:, None], T)[:, :, :3, :].float().contiguous()
    flags = torch.zeros(B, F, dtype=torch.int32)
    for b, f in o.get("skip", ()):
        flags[b, f] = 1
    skip = flags.clone()
    inp = dict(K=K, inv_K=inv_K, T=T, P=P, bins=bins_of(r))
    if r.form == "ring":
        seen = torch.tensor(o["seen"], dtype=torch.int64)
        skip = (skip.bool() | (seen[:, None] <= torch.arange(F)[None, :])).to(torch.int32)
        inp["state"] = torch.tensor([o["head"]] + list(o["seen"]), dtype=torch.int64).to(torch.int32)
        inp["skip_arg"] = None if o.get("skipnull") else flags
    look[skip.bool()] = float("nan")
    cur, look = cur.to(dt), look.to(dt)
    if r.form == "ring":
        ring = torch.empty(F, B, C, h, w, dtype=dt)
        for f in range(F):
            ring[slot_of(o["head"], f, F)] = look[:, f]
        inp["ring"] = ring
    inp.update(cur=cur, look=look, skip=skip)
    return inp


def from_tensors(name, cur, look, poses, K, inv_K, bins, eps=EPS7):
    """A row and its inputs from tensors as `ops.cost_volume_multi` takes them (fp32; a zeroed pose = that frame skipped)."""
    B, F, C, h, w = look.shape
    r = _r(name, B, F, C, h, w, bins.shape[0], eps=eps, what="given tensors")
    P = torch.matmul(K.double()[:, None], poses.double())[:, :, :3, :].float().contiguous()
    skip = (poses.reshape(B, F, -1).sum(2) == 0).to(torch.int32)
    return r, dict(cur=cur, look=look, K=K, inv_K=inv_K, T=poses.double(), P=P, bins=bins.float(), skip=skip)


def boundary_hits(r, ref):
    """Exact rows: samples of interior pixels whose double xv (yv) equals 2, w - 2 (2, h - 2), summed over the bins ->
    dict(x_lo, x_hi, y_lo, y_hi) of per-bin count lists."""
    inner = inner_mask(r)[None]
    out = dict(x_lo=[0] * r.D, x_hi=[0] * r.D, y_lo=[0] * r.D, y_hi=[0] * r.D)
    for p in ref.pos.values():
        for key, v, c in (("x_lo", p["xv"].v, 2.0), ("x_hi", p["xv"].v, r.w - 2.0), ("y_lo", p["yv"].v, 2.0),
                          ("y_hi", p["yv"].v, r.h - 2.0)):
            for d, n in enumerate(((v == c) & inner).sum(1).tolist()):
                out[key][d] += n
    return out


def slot_of(head_word, f, F, off_by_one=False):
    """Ring slot of lookup frame f: (head - 1 - f) mod F with the head word brought into 0 .. F - 1 first."""
    return (head_word % F - (0 if off_by_one else 1) - f) % F


def pack_pairs(x):
    """bf16 [.., C, h, w], C even -> int32 [.., C/2, h, w]: channel 2c in the low half, 2c + 1 in the high half."""
    bits = x.view(torch.int16).to(torch.int32) & 0xffff
    return (bits[..., 0::2, :, :] | (bits[..., 1::2, :, :] << 16)).contiguous()


def ring_advance_ref(state, F):
    """The three-line integer reference of cv_ring_advance."""
    head = (state[0] % F + 1) % F
    seen = [min(max(s, 0) + 1, F) for s in state[1:]]
    return [head] + seen


# ---------------------------------------------------------------------------------------------
# positions: the double chain with its running fp32 error, and the fp32 chain itself
# ---------------------------------------------------------------------------------------------
class _RE:
    """value (float64) and a bound on |fp32 value - value|"""
    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e


def _rnd(v, e):
    return _RE(v, e + U * (v.abs() + e))


def _add(a, b):
    return _rnd(a.v + b.v, a.e + b.e)


def _mul(a, b):
    return _rnd(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)


def _div(a, b):
    q = a.v / b.v
    den = b.v.abs() - b.e
    e = torch.where(den > 0, (a.e + q.abs() * b.e) / den.clamp_min(1e-300), torch.full_like(q, float("inf")))
    return _rnd(q, e)


def _scale(a, k):
    return _RE(a.v * k, a.e * k)


def _c(x, like):
    return _RE(torch.full_like(like, float(x)))


def _pixels(h, w, dtype):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    return xs.reshape(-1), ys.reshape(-1)


def positions64(r, inp, b, f):
    """-> dict of _RE [D, hw]: xv, yv, ix, iy, iz of item b, frame f: double values with the bound (a)."""
    xs, ys = _pixels(r.h, r.w, torch.float64)
    ik, pm = inp["inv_K"][b].double(), inp["P"][b, f].double()
    fx, fy = _RE(xs[None]), _RE(ys[None])
    ray = [_add(_add(_mul(_c(ik[k, 0], xs[None]), fx), _mul(_c(ik[k, 1], xs[None]), fy)), _c(ik[k, 2], xs[None])) for k in range(3)]
    depth = _RE(inp["bins"].double()[:, None].expand(r.D, r.h * r.w).contiguous())
    X = [_mul(depth, _RE(q.v.expand(r.D, -1), q.e.expand(r.D, -1))) for q in ray]
    one = X[0].v
    cam = [_add(_add(_add(_mul(_c(pm[q, 0], one), X[0]), _mul(_c(pm[q, 1], one), X[1])), _mul(_c(pm[q, 2], one), X[2])),
                _c(pm[q, 3], one)) for q in range(3)]
    iz = _add(cam[2], _c(r.eps, one))
    out = dict(iz=iz)
    for name, c, n in (("x", cam[0], r.w - 1), ("y", cam[1], r.h - 1)):
        gq = _scale(_add(_div(_div(c, iz), _c(n, one)), _c(-0.5, one)), 2.0)
        out[name + "v"] = _mul(_add(_scale(gq, 0.5), _c(0.5, one)), _c(n, one))
        out["i" + name] = _mul(_scale(_add(gq, _c(1.0, one)), 0.5), _c(n, one))
    return out


def positions32(r, inp, b, f, pose_from=None, trace=None):
    """The kernel's fp32 chain -> xv, yv, ix, iy [D, hw] float32 (`trace`: a list that receives every intermediate)."""
    xs, ys = _pixels(r.h, r.w, torch.float32)
    ik, pm = inp["inv_K"][b], inp["P"][b, f if pose_from is None else pose_from]
    ray = [(ik[k, 0] * xs + ik[k, 1] * ys) + ik[k, 2] for k in range(3)]
    depth = inp["bins"][:, None]
    X = [depth * q[None] for q in ray]
    cam = [((pm[q, 0] * X[0] + pm[q, 1] * X[1]) + pm[q, 2] * X[2]) + pm[q, 3] for q in range(3)]
    iz = cam[2] + torch.tensor(r.eps, dtype=torch.float32)
    wm, hm = float(r.w - 1), float(r.h - 1)
    ax, ay = cam[0] / iz, cam[1] / iz
    gx, gy = (ax / wm - 0.5) * 2.0, (ay / hm - 0.5) * 2.0
    xv, yv = (gx / 2.0 + 0.5) * wm, (gy / 2.0 + 0.5) * hm
    ix, iy = ((gx + 1.0) / 2.0) * wm, ((gy + 1.0) / 2.0) * hm
    if trace is not None:
        trace += ray + X + cam + [iz, ax, ay, ax / wm, ay / hm, gx, gy, gx / 2.0 + 0.5, gy / 2.0 + 0.5, gx + 1.0, gy + 1.0,
                                  xv, yv, ix, iy]
    return xv, yv, ix, iy


def _trace64(r, inp, b, f):
    """positions32's intermediates by the same expressions in double."""
    xs, ys = _pixels(r.h, r.w, torch.float64)
    ik, pm = inp["inv_K"][b].double(), inp["P"][b, f].double()
    ray = [(ik[k, 0] * xs + ik[k, 1] * ys) + ik[k, 2] for k in range(3)]
    depth = inp["bins"].double()[:, None]
    X = [depth * q[None] for q in ray]
    cam = [((pm[q, 0] * X[0] + pm[q, 1] * X[1]) + pm[q, 2] * X[2]) + pm[q, 3] for q in range(3)]
    iz = cam[2] + r.eps
    wm, hm = float(r.w - 1), float(r.h - 1)
    ax, ay = cam[0] / iz, cam[1] / iz
    gx, gy = (ax / wm - 0.5) * 2.0, (ay / hm - 0.5) * 2.0
    return ray + X + cam + [iz, ax, ay, ax / wm, ay / hm, gx, gy, gx / 2.0 + 0.5, gy / 2.0 + 0.5, gx + 1.0, gy + 1.0,
                            (gx / 2.0 + 0.5) * wm, (gy / 2.0 + 0.5) * hm, ((gx + 1.0) / 2.0) * wm, ((gy + 1.0) / 2.0) * hm]


def exact_positions_hold(r, inp):
    """Exact rows: every intermediate of the fp32 chain equals the double chain's, bit for bit, for every frame in use."""
    for b in range(r.B):
        for f in range(r.F):
            t32 = []
            positions32(r, inp, b, f, trace=t32)
            for a, d in zip(t32, _trace64(r, inp, b, f)):
                if not torch.equal(a.double(), d):
                    return False
    return True


def inner_mask(r, border=2):
    m = torch.zeros(r.h, r.w, dtype=torch.bool)
    m[border:r.h - border, border:r.w - border] = True
    return m.reshape(-1)


# ---------------------------------------------------------------------------------------------
# float64 reference with its bound
# ---------------------------------------------------------------------------------------------
def _bilinear64(maps, ix, iy, h, w):
    """maps [C, h, w] double, positions [D, hw] double -> [C, D, hw]: bilinear, zero outside the map (grid_sample, zeros,
    align_corners)."""
    ok = torch.isfinite(ix) & torch.isfinite(iy)
    ixc = torch.where(ok, ix, torch.zeros_like(ix)).clamp(-2.0, w + 1.0)
    iyc = torch.where(ok, iy, torch.zeros_like(iy)).clamp(-2.0, h + 1.0)
    x0, y0 = torch.floor(ixc), torch.floor(iyc)
    tx, ty = ixc - x0, iyc - y0
    x0, y0 = x0.long(), y0.long()
    flat = maps.reshape(maps.shape[0], -1)
    out = 0.0
    for dy, dx, wgt in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)), (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
        xx, yy = x0 + dx, y0 + dy
        inside = ok & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(-1)
        v = flat[:, idx].reshape(maps.shape[0], *ix.shape)
        out = out + torch.where(inside, wgt, torch.zeros_like(wgt))[None] * torch.where(inside[None], v, torch.zeros_like(v))
    return out, x0, y0


def _slopes(maps, h, w):
    """maps [C, h, w] double -> (Sx, Sy) [h + 1, w + 1]: at (y0, x0) the channel mean of the largest |difference| of horizontal
    (vertical) neighbours over the cell (y0, x0) and its eight neighbours, zeros outside the map."""
    vp = F_.pad(maps, (2, 2, 2, 2))
    hd = (vp[:, :, 1:] - vp[:, :, :-1]).abs()                  # [C, h + 4, w + 3]; column j: original columns j - 2, j - 1
    vd = (vp[:, 1:, :] - vp[:, :-1, :]).abs()                  # [C, h + 3, w + 4]
    sx = F_.max_pool2d(hd[None], (4, 3), 1)[0].mean(0)         # [h + 1, w + 1]; (r, j) = (y0 + 1, x0 + 1)
    sy = F_.max_pool2d(vd[None], (3, 4), 1)[0].mean(0)
    return sx, sy


Ref = collections.namedtuple("Ref", "cost diff edge undecided ebound pos bound counted n_undecided n_left_out mean_cost")


def reference(r, inp):
    """-> Ref: cost [B,D,hw] double; diff [B,F,D,hw]: the frame's mean |warp - cur| with the inner mask and the skip flags but
    NOT the edge mask applied; edge, undecided [B,F,D,hw] bool; ebound [B,F,D,hw]: e_f; pos: (b, f) -> positions64's dict;
    bound [B,D,hw] for the reference's own mask decisions; counted [B,D,hw] bool (not left out)."""
    B, F, C, h, w, D = r.B, r.F, r.C, r.h, r.w, r.D
    hw = h * w
    inner = inner_mask(r)
    diff = torch.zeros(B, F, D, hw, dtype=torch.float64)
    edge = torch.zeros(B, F, D, hw, dtype=torch.bool)
    und = torch.zeros(B, F, D, hw, dtype=torch.bool)
    eb = torch.zeros(B, F, D, hw, dtype=torch.float64)
    pos = {}
    for b in range(B):
        cur = inp["cur"][b].double().reshape(C, 1, hw)
        for f in range(F):
            if int(inp["skip"][b, f]):
                continue
            p = positions64(r, inp, b, f)
            pos[(b, f)] = p
            if r.opts.get("exact"):
                for q in ("xv", "yv", "ix", "iy"):
                    p[q] = _RE(p[q].v)                                   # (a) is 0: exact_positions_hold
            look = inp["look"][b, f].double()
            warped, x0, y0 = _bilinear64(look, p["ix"].v, p["iy"].v, h, w)
            d = (warped - cur).abs().mean(0)
            absw, _, _ = _bilinear64(look.abs().mean(0, keepdim=True), p["ix"].v, p["iy"].v, h, w)
            sx, sy = _slopes(look, h, w)
            yi, xi = y0.clamp(0, h - 1), x0.clamp(0, w - 1)
            ex, ey = p["ix"].e, p["iy"].e
            e = sx[yi + 1, xi + 1] * ex + sy[yi + 1, xi + 1] * ey + gamma(7) * absw[0] + 2 * U * d
            xv, yv, exv, eyv = p["xv"].v, p["yv"].v, p["xv"].e, p["yv"].e
            inside = (xv >= 2.0) & (xv <= w - 2) & (yv >= 2.0) & (yv <= h - 2)
            open_ = torch.zeros_like(inside)
            for v, ev, edges in ((xv, exv, (2.0, w - 2.0)), (yv, eyv, (2.0, h - 2.0))):
                for c in edges:
                    open_ |= ((v - c).abs() <= ev) & (ev > 0)
                open_ |= ~torch.isfinite(ev) | ~torch.isfinite(v)
            diff[b, f] = torch.where(inner[None], d, torch.zeros_like(d))
            edge[b, f] = inside & inner[None]
            und[b, f] = open_ & inner[None]
            eb[b, f] = torch.where(inner[None], e, torch.zeros_like(e))
    cost, bound = candidate(r, diff, eb, edge)
    nz = cost[cost > 0]
    mean_cost = float(nz.mean()) if nz.numel() else 0.0
    any_und = und.any(1)
    left = ~(bound <= VACUOUS * mean_cost)                              # NaN / Inf bounds are left out too
    return Ref(cost, diff, edge, und, eb, pos, bound, ~left, int((any_und & ~left).sum()), int(left.sum()), mean_cost)


def candidate(r, diff, eb, use):
    """Cost and bound [B,D,hw] with the frames `use` [B,F,D,hw] contributing."""
    z = torch.zeros_like(diff)
    d = torch.where(use, diff, z)
    n = (d > 0).sum(1).double()
    s = d.sum(1)
    e = torch.where(use, eb, z).sum(1)
    cost = s / (n + EPS7)
    g = gamma(r.F + 1)
    bound = torch.where(n > 0, (1 + g) * e / (n + EPS7) + g * cost, torch.zeros_like(cost))
    return cost, bound


def hold(r, ref, got):
    """got [B,D,h,w] (any float dtype) against the reference -> dict(ratio: worst err / bound over the counted entries that are
    not undecided, outside: counted entries outside every candidate's bound, undecided, left_out, max_err)."""
    got = got.detach().cpu().double().reshape(r.B, r.D, r.h * r.w)
    err = (got - ref.cost).abs()
    ok = err <= ref.bound
    any_und = ref.undecided.any(1)
    if bool(any_und.any()):
        for assign in itertools.product((False, True), repeat=r.F):
            a = torch.tensor(assign).view(1, r.F, 1, 1).expand_as(ref.edge)
            valid = ((a == ref.edge) | ref.undecided).all(1) & any_und
            if not bool(valid.any()):
                continue
            c, bnd = candidate(r, ref.diff, ref.ebound, a)
            ok |= valid & ((got - c).abs() <= bnd)
    decided = ref.counted & ~any_und
    ratio = torch.where(err == 0, torch.zeros_like(err), err / ref.bound.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    finite = err[decided & torch.isfinite(err)]
    return dict(ratio=float(ratio[decided].max()) if bool(decided.any()) else 0.0, outside=int((ref.counted & ~ok).sum()),
                undecided=ref.n_undecided, left_out=ref.n_left_out, max_err=float(finite.max()) if finite.numel() else 0.0)


def no_degenerate_depth(r, inp):
    """No sample of the row has cam z + eps == 0, in fp32 or in double (the value there is out of scope)."""
    for b in range(r.B):
        for f in range(r.F):
            if int(inp["skip"][b, f]):
                continue
            t = []
            positions32(r, inp, b, f, trace=t)
            if bool((t[9] == 0).any()) or bool((positions64(r, inp, b, f)["iz"].v == 0).any()):
                return False
    return True


# ---------------------------------------------------------------------------------------------
# the kernel's arithmetic in fp32 torch, and the faults the bound has to catch
# ---------------------------------------------------------------------------------------------
FAULTS = ("gt_for_ge", "lt_for_le", "swap_tx_ty", "corner_column_plus_one", "bottom_row_from_top", "frame_order_reversed_poses",
          "ring_slot_off_by_one", "count_skipped_frame", "tail_bin_unwritten", "pair_hi_lo_swapped", "inner_mask_one_pixel", "nan")


def fault_applies(r, fault):
    o = r.opts
    if fault in ("gt_for_ge", "lt_for_le"):                 # a set of measure zero on generic poses: the exact integer rows
        return bool(o.get("exact")) and r.D > 1
    if fault == "frame_order_reversed_poses":               # needs two frames with different poses
        return r.F > 1 and not o.get("equal")
    if fault == "ring_slot_off_by_one":
        return r.form == "ring" and r.F > 1
    if fault == "count_skipped_frame":                      # an item with a skipped frame and one that contributes
        sk = make_inputs(r)["skip"].bool()
        return bool((sk.any(1) & ~sk.all(1)).any())
    if fault == "pair_hi_lo_swapped":
        return r.dtype == "bf16"
    if fault == "inner_mask_one_pixel":                     # the second ring of pixels must have samples inside the edge mask
        return min(r.h, r.w) > 5 and not o.get("exact")
    if fault in ("swap_tx_ty", "corner_column_plus_one", "bottom_row_from_top"):
        return r.name != "exact_f1" and r.name != "exact_f2" and r.name != "exact_f2_bf16_ring"     # integer positions: weight 1 on one corner
    return True


def evaluate(r, inp, fault=None):
    """-> cost [B,D,h,w] float32 as the kernel computes it; `fault`: one of FAULTS, a wrong kernel's output."""
    B, F, C, h, w, D = r.B, r.F, r.C, r.h, r.w, r.D
    hw = h * w
    inner = inner_mask(r, 1 if fault == "inner_mask_one_pixel" else 2)
    out = torch.zeros(B, D, hw, dtype=torch.float32)
    ring = r.form == "ring"
    for b in range(B):
        cur = inp["cur"][b].float().reshape(C, 1, hw)
        total = torch.zeros(D, hw, dtype=torch.float32)
        count = torch.zeros(D, hw, dtype=torch.float32)
        for f in range(F):
            if ring:
                seen = int(inp["state"][1 + b])
                flagged = inp["skip_arg"] is not None and int(inp["skip_arg"][b, f]) != 0
                skipped = seen <= f or flagged
                look = inp["ring"][slot_of(int(inp["state"][0]), f, F, fault == "ring_slot_off_by_one"), b]
            else:
                skipped = int(inp["skip"][b, f]) != 0
                look = inp["look"][b, f]
            if skipped:
                if fault == "count_skipped_frame":
                    count = count + inner[None].float()
                continue
            look = look.float()
            if fault == "pair_hi_lo_swapped":
                look = look.reshape(C // 2, 2, h, w).flip(1).reshape(C, h, w)
            xv, yv, ix, iy = positions32(r, inp, b, f, pose_from=F - 1 - f if fault == "frame_order_reversed_poses" else None)
            lo_x, lo_y = (xv > 2.0, yv > 2.0) if fault == "gt_for_ge" else (xv >= 2.0, yv >= 2.0)
            hi_x, hi_y = (xv < float(w - 2), yv < float(h - 2)) if fault == "lt_for_le" else (xv <= float(w - 2), yv <= float(h - 2))
            m = lo_x & hi_x & lo_y & hi_y & inner[None]
            ixs, iys = torch.where(m, ix, torch.full_like(ix, 2.0)), torch.where(m, iy, torch.full_like(iy, 2.0))
            flx, fly = torch.floor(ixs), torch.floor(iys)
            tx, ty = ixs - flx, iys - fly
            if fault == "swap_tx_ty":
                tx, ty = ty, tx
            w00, w01, w10, w11 = (1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty
            x0, y0 = flx.long(), fly.long()
            flat = look.reshape(C, hw)

            def at(dy, dx):
                # zero fill outside the map, corner by corner: the kernel's last-column / last-row branch
                xx, yy = x0 + dx, y0 + dy
                inside = (xx < w) & (yy < h)
                v = flat[:, (yy.clamp(max=h - 1) * w + xx.clamp(max=w - 1)).reshape(-1)].reshape(C, D, hw)
                return torch.where(inside[None], v, torch.zeros_like(v))
            cx = 2 if fault == "corner_column_plus_one" else 1
            by = 0 if fault == "bottom_row_from_top" else 1
            warped = ((at(0, 0) * w00 + at(0, cx) * w01) + at(by, 0) * w10) + at(by, cx) * w11
            d = ((warped - cur).abs().double().sum(0) / float(C)).float()
            d = torch.where(m, d, torch.zeros_like(d))
            total = total + d
            count = count + (d > 0).float()
        out[b] = total / (count + torch.tensor(1e-7, dtype=torch.float32))
    if fault == "tail_bin_unwritten":
        out[:, D - 1] = float("nan")
    if fault == "nan":
        live = (out != 0).reshape(-1).nonzero()
        out.view(-1)[int(live[live.numel() // 2]) if live.numel() else out.numel() // 2] = float("nan")
    return out.reshape(B, D, h, w)


# ---------------------------------------------------------------------------------------------
# the kernel's last-column / last-row branch: can a sample inside the edge mask have floor(ix) + 1 >= w ?
# ---------------------------------------------------------------------------------------------
def rare_branch_count(r, inp):
    """-> (samples inside the edge mask, those of them with floor(ix) + 1 >= w or floor(iy) + 1 >= h) by the fp32 chain."""
    n = hit = 0
    for b in range(r.B):
        for f in range(r.F):
            if int(inp["skip"][b, f]):
                continue
            xv, yv, ix, iy = positions32(r, inp, b, f)
            m = (xv >= 2.0) & (xv <= float(r.w - 2)) & (yv >= 2.0) & (yv <= float(r.h - 2))
            n += int(m.sum())
            hit += int((m & ((torch.floor(ix) + 1 >= r.w) | (torch.floor(iy) + 1 >= r.h))).sum())
    return n, hit


def pose_sweep_rows():
    """A dense sweep of poses on the 5 x 5 and the 21 x 37 map: translations that push the samples across and onto the upper
    mask edge, with and without rotation, eps on and off."""
    rows = []
    for h, w in ((5, 5), (21, 37)):
        for i in range(40):
            for eps in (0.0, EPS7):
                t = (0.05 * i - 0.4, 0.03 * i - 0.3, 0.02 * (i % 7) - 0.05)
                rows.append(_r(f"sweep_{h}x{w}_{i}_{eps}", 1, 4, 1, h, w, 13, eps=eps, t0=t, dt=(0.013, 0.007, 0.011),
                               rot=(0.003 * (i % 5), 0.002 * (i % 3)), bins=(0.5, 10.0), centre=bool(i % 2)))
    return rows
