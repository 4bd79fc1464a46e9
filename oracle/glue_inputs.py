"""TEST INFRASTRUCTURE ONLY -- case tables, seeded inputs, float64 references and per-element error bounds for the stencil and
glue kernels that run between the pinned families: csrc/dwconv3x3.hip (forward, affine forward, data and filter gradient),
csrc/nhwc_decoder.hip (reflect pad, bias + ELU, upsample-cat in channels_last), csrc/bias_act.hip (NCHW bias + ELU),
csrc/pad.hip (NCHW reflect pad) and csrc/nhwc_pool.hip (the pose max-pool).  Pure torch; everything is a function of its
arguments and the seed.  Which stencil kernel a row reaches is NOT restated here: a row names the arm it claims and
tests/test_glue_arms_cpu.py asks the library's own query (ops.dwconv3x3_plan, the function both launchers switch on).  The
slab / chunk / part plans of the other kernels ARE restated (slab_plan, chunk_plan, wgrad_plan: the CPU file needs them to
emulate the partial sums) and both test files hold the restatement to the library's queries on every row.  The CPU file also
proves the census, the references against torch's own ops in double, that an honest fp32 run stays inside every bound and
that planted faults do not; tests/test_glue_arms_gpu.py runs every row on the device.

THE BOUNDS (derived as in oracle/conv_inputs.py, not tuned).  u = 2^-24 is the unit roundoff of fp32, U_ACC = 2^-23 = 2 u the
allowance per operation, U_BF16 = 2^-8 the unit roundoff of bf16.  A round-to-nearest result fl(v) obeys |fl(v) - v| <=
u / (1 + u) |v|, so a value v with |v - ref| <= e stored as bf16 lies within U_BF16 |ref| + e (1 + U_BF16) - U_BF16^2 / (1 +
U_BF16) |ref| of ref: with e counted at 2 u per operation where the arithmetic commits u, `e + U_BF16 |ref|` covers it.

    pure data movement            bit patterns, bound 0: both reflect-pad forwards, up2cat forward, the db half of up2cat
                                  backward, max-pool values (and its one-byte window index)
    sums of n fp32 terms          n * U_ACC * A, A = sum |terms|  (+ U_BF16 |ref| for a bf16 output); n:
        reflect-pad backward        9          (<= 9 padded positions mirror onto one pixel)
        up2cat da                   4
        max-pool backward           4          (a pixel lies in <= 4 windows)
        3x3 forward                 9
        3x3 affine forward          10         (s * conv + o: A = |s| A_conv + |o|; ReLU applied in double, 1-Lipschitz)
        3x3 data gradient           9 at stride 1, 4 at stride 2
        3x3 filter gradient         N * Ho * Wo  (the parts and their sum are N Ho Wo - 1 additions in all)
        bias-gradient partials      pixels per channel; the partials are added on the test side in float64 over all slabs /
                                    chunks.  The kernel sums the fp32 products BEFORE it rounds dz for storage: the reference
                                    is the double sum of the exact dz, not of the stored dz
    ELU forward                   v = fl(z + b) is within u |v| of the exact argument and ELU' = min(1, e^v):
                                  u |v| min(1, e^v); the positive branch adds nothing; the negative branch adds E_ELU, the
                                  absolute error of the device's expm1f; + U_BF16 |ref| for a bf16 output
    ELU backward                  the reference takes the STORED y as the kernel does: dz = dy * (y > 0 ? 1 : y + 1) in double;
                                  fl(y + 1) and the product are two roundings, (1 + u / (1 + u))^2 - 1 < 2 u = U_ACC:
                                  U_ACC |ref|  (+ U_BF16 |ref|)
    max-pool                      the reference computes its own window index: the first maximum in (row, column) scan order
                                  of the in-bounds window, updated on every NaN (torch's rule); the gradient is gathered in
                                  double.  The CPU file holds the index to F.max_pool2d(..., return_indices=True)

E_ELU is the one number that cannot be derived from the project.  Measured on the CPU (torch float32 expm1 against float64):
over EVERY negative finite bf16 value 5.32e-8, over a dense fp32 grid of 2e7 points on [-104, 0) (the rows' argument range:
|z| <= 6 and the planted -100, |b| <= 4) 5.96e-8 = 2^-24, over 2e6 points spaced logarithmically on [-1, -2^-30] 2.99e-8:
    E_ELU = 4 * 5.96e-8 = 2.384e-7
The margin of 4 is for a device function that is not correctly rounded.  tests/test_glue_arms_cpu.py measures it again.
Every element is held to its own bound; none may lie outside.
"""
import collections
import math

import torch
import torch.nn.functional as F

from oracle.conv_inputs import U_ACC, U_BF16, worst  # noqa: F401  (worst: re-exported for the tests)
from oracle.dwconv_inputs import GUARD, GUARD_BITS, guarded, guards_intact  # noqa: F401  (re-exported for the tests)

U_F32 = 2.0 ** -24
E_ELU_MEASURED, ELU_RANGE = 5.96e-8, 104.0
E_ELU = 4 * E_ELU_MEASURED
BF16, F32 = torch.bfloat16, torch.float32
ERR_UNSUPPORTED = -1

# the arms of ppea_dwconv3x3_plan and its modes
GENERIC, V_S1, V_S2_FWD, V_S2_BWD = 0, 1, 2, 3
ALL_DW3_ARMS = frozenset((GENERIC, V_S1, V_S2_FWD, V_S2_BWD))
DW3_ARM_NAMES = {GENERIC: "dw3 generic", V_S1: "dw3v_s1", V_S2_FWD: "dw3v_s2_fwd", V_S2_BWD: "dw3v_s2_bwd", None: "refused"}
MODE_FWD, MODE_BWD, MODE_AFFINE = 0, 1, 2


def dt_of(name):
    return BF16 if name == "bf16" else F32


def _gen(*vals):
    s = 47
    for v in vals:
        v = sum(ord(ch) for ch in v) if isinstance(v, str) else int(v)
        s = (s * 1000003 + v) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _randn(shape, dt, g, scale=1.0):
    return (scale * torch.randn(shape, generator=g)).to(dt)


def _bound(ref, term, dt):
    return term + (U_BF16 * ref.abs() if dt == BF16 else 0.0)


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def check(got, ref, bound):
    """-> (worst err / bound, elements outside).  bound None: bit equality with `ref` (same dtype)."""
    if bound is None:
        assert got.dtype == ref.dtype, (got.dtype, ref.dtype)
        bad = int((bits(got) != bits(ref)).sum())
        return (float("inf") if bad else 0.0), bad
    return worst(got, ref, bound if torch.is_tensor(bound) else torch.full_like(ref, bound))


def guarded_u8(shape, device):
    """The max-pool index: 0xFF-filled (no window index) inside guards of 0x5A."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=device)
    body = buf[GUARD:GUARD + n]
    body.fill_(0xFF)
    return buf, body.view(shape)


def guards_ok(buf, dtype):
    if dtype == torch.uint8:
        return bool((buf[:GUARD] == 0x5A).all()) and bool((buf[-GUARD:] == 0x5A).all())
    return guards_intact(buf, dtype)


def special_bits(shape, dt, g):
    """Arbitrary bit patterns with NaN payloads, +-Inf, denormals and -0.0 planted: what a pure copy must carry unchanged."""
    n = math.prod(shape)
    if dt == BF16:
        t = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g, dtype=torch.int32).to(torch.int16)
        sp = torch.tensor([0x7FC0, 0x7FA5, 0xFFC1 - 65536, 0x7F80, 0xFF80 - 65536, 0x0001, 0x8001 - 65536, 0x007F, 0x8000 - 65536, 0x7F81],
                          dtype=torch.int16)
    else:
        t = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
        sp = torch.tensor([0x7FC00000, 0x7FA5A5A5, 0xFFC00001 - 2 ** 32, 0x7F800000, 0xFF800000 - 2 ** 32, 1, 0x80000001 - 2 ** 32,
                           0x007FFFFF, 0x80000000 - 2 ** 32, 0x7F800001], dtype=torch.int32)
    k = min(n, 3 * len(sp))
    t[torch.arange(k) * (n // k)] = sp[torch.arange(k) % len(sp)]
    return t.view(dt).view(shape)


# =============================================================================================
# 3x3 depthwise stencil: forward, affine forward (relu 0 and 1) and data gradient of one (dtype, shape, stride)
# =============================================================================================
Dw = collections.namedtuple("Dw", "name dt N C H W stride arm_fwd arm_bwd why")
# arm_fwd: the claimed arm of the forward AND the affine forward;  arm_bwd: of the data gradient;  None: refused


def _dw_rows():
    G = GENERIC
    spec = (
        # (tag, N, C, H, W, {stride: (bf16 forward arm, bf16 data-gradient arm)}, why)
        ("1x1", 2, 3, 1, 1, {1: (G, G), 2: (G, G)}, "one pixel: every tap but the centre outside"),
        ("1x5", 2, 3, 1, 5, {1: (G, G), 2: (G, G)}, "one row"),
        ("7x9", 2, 3, 7, 9, {1: (G, G), 2: (G, G)}, "odd sizes, N C = 6 planes of C = 3: plane % C wraps"),
        ("130x127_cap", 1, 2, 130, 127, {1: (G, G), 2: (G, G)}, "a plane above 16384 pixels: the 64-block cap, the grid-stride loop"),
        ("259x255_cap_s2", 1, 1, 259, 255, {2: (G, G)}, "stride 2 with above 16384 OUTPUTS: the forward's grid-stride loop"),
        ("v_w8", 2, 3, 5, 8, {1: (V_S1, V_S1)}, "one vector tile, both halos zero"),
        ("v_w16", 2, 3, 5, 16, {1: (V_S1, V_S1)}, "two tiles: one halo each"),
        ("v_w40", 1, 3, 4, 40, {1: (V_S1, V_S1)}, "five tiles: inner tiles with both halos"),
        ("v_h1", 2, 2, 1, 16, {1: (V_S1, V_S1)}, "H = 1: only the centre row of taps"),
        ("v_h2", 2, 2, 2, 24, {1: (V_S1, V_S1)}, "H = 2"),
        ("v_2x16", 2, 3, 2, 16, {1: (V_S1, V_S1), 2: (V_S2_FWD, V_S2_BWD)}, "stride 2: one output row, one tile"),
        ("v_6x48", 2, 3, 6, 48, {2: (V_S2_FWD, V_S2_BWD)}, "stride 2: three tiles per output row"),
        ("v_4x32", 2, 3, 4, 32, {1: (V_S1, V_S1), 2: (V_S2_FWD, V_S2_BWD)}, "stride 2: two tiles"),
        ("v_blocks", 2, 5, 16, 64, {1: (V_S1, V_S1), 2: (V_S2_FWD, V_S2_BWD)}, "several blocks, the last one ragged"),
        ("fb_5x32", 2, 3, 5, 32, {2: (G, G)}, "bf16 stride 2 with odd H falls back to the generic kernel"),
        ("fb_6x24", 2, 3, 6, 24, {2: (G, G)}, "bf16 stride 2 with Wo % 8 != 0 falls back"),
        ("fb_6x17", 2, 3, 6, 17, {2: (G, G)}, "bf16 stride 2 with odd W falls back"),
        ("c1", 3, 1, 4, 16, {1: (V_S1, V_S1), 2: (V_S2_FWD, V_S2_BWD)}, "C = 1, N = 3"),
        ("stride3", 2, 3, 7, 9, {3: (None, None)}, "refused: stride 3"),
        ("planes65536", 256, 256, 1, 1, {1: (None, None), 2: (None, None)}, "refused: N C = 65536 planes"),
    )
    rows = []
    for tag, N, C, H, W, by_stride, why in spec:
        for s, (af, ab) in by_stride.items():
            for dt in ("f32", "bf16"):
                f, b = (af, ab) if dt == "bf16" else ((None, None) if af is None else (G, G))
                rows.append(Dw(f"{tag}_s{s}_{dt}", dt, N, C, H, W, s, f, b, why))
    return tuple(rows)


DW_CASES = _dw_rows()


def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def make_dw_inputs(c):
    g = _gen("dw", c.name, c.N, c.C, c.H, c.W, c.stride)
    dt = dt_of(c.dt)
    Ho, Wo = out_hw(c.H, c.W, max(c.stride, 1))
    return dict(x=_randn((c.N, c.C, c.H, c.W), dt, g), w=0.5 * torch.randn(c.C, 1, 3, 3, generator=g),
                s=torch.rand(c.C, generator=g) + 0.5, o=0.5 * torch.randn(c.C, generator=g), dy=_randn((c.N, c.C, Ho, Wo), dt, g))


def _dw_all(c, x, w, s, o, dy, dtype):
    """The four results in `dtype` arithmetic with their magnitude sums: (fwd, A), (aff pre-activation, A), (bwd, A)."""
    st, H, W = c.stride, c.H, c.W
    Ho, Wo = out_hw(H, W, st)
    x, w, s, o, dy = (t.to(dtype) for t in (x, w, s, o, dy))
    conv = lambda a, b: F.conv2d(a, b, stride=st, padding=1, groups=c.C)                       # noqa: E731
    opad = (H - (Ho - 1) * st - 1, W - (Wo - 1) * st - 1)
    tconv = lambda a, b: F.conv_transpose2d(a, b, stride=st, padding=1, output_padding=opad, groups=c.C)     # noqa: E731
    y, A = conv(x, w), conv(x.abs(), w.abs())
    sv, ov = s.view(1, -1, 1, 1), o.view(1, -1, 1, 1)
    return (y, A), (sv * y + ov, sv.abs() * A + ov.abs()), (tconv(dy, w), tconv(dy.abs(), w.abs()))


def dw_reference(c, inp):
    """-> dict(fwd, aff0, aff1, bwd) of (ref, bound)."""
    dt = dt_of(c.dt)
    (y, A), (ya, Aa), (dx, Ad) = _dw_all(c, inp["x"], inp["w"], inp["s"], inp["o"], inp["dy"], torch.float64)
    nb = 9 if c.stride == 1 else 4
    yr = ya.clamp_min(0)
    return dict(fwd=(y, _bound(y, 9 * U_ACC * A, dt)), aff0=(ya, _bound(ya, 10 * U_ACC * Aa, dt)),
                aff1=(yr, _bound(yr, 10 * U_ACC * Aa, dt)), bwd=(dx, _bound(dx, nb * U_ACC * Ad, dt)))


def emulate_dw(c, inp, fault=None):
    """The kernels' arithmetic in fp32 (torch's summation order), one rounding to the output type.
    fault: halo_drop (the left halo tap of the vector tile at column 8 is dropped) | right_edge (in[9] of the last tile reads
    the element after the row's end instead of zero) | round_twice (the accumulator is rounded to bf16 before the affine)."""
    dt = dt_of(c.dt)
    x = inp["x"].float()
    (y, _), (ya, _), (dx, _) = _dw_all(c, x, inp["w"], inp["s"], inp["o"], inp["dy"], torch.float32)
    conv = lambda a, pad: F.conv2d(a, inp["w"], stride=c.stride, padding=pad, groups=c.C)     # noqa: E731
    if fault == "halo_drop":
        xz = x.clone()
        xz[..., 7] = 0
        y = y.clone()
        y[..., 8] = conv(xz, 1)[..., 8]
    if fault == "right_edge":
        nxt = x.flatten().roll(-1).view_as(x)[..., -1:]
        y = conv(torch.cat([x, nxt], -1), 1)[..., :c.W].contiguous()
    if fault == "round_twice":
        ya = inp["s"].view(1, -1, 1, 1) * y.to(dt).float() + inp["o"].view(1, -1, 1, 1)
    return dict(fwd=y.to(dt), aff0=ya.to(dt), aff1=ya.clamp_min(0).to(dt), bwd=dx.to(dt))


# =============================================================================================
# 3x3 filter gradient
# =============================================================================================
Wg = collections.namedtuple("Wg", "name dt N C H W stride ints claims")
# ints: integer-valued inputs, every partial sum exact in fp32: bound 0;  claims: parts, rows_per_part, and what the row is for


def wgrad_plan(N, H, W, stride):
    """wgrad_rows_per_part / wgrad_parts of csrc/dwconv3x3.hip restated -> dict(rows, rows_per_part, parts, want)."""
    Ho, Wo = out_hw(H, W, stride)
    rows = N * Ho
    want = (rows * Wo + 8191) // 8192
    parts = max(1, min(want, 64, rows))
    rpp = (rows + parts - 1) // parts
    return dict(rows=rows, rows_per_part=rpp, parts=(rows + rpp - 1) // rpp, want=want)


def wgrad_workspace_bytes(N, C, H, W, stride):
    if not (N > 0 and C > 0 and H > 0 and W > 0 and stride in (1, 2) and C <= 65535 * 32):
        return ERR_UNSUPPORTED
    return C * wgrad_plan(N, H, W, stride)["parts"] * 9 * 4


def _wg_rows():
    spec = (
        # (tag, N, C, H, W, strides, dtypes, claims)
        ("one_part", 1, 3, 5, 7, (1, 2), ("f32", "bf16"), dict(parts=1)),
        ("rows_lt4", 1, 2, 2, 9, (1, 2), ("f32", "bf16"), dict(parts=1, idle_waves=True)),
        ("ragged_wide", 2, 2, 50, 200, (1,), ("f32", "bf16"), dict(parts=3, ragged=True, lane_loop=True)),
        ("ragged_wide", 2, 2, 100, 400, (2,), ("f32", "bf16"), dict(parts=3, ragged=True, lane_loop=True)),
        ("clamp", 1, 2, 2, 20000, (1,), ("f32", "bf16"), dict(parts=2, clamp=True, lane_loop=True)),
        ("clamp", 1, 2, 3, 40000, (2,), ("f32", "bf16"), dict(parts=2, clamp=True, lane_loop=True)),
        ("cap64", 1, 1, 768, 704, (1,), ("bf16",), dict(parts=64, cap=True)),
        ("cap64", 1, 1, 1450, 1460, (2,), ("f32",), dict(parts=61, cap=True)),
    )
    rows = []
    for tag, N, C, H, W, strides, dts, claims in spec:
        for s in strides:
            for dt in dts:
                rows.append(Wg(f"{tag}_s{s}_{dt}", dt, N, C, H, W, s, False, claims))
    rows.append(Wg("ints_ragged_s1_bf16", "bf16", 2, 2, 50, 200, 1, True, dict(parts=3, ragged=True)))
    rows.append(Wg("ints_cap64_s1_f32", "f32", 1, 1, 768, 704, 1, True, dict(parts=64, cap=True)))
    rows.append(Wg("ints_clamp_s2_bf16", "bf16", 1, 2, 3, 40000, 2, True, dict(parts=2, clamp=True)))
    return tuple(rows)


WG_CASES = _wg_rows()
WG_UNSUPPORTED = ((1, 2, 5, 7, 3), (0, 2, 5, 7, 1))          # (N, C, H, W, stride) the entry and the workspace query refuse


def make_wg_inputs(c):
    g = _gen("wg", c.name, c.N, c.C, c.H, c.W, c.stride)
    dt = dt_of(c.dt)
    Ho, Wo = out_hw(c.H, c.W, c.stride)
    if c.ints:                                               # |x|, |dy| <= 2: every sum below 4 N Ho Wo < 2^24 is exact in fp32
        return dict(x=torch.randint(-2, 3, (c.N, c.C, c.H, c.W), generator=g).to(dt), dy=torch.randint(-2, 3, (c.N, c.C, Ho, Wo), generator=g).to(dt))
    return dict(x=_randn((c.N, c.C, c.H, c.W), dt, g), dy=_randn((c.N, c.C, Ho, Wo), dt, g))


def _wg_products(c, x, dy):
    """[9] tensors [N, C, Ho, Wo]: dy * x shifted by tap (u, v), zero outside the plane."""
    s = c.stride
    Ho, Wo = out_hw(c.H, c.W, s)
    xp = F.pad(x, (1, 1, 1, 1))
    return [dy * xp[:, :, u:u + s * (Ho - 1) + 1:s, v:v + s * (Wo - 1) + 1:s] for u in range(3) for v in range(3)]


def wg_reference(c, inp):
    """-> dict(dw=(ref [C,1,3,3], bound)).  The workspace is held to the same (summed over its parts in double)."""
    pr = _wg_products(c, inp["x"].double(), inp["dy"].double())
    ref = torch.stack([p.sum((0, 2, 3)) for p in pr], 1).view(c.C, 1, 3, 3)
    A = torch.stack([p.abs().sum((0, 2, 3)) for p in pr], 1).view(c.C, 1, 3, 3)
    Ho, Wo = out_hw(c.H, c.W, c.stride)
    return dict(dw=(ref, torch.zeros_like(ref) if c.ints else c.N * Ho * Wo * U_ACC * A))


def emulate_wg(c, inp, fault=None):
    """One fp32 sum per part, the parts added in index order -> dict(dw [C,1,3,3], ws [C, parts, 9]) fp32.
    fault: drop_last_part."""
    p = wgrad_plan(c.N, c.H, c.W, c.stride)
    pr = _wg_products(c, inp["x"].float(), inp["dy"].float())
    Ho, _ = out_hw(c.H, c.W, c.stride)
    rows = torch.stack([t.permute(1, 0, 2, 3).reshape(c.C, c.N * Ho, -1).sum(2) for t in pr], 2)          # [C, rows, 9]
    rpp, parts = p["rows_per_part"], p["parts"]
    ws = torch.stack([rows[:, k * rpp:(k + 1) * rpp].sum(1) for k in range(parts)], 1)                    # [C, parts, 9]
    dw = torch.zeros(c.C, 9)
    for k in range(parts - (1 if fault == "drop_last_part" else 0)):
        dw = dw + ws[:, k]
    return dict(dw=dw.view(c.C, 1, 3, 3), ws=ws)


# =============================================================================================
# reflect pad 1, channels_last and NCHW
# =============================================================================================
Pd = collections.namedtuple("Pd", "name layout dt B C H W bwd kind why")
# layout "nhwc": storage [B, H, W, C];  "nchw": [B, C, H, W].  kind "randn" | "bits" (arbitrary bit patterns, forward only)
_PAD_SIZES = ((2, 2), (2, 7), (7, 2), (3, 3), (3, 4), (4, 3), (4, 4), (3, 7), (7, 4), (7, 7))


def _pd_rows():
    rows = []
    for i, (H, W) in enumerate(_PAD_SIZES):
        for dt in ("f32", "bf16"):
            Cn = (8, 24, 64)[(i + (dt == "bf16")) % 3]
            for layout, B, C in (("nhwc", 2, Cn), ("nchw", 2, 3)):
                rows.append(Pd(f"{layout}_fwd_{H}x{W}_c{C}_{dt}", layout, dt, B, C, H, W, False, "randn", "mirror rows and columns"))
                if H >= 3 and W >= 3:
                    rows.append(Pd(f"{layout}_bwd_{H}x{W}_c{C}_{dt}", layout, dt, B, C, H, W, True, "randn",
                                   "both border copies on one line" if 3 in (H, W) else "one border copy per line"))
    for dt in ("f32", "bf16"):
        rows.append(Pd(f"nhwc_fwd_bits_{dt}", "nhwc", dt, 2, 24, 5, 6, False, "bits", "NaN payloads, Inf, denormals through the copy"))
        rows.append(Pd(f"nchw_fwd_bits_{dt}", "nchw", dt, 2, 3, 5, 6, False, "bits", "NaN payloads, Inf, denormals through the copy"))
    # above 2,097,152 elements either way: the 8192-block cap and the grid-stride loop of csrc/pad.hip
    rows.append(Pd("nchw_fwd_cap_bf16", "nchw", "bf16", 2, 16, 254, 260, False, "randn", "8192-block cap"))
    rows.append(Pd("nchw_bwd_cap_bf16", "nchw", "bf16", 2, 16, 254, 260, True, "randn", "8192-block cap"))
    rows.append(Pd("nchw_bwd_cap_f32", "nchw", "f32", 2, 16, 254, 260, True, "randn", "8192-block cap"))
    return tuple(rows)


PD_CASES = _pd_rows()
PD_UNSUPPORTED = (("nhwc", True, 2, 8, 2, 5), ("nhwc", True, 2, 8, 5, 2), ("nhwc", False, 2, 8, 1, 5), ("nhwc", False, 2, 12, 4, 4),
                  ("nchw", True, 2, 3, 2, 5), ("nchw", True, 2, 3, 5, 2), ("nchw", False, 2, 3, 1, 5))     # (layout, bwd, B, C, H, W)


def to_storage(t, layout):
    """A logical [B, C, H, W] tensor as the layout's dense storage."""
    return t.permute(0, 2, 3, 1).contiguous() if layout == "nhwc" else t.contiguous()


def to_logical(t, layout):
    return t.permute(0, 3, 1, 2) if layout == "nhwc" else t


def _refl(n, fault=None):
    idx = [abs(i) if i < n else 2 * n - 2 - i for i in range(-1, n + 1)]
    if fault == "mirror_off_by_one":
        idx[0] = 0
    return torch.tensor(idx)


def make_pd_inputs(c):
    g = _gen("pd", c.name, c.B, c.C, c.H, c.W)
    dt = dt_of(c.dt)
    shape = (c.B, c.C, c.H + 2, c.W + 2) if c.bwd else (c.B, c.C, c.H, c.W)
    t = special_bits(shape, dt, g) if c.kind == "bits" else _randn(shape, dt, g)
    return dict(a=to_storage(t, c.layout))


def _pad_adjoint(d, c, skip_second_border=False):
    iy, ix = _refl(c.H).to(d.device), _refl(c.W).to(d.device)
    if skip_second_border:
        d = d.clone()
        d[:, :, c.H + 1] = 0
    t = torch.zeros(c.B, c.C, c.H, c.W + 2, dtype=d.dtype, device=d.device).index_add_(2, iy, d)
    return torch.zeros(c.B, c.C, c.H, c.W, dtype=d.dtype, device=d.device).index_add_(3, ix, t)


def pd_reference(c, inp):
    """-> dict(out=(ref in storage layout, bound));  forward: bound None (bit equality)."""
    a = to_logical(inp["a"], c.layout)
    if not c.bwd:
        iy, ix = _refl(c.H).to(a.device), _refl(c.W).to(a.device)
        return dict(out=(to_storage(a[:, :, iy][:, :, :, ix], c.layout), None))
    d = a.double()
    ref, A = _pad_adjoint(d, c), _pad_adjoint(d.abs(), c)
    return dict(out=(to_storage(ref, c.layout), to_storage(_bound(ref, 9 * U_ACC * A, dt_of(c.dt)), c.layout)))


def emulate_pd(c, inp, fault=None):
    """fault: mirror_off_by_one (padded row -1 reads row 0) | skip_second_border (H = 3: the copy from padded row H + 1 omitted)."""
    a = to_logical(inp["a"], c.layout)
    if not c.bwd:
        iy, ix = _refl(c.H, fault), _refl(c.W)
        return dict(out=to_storage(a[:, :, iy][:, :, :, ix], c.layout))
    return dict(out=to_storage(_pad_adjoint(a.float(), c, fault == "skip_second_border").to(dt_of(c.dt)), c.layout))


# =============================================================================================
# bias + ELU, channels_last ([P, C]) and NCHW ([N, C, HW])
# =============================================================================================
Be = collections.namedtuple("Be", "name layout dt bdt N C HW claims")
# nhwc: P = N * HW pixels, the raw entry takes (P, C);  claims: slabs / chunks and what the row is for


def nhwc_c_ok(C):
    return C >= 8 and C % 8 == 0 and C // 8 <= 256 and 256 % (C // 8) == 0


def slab_plan(P, C):
    """plan_slabs of csrc/nhwc_decoder.hip restated -> dict(RL, want, rows, slabs) or None (refused)."""
    if P <= 0 or not nhwc_c_ok(C):
        return None
    RL = 256 // (C // 8)
    want = (P + RL * 8 - 1) // (RL * 8)
    slabs = max(1, min(want, 1024))
    rows = (P + slabs - 1) // slabs
    return dict(RL=RL, want=want, rows=rows, slabs=(P + rows - 1) // rows)


def chunk_plan(planes, HW):
    """plan of csrc/bias_act.hip restated -> dict(chunks, per)."""
    chunks = 1
    while planes * chunks < 2048 and HW // (chunks * 2) >= 2048:
        chunks *= 2
    return dict(chunks=chunks, per=((HW + chunks - 1) // chunks + 7) // 8 * 8)


def _be_rows():
    rows = []
    nhwc = (
        # (tag, P, C, dtypes, claims)
        ("c8_idle", 20, 8, ("f32", "bf16"), dict(RL=256, slabs=1, idle_lanes=True)),
        ("c64_one_slab", 256, 64, ("f32", "bf16"), dict(RL=32, slabs=1)),
        ("c64_ragged", 601, 64, ("f32", "bf16"), dict(RL=32, slabs=3, ragged=True)),
        ("c8_ragged", 5000, 8, ("f32", "bf16"), dict(RL=256, slabs=3, ragged=True)),
        ("c1024_idle", 1, 1024, ("f32", "bf16"), dict(RL=2, slabs=1, idle_lanes=True)),
        ("c1024_ragged", 37, 1024, ("f32", "bf16"), dict(RL=2, slabs=3, ragged=True)),
        ("c2048", 20, 2048, ("f32", "bf16"), dict(RL=1, slabs=3, ragged=True)),
        ("c2048_cap", 8200, 2048, ("bf16",), dict(RL=1, slabs=912, cap=True, ragged=True)),
    )
    for i, (tag, P, C, dts, claims) in enumerate(nhwc):
        for dt in dts:
            rows.append(Be(f"nhwc_{tag}_{dt}", "nhwc", dt, ("f32", "bf16")[(i + (dt == "bf16")) % 2], 1, C, P, claims))
    nchw = (
        # (tag, N, C, HW, claims)
        ("hw64", 2, 3, 64, dict(chunks=1, vector=True)),
        ("hw63", 2, 3, 63, dict(chunks=1, vector=False)),
        ("hw5", 3, 2, 5, dict(chunks=1, vector=False)),
        ("hw4104_ragged", 1, 1, 4104, dict(chunks=2, vector=True, ragged=True)),
        ("hw8200_ragged", 1, 2, 8200, dict(chunks=4, vector=True, ragged=True)),
        ("hw67x63", 1, 1, 67 * 63, dict(chunks=2, vector=False, ragged=True)),
        ("planes2048_hw1", 2, 1024, 1, dict(chunks=1, vector=False)),
    )
    for i, (tag, N, C, HW, claims) in enumerate(nchw):
        for dt in ("f32", "bf16"):
            rows.append(Be(f"nchw_{tag}_{dt}", "nchw", dt, ("f32", "bf16")[(i + (dt == "f32")) % 2], N, C, HW, claims))
    return tuple(rows)


BE_CASES = _be_rows()
BE_UNSUPPORTED_C = (24, 4104, 4)                             # channels_last channel counts the entries and the slab query refuse


def be_shape(c):
    return (c.N * c.HW, c.C) if c.layout == "nhwc" else (c.N, c.C, c.HW)


def _be_channel(c, flat):
    return flat % c.C if c.layout == "nhwc" else (flat // c.HW) % c.C


def _be_bias_view(c, b):
    return b.view(1, -1) if c.layout == "nhwc" else b.view(1, -1, 1)


def be_plan(c):
    return slab_plan(c.N * c.HW, c.C) if c.layout == "nhwc" else chunk_plan(c.N * c.C, c.HW)


def be_partial_shape(c):
    p = be_plan(c)
    return (p["slabs"], c.C) if c.layout == "nhwc" else (c.N * c.C, p["chunks"])


def make_be_inputs(c):
    """z, bias, dy.  Planted in z (where the row has the elements): u = z + b exactly 0 and u = -100 (y == -1, y + 1 == 0)."""
    g = _gen("be", c.name, c.N, c.C, c.HW)
    dt, shape = dt_of(c.dt), be_shape(c)
    z = _randn(shape, dt, g)
    b = (0.5 * torch.randn(c.C, generator=g)).bfloat16()
    n = z.numel()
    zf = z.view(-1)
    for k, flat in enumerate((n // 3, n // 2 + 1, n - 1, 0)):
        ch = _be_channel(c, flat)
        zf[flat] = (-b[ch].float()).to(dt) if k % 2 == 0 else torch.tensor(-100.0).to(dt) - b[ch].float().to(dt)
    return dict(z=z, bias=b.float() if c.bdt == "f32" else b, dy=_randn(shape, dt, g))


def plant_y(y):
    """The backward's y input: the stored forward output with +0.0, -0.0 and -1 planted (the derivative is read from it)."""
    y = y.clone()
    yf = y.view(-1)
    for k, v in enumerate((0.0, -0.0, -1.0)):
        if yf.numel() > 2 * k + 1:
            yf[2 * k + 1] = v
    return y


def elu64(u):
    return torch.where(u > 0, u, torch.expm1(u))


def be_fwd_reference(c, inp):
    u = inp["z"].double() + _be_bias_view(c, inp["bias"].double())
    ref = elu64(u)
    term = U_F32 * u.abs() * torch.exp(u.clamp_max(0)) + (u <= 0).double() * E_ELU
    return dict(y=(ref, _bound(ref, term, dt_of(c.dt))))


def be_bwd_reference(c, inp, y_in):
    """-> dict(dz, db): db [C] against the double sum of the partials (be_partial_sum)."""
    y, dy = y_in.double(), inp["dy"].double()
    dz = dy * torch.where(y > 0, 1.0, y + 1.0)
    dims = (0,) if c.layout == "nhwc" else (0, 2)
    n = c.N * c.HW
    return dict(dz=(dz, _bound(dz, U_ACC * dz.abs(), dt_of(c.dt))), db=(dz.sum(dims), n * U_ACC * dz.abs().sum(dims)))


def be_partial_sum(c, partial):
    return partial.double().sum(0) if c.layout == "nhwc" else partial.double().view(c.N, c.C, -1).sum((0, 2))


def emulate_be_fwd(c, inp, fault=None):
    """fault: tail_unwritten (NCHW: the HW % 8 tail of every plane is never stored)."""
    u = inp["z"].float() + _be_bias_view(c, inp["bias"].float())
    y = torch.where(u > 0, u, torch.expm1(u)).to(dt_of(c.dt))
    if fault == "tail_unwritten":
        y[..., c.HW - c.HW % 8:] = float("nan")
    return dict(y=y)


def emulate_be_bwd(c, inp, y_in, fault=None):
    """-> dict(dz, partial): the fp32 products summed per slab / chunk before dz is rounded.  fault: drop_last (the last slab /
    the last chunk of every plane adds nothing)."""
    y = y_in.float()
    o = inp["dy"].float() * torch.where(y > 0, torch.ones_like(y), y + 1.0)
    p = be_plan(c)
    if c.layout == "nhwc":
        part = torch.stack([o[k * p["rows"]:(k + 1) * p["rows"]].sum(0) for k in range(p["slabs"])])
        if fault == "drop_last":
            part[-1] = 0
    else:
        part = torch.stack([o[..., k * p["per"]:(k + 1) * p["per"]].sum(-1) for k in range(p["chunks"])], -1).reshape(c.N * c.C, -1)
        if fault == "drop_last":
            part[:, -1] = 0
    return dict(dz=o.to(dt_of(c.dt)), partial=part.contiguous())


def measure_e_elu(grid=2_000_001):
    """Worst |expm1_f32 - expm1_f64| over every negative finite bf16 value and dense fp32 grids on [-ELU_RANGE, 0)."""
    allb = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(BF16).float()
    pts = [allb[(allb < 0) & torch.isfinite(allb)], torch.linspace(-ELU_RANGE, 0, grid, dtype=torch.float64).float(),
           -torch.logspace(-30, 0, grid, base=2, dtype=torch.float64).float()]
    return max(float((torch.expm1(u).double() - torch.expm1(u.double())).abs().max()) for u in (p[p < 0] for p in pts))


# =============================================================================================
# nearest 2x upsampling + concatenation, channels_last
# =============================================================================================
Uc = collections.namedtuple("Uc", "name dt N C1 C2 H W kind why")
# H, W: the OUTPUT size.  storage: a [N, H/2, W/2, C1], b [N, H, W, C2], out / dout [N, H, W, C1 + C2]


def _uc_rows():
    spec = (("c2_0_2x2", 1, 8, 0, 2, 2, "no skip tensor, one source pixel"), ("c8_8_2x2", 1, 8, 8, 2, 2, "H = W = 2"),
            ("c8_8_4x4", 2, 8, 8, 4, 4, "N = 2"), ("c24_40_6x10", 2, 24, 40, 6, 10, "C / 8 = 3 and 5, a 3 x 5 source, four blocks"),
            ("c16_0_6x4", 3, 16, 0, 6, 4, "no skip tensor, odd source height"))
    rows = [Uc(f"{tag}_{dt}", dt, N, C1, C2, H, W, "randn", why) for tag, N, C1, C2, H, W, why in spec for dt in ("f32", "bf16")]
    rows += [Uc(f"bits_{dt}", dt, 2, 24, 40, 6, 10, "bits", "NaN payloads, Inf, denormals through the copies") for dt in ("f32", "bf16")]
    return tuple(rows)


UC_CASES = _uc_rows()
UC_UNSUPPORTED = ((1, 8, 8, 3, 4), (1, 8, 8, 4, 6 + 1), (1, 12, 8, 4, 4), (1, 8, 4, 4, 4), (1, 0, 8, 4, 4))      # (N, C1, C2, H, W)


def make_uc_inputs(c):
    g = _gen("uc", c.name, c.N, c.C1, c.C2, c.H, c.W)
    dt = dt_of(c.dt)
    mk = (lambda s: special_bits(s, dt, g)) if c.kind == "bits" else (lambda s: _randn(s, dt, g))
    return dict(a=mk((c.N, c.H // 2, c.W // 2, c.C1)), b=mk((c.N, c.H, c.W, c.C2)) if c.C2 else None, dout=mk((c.N, c.H, c.W, c.C1 + c.C2)))


def _up2(a):
    return a.repeat_interleave(2, 1).repeat_interleave(2, 2)


def _block_sum(d, c):
    return d.view(c.N, c.H // 2, 2, c.W // 2, 2, c.C1).sum((2, 4))


def uc_reference(c, inp):
    """-> dict(out, da, db); out and db bit-exact.  A `bits` row holds no da (sums of arbitrary patterns)."""
    up = _up2(inp["a"])
    out = dict(out=(torch.cat([up, inp["b"]], -1) if c.C2 else up, None))
    if c.kind != "bits":
        d = inp["dout"][..., :c.C1].double()
        da = _block_sum(d, c)
        out["da"] = (da, _bound(da, 4 * U_ACC * _block_sum(d.abs(), c), dt_of(c.dt)))
    if c.C2:
        out["db"] = (inp["dout"][..., c.C1:].contiguous(), None)
    return out


def emulate_uc(c, inp, fault=None):
    """fault: round_twice (da: the first row pair is rounded to the output type before the second is added)."""
    up = _up2(inp["a"])
    out = dict(out=torch.cat([up, inp["b"]], -1) if c.C2 else up)
    dt = dt_of(c.dt)
    if c.kind != "bits":
        d = inp["dout"][..., :c.C1].float().view(c.N, c.H // 2, 2, c.W // 2, 2, c.C1)
        top, bot = d[:, :, 0].sum(3), d[:, :, 1].sum(3)
        out["da"] = ((top.to(dt).float() if fault == "round_twice" else top) + bot).to(dt)
    if c.C2:
        out["db"] = inp["dout"][..., c.C1:].contiguous()
    return out


# =============================================================================================
# MaxPool2d(3, 2, 1), channels_last
# =============================================================================================
Mp = collections.namedtuple("Mp", "name dt N C H W kind why")
# storage x / dx [N, H, W, C], y / idx / dy [N, Ho, Wo, C].  kind "relu" (ties at exact zeros) | "nan"


def _mp_rows():
    rows = []
    for i, (H, W) in enumerate(((1, 1), (2, 2), (13, 19), (24, 40))):
        for C in (8, 24):
            for dt in ("f32", "bf16"):
                rows.append(Mp(f"{H}x{W}_c{C}_{dt}", dt, 2, C, H, W, "relu", "post-ReLU ties"))
    rows += [Mp(f"nan_13x19_c8_{dt}", dt, 2, 8, 13, 19, "nan", "NaNs, two in one window") for dt in ("f32", "bf16")]
    return tuple(rows)


MP_CASES = _mp_rows()
MP_UNSUPPORTED = ((2, 12, 4, 4), (2, 4, 4, 4), (0, 8, 4, 4))          # (N, C, H, W)


def make_mp_inputs(c):
    g = _gen("mp", c.name, c.N, c.C, c.H, c.W)
    dt = dt_of(c.dt)
    Ho, Wo = out_hw(c.H, c.W, 2)
    x = torch.randn(c.N, c.H, c.W, c.C, generator=g)
    if c.kind == "relu":
        x = x.clamp_min(0)
        if c.H * c.W >= 4:                                   # coarse values: ties between positive maxima as well
            x = (x * 2).round() / 2
    else:
        x[0, 3, 4, :] = float("nan")                         # two in the window of output (2, 2): rows 3-5, columns 3-5
        x[0, 4, 5, ::2] = float("nan")
        x[1, 0, 0, 1] = float("nan")                         # a corner window
        x[1, c.H - 1, c.W - 1, :] = float("nan")
        x[0, 8, 9, 3] = float("-inf")
    return dict(x=x.to(dt), dy=_randn((c.N, Ho, Wo, c.C), dt, g))


def mp_index(x, rule="first"):
    """The window index 3 r + s [N, Ho, Wo, C] (uint8) and the in-plane position iy * W + ix of the maximum: the first maximum
    in scan order of the in-bounds window, updated on every NaN.  rule "last": the tie fault."""
    N, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, 2)
    xd = x.double()
    oy, ox = torch.arange(Ho, device=x.device), torch.arange(Wo, device=x.device)
    best = torch.zeros(N, Ho, Wo, C, dtype=torch.float64, device=x.device)
    bi = torch.full((N, Ho, Wo, C), 255, dtype=torch.int64, device=x.device)
    pos = torch.zeros_like(bi)
    for r in range(3):
        iy = 2 * oy - 1 + r
        for s in range(3):
            ix = 2 * ox - 1 + s
            valid = ((iy >= 0) & (iy < H)).view(1, Ho, 1, 1) & ((ix >= 0) & (ix < W)).view(1, 1, Wo, 1)
            val = xd[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            better = (val >= best) if rule == "last" else (val > best)
            upd = valid & ((bi == 255) | better | torch.isnan(val))
            best = torch.where(upd, val, best)
            bi = torch.where(upd, torch.full_like(bi, 3 * r + s), bi)
            pos = torch.where(upd, (iy.clamp(0, H - 1).view(1, Ho, 1, 1) * W + ix.clamp(0, W - 1).view(1, 1, Wo, 1)).expand_as(pos), pos)
    return bi.to(torch.uint8), pos


def _mp_gather(x, pos):
    N, H, W, C = x.shape
    return bits(x).view(N, H * W, C).gather(1, pos.view(N, -1, C)).view(x.dtype).view(pos.shape)


def _mp_scatter(dy, pos, H, W):
    N, Ho, Wo, C = dy.shape
    return torch.zeros(N, H * W, C, dtype=dy.dtype, device=dy.device).scatter_add_(1, pos.view(N, -1, C), dy.view(N, -1, C)).view(N, H, W, C)


def mp_reference(c, inp):
    """-> dict(y, idx (bit-exact), dx)."""
    idx, pos = mp_index(inp["x"])
    d = inp["dy"].double()
    dx = _mp_scatter(d, pos, c.H, c.W)
    return dict(y=(_mp_gather(inp["x"], pos), None), idx=(idx, None),
                dx=(dx, _bound(dx, 4 * U_ACC * _mp_scatter(d.abs(), pos, c.H, c.W), dt_of(c.dt))))


def emulate_mp(c, inp, fault=None):
    """fault: last_max (the last maximum of a window wins a tie)."""
    idx, pos = mp_index(inp["x"], "last" if fault == "last_max" else "first")
    return dict(y=_mp_gather(inp["x"], pos), idx=idx, dx=_mp_scatter(inp["dy"].float(), pos, c.H, c.W).to(dt_of(c.dt)))
