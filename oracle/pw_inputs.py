"""TEST INFRASTRUCTURE ONLY -- case tables, seeded inputs, float64 references and per-element error bounds for the pointwise
GEMM family: csrc/pwconv.hip (v1 pwconv_kernel, v2 pwconv2_kernel on the LDS-DMA ring), csrc/pwgrad.hip (pwgrad_kernel,
pwgrad2_kernel<32>, pwgrad2_pair_kernel<32> and the two reduce kernels) and csrc/tapsum.hip.  Pure torch; everything is a
function of its arguments and the seed.  Which kernel a row reaches is NOT restated here: a row names the arm it claims and how
it gets there (`natural`: no switch set; `hook`: under the variables in `env`), and tests/test_pw_arms_cpu.py asks the
library's own plan queries (ops.pwconv_plan / pwgrad_plan / pwgrad_pair_plan, the functions the launches go by) whether it
does.  That file also proves the census, the references, the bounds and that the bounds catch index faults;
tests/test_pw_arms_gpu.py runs every row on the device.

THE BOUND (derived as in oracle/conv_inputs.py, not tuned).  bf16 operands multiply exactly in fp32; n products added in fp32
in any order, rounding or truncating, stay within n * 2^-23 * A of the exact sum, A = sum |a_i b_i|; one round-to-nearest to
bf16 adds 2^-8 of the value:

    bf16 output:  |got - ref| <= 2^-8 |ref| + (1 + 2^-8) * n * 2^-23 * A
    fp32 output:  |got - ref| <=              (1 + 2^-8) * n * 2^-23 * A

    pwconv              n = K (+ 1 with a bias, |bias| joins A)
    EPI 2               Y = acc * GELU'(aux): the accumulation term is scaled by |GELU'(aux)|, n = K + 1 (the fp32 product
                        rounds once more), plus |acc| * D_DGELU for the evaluation of GELU' (below)
    EPI 1, second output  GELU in double of the first output AS THE KERNEL STORED IT (the kernel rounds pre to bf16 and activates
                        the stored value; the first output is held to its own bound, so this chains and does not circle):
                        2^-8 |ref| + G_GELU * |pre|
    EPI 4               per channel, the double sum over all P partials against the double sum (sum of squares) of the stored
                        output: (m + 1) * 2^-23 * sum |y| (sum y^2), m = 128 / WN, the pixels one partial adds up (+ 1: the
                        square rounds); P is the plan's
    EPI 5               the float64 reference and the max-norm bound of tests/test_inference_gpu.py (`infer_reference`,
                        INFER_TOL), shared with that file
    pwgrad              weights and row sums: n = B * HW (the split partials and their sum are B * HW - 1 additions in all)
    tapsum forward      n = 10 (nine taps and the bias); h like the second output of EPI 1
    tapsum backward     pure data movement: bit equality with a gather written in torch (bound 0)

THE ACTIVATION TERM is the one number that cannot be derived from the project: the device evaluates GELU / GELU' in fp32 with
its own `erff` / `__expf`.  Measured on the CPU (torch float32 against float64, the kernels' formulas
0.5 x (1 + erf(x / sqrt 2)) and 0.5 (1 + erf(x / sqrt 2)) + x phi(x)) over EVERY bf16 value of the rows' argument range:
    GELU,  0 < |x| <= 8:  max |err| / |x| = 8.53e-8   ->  G_GELU  = 4 * 8.53e-8 = 3.41e-7  (absolute term G_GELU * |x|)
    GELU', |x| <= 6:      max |err|       = 9.74e-8   ->  D_DGELU = 4 * 9.74e-8 = 3.90e-7  (absolute)
The margin of 4 is for device functions that are not correctly rounded.  The error is absolute in nature (1 + erf cancels for
negative arguments), so against 2^-8 |ref| it is small where the activation is not: G_GELU |x| / (2^-8 |GELU(x)|) < 2e-4 for
x > 0 and < 1e-3 for x > -1; it is NOT small in the negative tail (x = -4: GELU = -1.3e-4, 2^-8 |ref| = 5e-7 against
G_GELU |x| = 1.4e-6; GELU'(-6) = -4e-8 lies below D_DGELU altogether).  There the bound is the absolute term, about 1e-6 on
outputs of order one, and nothing is widened to hide that.  Every element is held to its own bound; none may lie outside.
"""
import collections
import math

import torch
import torch.nn.functional as F

from oracle.conv_inputs import U_ACC, U_BF16, worst  # noqa: F401  (worst: re-exported for the tests)
from oracle.dwconv_inputs import GUARD, GUARD_BITS, guarded, guards_intact  # noqa: F401  (re-exported for the tests)

G_GELU = 4 * 8.53e-8
D_DGELU = 4 * 9.74e-8
GELU_RANGE, DGELU_RANGE = 8.0, 6.0
INFER_TOL = 2.0 ** -7       # max-norm bound of the inference epilogue (tests/test_inference_gpu.py)
BF16, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------------------------------------
# the arm census of pwconv: (version, transposed A, BM, BK, EPI)
# ---------------------------------------------------------------------------------------------
def arm(version, ta, bm, bk, epi):
    return (version, int(ta), bm, bk, epi)


V2_TILES = ((128, 32), (128, 64), (64, 32), (64, 64), (32, 64))
V1_TILES = ((128, 32), (64, 32), (64, 64), (32, 32), (32, 64))
ALL_PW_ARMS = frozenset(
    [arm(2, 0, bm, bk, e) for bm, bk in V2_TILES for e in (0, 1, 2, 4, 5)] + [arm(2, 1, 128, 32, e) for e in (0, 1, 2)]
    + [arm(1, 0, bm, bk, e) for bm, bk in V1_TILES for e in (0, 1, 2, 4)]
    + [arm(1, 1, bm, bk, e) for bm, bk in V1_TILES for e in (0, 1, 2)])
assert len(ALL_PW_ARMS) == 63
PWGRAD_KERNELS = frozenset(("pwgrad_kernel", "pwgrad2_kernel<32>", "pwgrad2_pair_kernel<32>", "pwgrad_reduce_ex_kernel",
                            "pwgrad_reduce_ex2_kernel"))


def epis_of(ta):
    """Epilogues an exported entry point reaches in this A mode on v2 (v1 has no EPI 5)."""
    return (0, 1, 2) if ta else (0, 1, 2, 4, 5)


def arm_of_plan(plan, ta, epi):
    return arm(plan["version"], ta, plan["BM"], plan["BK"], epi)


def arm_of_key(key, ta, epi):
    """The arm of one byte of ops.pwconv_plan_sweep."""
    return arm(2 if key & 1 else 1, ta, (32, 64, 128)[(key >> 1) & 3], 64 if key & 8 else 32, epi)


Pw = collections.namedtuple("Pw", "name B M K HW ta epi bias env arm claims")
# bias: None | "f32" | "bf16";  env: dict of hook variables ({}: natural);  arm: the claimed instantiation, or None where the
# row claims only its family claims["family"] = (version, ta);  claims: further plan properties (steps, total)


def how(c):
    return "hook" if c.env else "natural"


def _pw(name, shape, ta=False, epi=0, bias=None, env=None, tile=None, version=2, **claims):
    B, M, K, HW = shape
    a = arm(version, ta, tile[0], tile[1], epi) if tile is not None else None
    claims.setdefault("family", (version, int(ta)))
    if epi == 4 and bias == "bf16":                          # ppea_pwconv_stats_bf16 takes an fp32 bias
        bias = "f32"
    return Pw(name, B, M, K, HW, bool(ta), epi, bias, dict(env or {}), a, claims)


_BIASES = (None, "f32", "bf16")
# natural shapes, derived from pw_choose (nb = ceil(HW / 128) pixel tiles):
#   v2 128/32: M >= 128 and nb * ceil(M / 128) * B >= 256:  B 8, M 136 (second M tile: 8 rows), HW 1928 (16 tiles, the last 8 pixels)
#   v2 64/32 | 64/64 (K >= 512, K % 64 == 0): 32 < M < 128 and nb * ceil(M / 64) * B >= 256:  B 3, M 72, HW 5384 (43 tiles, 8 pixels)
#   v2 32/64 (K % 64 == 0) | 64/32 (else) below that:  B 1, M 40, HW 200
#   v2 transposed 128/32: M >= 128, M % 8 == 0, nb * ceil(M / 128) * B >= 128:  B 4, M 136, HW 1928
#   v1 transposed (everything else with a transposed matrix) 64/32 | 64/64 (K >= 512): B 3, M 72, HW 5384;  32/32 | 32/64: B 1, M 40,
#     HW 200;  K = 544: the zero-filled half of the last 64-channel step
_NATURAL = {
    (2, 0, 128, 32): (8, 136, 96, 1928), (2, 0, 64, 32): (3, 72, 32, 5384), (2, 0, 64, 64): (3, 72, 512, 5384),
    (2, 0, 32, 64): (1, 40, 64, 200),
    (2, 1, 128, 32): (4, 136, 96, 1928),
    (1, 1, 64, 32): (3, 72, 96, 5384), (1, 1, 64, 64): (3, 72, 544, 5384), (1, 1, 32, 32): (1, 40, 96, 200),
    (1, 1, 32, 64): (1, 40, 544, 200),
}
# hook-only arms on one small ragged shape: M 200 = 128 + 72 = 3 * 64 + 8 = 6 * 32 + 8, HW 264 = 2 * 128 + 8
_SMALL = (2, 200, 128, 264)
_V1_TILE_ENV = {(128, 32): "128", (64, 32): "64", (64, 64): "64d", (32, 32): "32", (32, 64): "32d"}


def _tile_cases():
    rows = []
    for (ver, ta, bm, bk), shape in _NATURAL.items():
        for i, e in enumerate(epis_of(ta) if ver == 2 else (0, 1, 2)):
            rows.append(_pw(f"v{ver}{'t' if ta else ''}_{bm}x{bk}_epi{e}", shape, ta, e, None if e in (2, 5) else _BIASES[(i + bm // 32) % 3],
                            tile=(bm, bk), version=ver))
    # the 64/32 fallback at the bottom of the dispatch (K % 64 != 0, too few tiles for anything else)
    for i, e in enumerate(epis_of(False)):
        rows.append(_pw(f"v2_64x32_low_epi{e}", (1, 40, 96, 200), False, e, None if e in (2, 5) else _BIASES[i % 3], tile=(64, 32)))
    for i, e in enumerate(epis_of(False)):
        rows.append(_pw(f"v2_128x64_epi{e}", _SMALL, False, e, None if e in (2, 5) else _BIASES[i % 3], env={"PPEA_PW_V2": "128,64"},
                        tile=(128, 64)))
    for (bm, bk), tag in _V1_TILE_ENV.items():
        # K = 96 under 64-channel steps: the zero-filled half step on the row-major matrix
        shape = (2, 200, 96, 264)
        for i, e in enumerate((0, 1, 2, 4)):
            rows.append(_pw(f"v1_{bm}x{bk}_epi{e}", shape, False, e, None if e == 2 else _BIASES[(i + bm // 64) % 3],
                            env={"PPEA_PW_V2": "0", "PPEA_PW_TILE": tag}, tile=(bm, bk), version=1))
    for i, e in enumerate((0, 1, 2)):
        rows.append(_pw(f"v1t_128x32_epi{e}", (2, 200, 96, 264), True, e, None if e == 2 else _BIASES[i], env={"PPEA_PW_TILE": "128"},
                        tile=(128, 32), version=1))
    return tuple(rows)


TILE_CASES = _tile_cases()


def _edge_cases():
    rows = []
    v1 = {"PPEA_PW_V2": "0"}

    def both(name, shape, epi=0, bias=None, **claims):                     # row-major, v2 natural and v1 by the hook
        rows.append(_pw(f"v2_{name}", shape, False, epi, bias, **claims))
        c1 = {k: v for k, v in claims.items() if k != "total"}
        rows.append(_pw(f"v1_{name}", shape, False, epi, bias, env=v1, version=1, **c1))

    # M: one row, less than a 16-row fragment, no multiple of 16, a last tile of one row; HW: 8, 136, % 128 in {8, 64, 120};
    # B 1 and >= 3; tile totals 1, 7, 9 (the XCD remap); every bias form; EPI 4 on a ragged M and a plane tail (HW 136: the
    # pixel-waves 1.. of the second tile lie wholly outside the plane)
    both("m1_hw8", (1, 1, 32, 8), 0, "f32", total=1)
    both("m5_hw136", (1, 5, 64, 136), 4, "bf16", total=2)
    both("m20_hw72_b3", (3, 20, 96, 72), 1, "bf16")
    both("m33_hw192", (2, 33, 128, 192), 4, None)                          # 32-row tiles: the second holds one row
    both("m129_hw248", (1, 129, 64, 248), 0, "bf16")
    both("total7", (7, 24, 64, 120), 2, None, total=7)
    both("total9", (3, 8, 96, 264), 0, None, total=9)
    both("dgelu_tails", (3, 40, 64, 136), 2, None)
    both("gelu_m65", (2, 65, 96, 200), 1, "f32")                           # 64-row tiles: the second holds one row
    rows.append(_pw("v2_total75", (5, 136, 64, 264), False, 4, "f32", env={"PPEA_PW_V2": "32,64"}, tile=(32, 64), total=75))
    rows.append(_pw("v2_128_m129", (1, 129, 32, 136), False, 1, "f32", env={"PPEA_PW_V2": "128,32"}, tile=(128, 32), total=4))
    # K of exactly 1, 2, 3, 4 steps: the ring's prologue and drain differ for each
    for s in (1, 2, 3, 4):
        rows.append(_pw(f"v2_32step_x{s}", (2, 72, 32 * s, 136), False, 0, _BIASES[s % 3], env={"PPEA_PW_V2": "64,32"}, tile=(64, 32), steps=s))
        rows.append(_pw(f"v2_64step_x{s}", (2, 72, 64 * s, 136), False, 1, _BIASES[s % 3], env={"PPEA_PW_V2": "32,64"}, tile=(32, 64), steps=s))
        rows.append(_pw(f"v1_32step_x{s}", (2, 72, 32 * s, 136), False, 0, _BIASES[s % 3], env=dict(v1, PPEA_PW_TILE="32"), tile=(32, 32),
                        version=1, steps=s))
        rows.append(_pw(f"v2t_32step_x{s}", (64, 136, 32 * s, 8), True, (0, 1, 2, 0)[s - 1], (None, "f32", None, "bf16")[s - 1],
                        tile=(128, 32), steps=s))
        rows.append(_pw(f"v1t_32step_x{s}", (2, 24, 32 * s, 136), True, (0, 1, 2, 0)[s - 1], (None, "f32", None, "bf16")[s - 1],
                        tile=(32, 32), version=1, steps=s))
    rows.append(_pw("v1_64step_k96", (2, 72, 96, 136), False, 4, "f32", env=dict(v1, PPEA_PW_TILE="64d"), tile=(64, 64), version=1, steps=2))
    rows.append(_pw("v1_64step_k544", (1, 40, 544, 200), False, 0, "bf16", env=v1, tile=(32, 64), version=1, steps=9))
    rows.append(_pw("v1t_64step_k96", (2, 24, 96, 136), True, 1, "bf16", env={"PPEA_PW_TILE": "32d"}, tile=(32, 64), version=1, steps=2))
    # transposed A: M 8 (v1), no multiple of 16, B 1 and >= 3, HW % 128 in {8, 64, 120}
    rows.append(_pw("v1t_m8_hw8", (1, 8, 32, 8), True, 0, "f32", version=1))
    rows.append(_pw("v1t_m24_hw192", (3, 24, 64, 192), True, 1, "bf16", version=1))
    rows.append(_pw("v1t_m40_hw248_dgelu", (3, 40, 64, 248), True, 2, None, version=1))
    rows.append(_pw("v1t_m72_hw136", (1, 72, 96, 136), True, 0, None, version=1))
    # v2 transposed needs >= 128 tiles of 128 rows: many images of a small plane; 130 tiles: total & 7 = 2
    rows.append(_pw("v2t_hw136", (32, 136, 64, 136), True, 1, "bf16", tile=(128, 32), total=128))
    rows.append(_pw("v2t_total130_dgelu", (65, 136, 64, 8), True, 2, None, tile=(128, 32), total=130))
    rows.append(_pw("v2t_hw192_b1", (1, 136, 32, 128 * 63 + 64), True, 0, "f32", tile=(128, 32), total=128))
    rows.append(_pw("v2t_hw120", (64, 256, 32, 120), True, 0, None, tile=(128, 32), total=128))
    return tuple(rows)


EDGE_CASES = _edge_cases()
# refused by the entry points: nothing may be written
UNSUPPORTED_PW = (_pw("k48", (1, 16, 48, 64)), _pw("hw12", (1, 16, 32, 12)), _pw("ta_m12", (1, 12, 32, 64), True, version=1))
INFER_ACTS = {(128, 32): 0, (128, 64): 1, (64, 32): 2, (64, 64): 0, (32, 64): 2}     # act of the EPI 5 row of each tile


# ---------------------------------------------------------------------------------------------
# pwgrad / tapsum tables
# ---------------------------------------------------------------------------------------------
Pg = collections.namedtuple("Pg", "name B M N H W rowsum env claims")
# claims: step (0 v1 | 32 v2), optionally S, short (last split shorter), cut ("inside" an image | "image" boundary)


def _pg(name, shape, rowsum=True, env=None, **claims):
    B, M, N, H, W = shape
    return Pg(name, B, M, N, H, W, rowsum, dict(env or {}), claims)


_V1G = {"PPEA_PWGRAD_V2": "0"}
PWGRAD_CASES = (
    _pg("v2_s1", (1, 1, 1, 8, 8), step=32, S=1),
    _pg("v2_s2_image_cut", (2, 2, 3, 16, 16), False, step=32, S=2, cut="image"),
    _pg("v2_s2_short_inside", (3, 3, 2, 8, 20), step=32, S=2, short=True, cut="inside"),
    _pg("v2_s16", (4, 34, 130, 32, 32), step=32, S=16),
    _pg("v2_130x34", (2, 130, 34, 8, 32), False, step=32),
    _pg("v2_514x130", (2, 514, 130, 8, 16), step=32),
    _pg("v2_130x514", (2, 130, 514, 8, 16), step=32),
    _pg("v1_hw8", (3, 34, 130, 2, 4), step=0, S=1),
    _pg("v1_hw24", (5, 3, 2, 3, 8), False, step=0),
    _pg("v1_hw40", (2, 1, 1, 5, 8), step=0),
    _pg("v1_hw72_short", (9, 130, 34, 9, 8), step=0, S=5, short=True, cut="image"),
    _pg("v1_hw136_inside", (5, 2, 3, 17, 8), step=0, S=4, short=True, cut="inside"),
    _pg("v1_hook_hw256", (2, 130, 514, 16, 16), env=_V1G, step=0),
    _pg("v1_hook_norowsum", (2, 2, 3, 16, 16), False, env=_V1G, step=0),
)

Pi = collections.namedtuple("Pi", "name B Ch N H W taps wdt bdt bwin env claims")
# taps 1: P [B, Ch, H, W];  taps 9: P [B, 9 Ch, H, W] tap-major, built from g [B, Ch, H, W];  wdt / bdt "f32" | "bf16" (bdt None: no
# bias);  bwin: "all" | "centre" | "one" | "end" -> (b_row0, b_rows)


def _pi(name, shape, taps=1, wdt="f32", bdt=None, bwin="all", env=None, **claims):
    B, Ch, N, H, W = shape
    return Pi(name, B, Ch, N, H, W, taps, wdt, bdt, bwin, dict(env or {}), claims)


def bias_window(c):
    M = c.Ch * c.taps
    return {"all": (0, M), "centre": (4 * c.Ch if c.taps == 9 else M // 2, c.Ch if c.taps == 9 else 1), "one": (min(3, M - 1), 1),
            "end": (M - min(5, M), min(5, M))}[c.bwin]


INTO_CASES = (
    _pi("t1_f32_f32_all", (2, 34, 130, 8, 16), 1, "f32", "f32", "all", step=32),
    _pi("t1_bf16_bf16_one", (2, 130, 34, 8, 16), 1, "bf16", "bf16", "one", step=32),
    _pi("t1_bf16_nobias", (3, 3, 2, 8, 20), 1, "bf16", None, step=32),
    _pi("t1_f32_bf16_end_v1", (3, 34, 130, 3, 8), 1, "f32", "bf16", "end", step=0),
    _pi("t9_f32_f32_centre", (2, 5, 34, 8, 16), 9, "f32", "f32", "centre", step=32),
    _pi("t9_bf16_bf16_centre_2tiles", (2, 32, 130, 8, 8), 9, "bf16", "bf16", "centre", step=32),
    _pi("t9_bf16_nobias_v1", (3, 3, 6, 5, 8), 9, "bf16", None, step=0),
    _pi("t9_f32_f32_all_hook", (2, 1, 3, 4, 8), 9, "f32", "f32", "all", env=_V1G, step=0),
    _pi("t9_f32_bf16_end", (1, 2, 1, 8, 4), 9, "f32", "bf16", "end", step=32),
)
# (name, problem 0, problem 1, env, served by the pair kernel)
PAIR_CASES = (
    ("pair_many_one", INTO_CASES[1]._replace(name="a"), _pi("b", (2, 3, 2, 8, 16), 1, "f32", "f32", "all"), {}, True),
    ("pair_one_many", _pi("a", (2, 3, 2, 8, 16), 1, "bf16", None), _pi("b", (2, 32, 130, 8, 16), 9, "bf16", "bf16", "centre"), {}, True),
    ("pair_adapter", _pi("a", (3, 130, 34, 8, 20), 1, "f32", "f32", "all"), _pi("b", (3, 34, 130, 8, 20), 1, "bf16", "bf16", "all"), {}, True),
    ("pair_hw40_two_launches", _pi("a", (3, 130, 34, 5, 8), 1, "f32", "f32", "all"), _pi("b", (3, 5, 130, 5, 8), 9, "bf16", "f32", "centre"),
     {}, False),
    ("pair_hook_two_launches", _pi("a", (2, 34, 130, 8, 16), 1, "f32", "bf16", "end"), _pi("b", (2, 2, 3, 8, 16), 1, "f32", None), _V1G, False),
)

Ts = collections.namedtuple("Ts", "name B Ch H W bias")
TAPSUM_CASES = tuple(Ts(f"b{B}c{Ch}_{H}x{W}_{b or 'nobias'}", B, Ch, H, W, b)
                     for (B, Ch, H, W) in ((1, 1, 1, 4), (2, 3, 2, 4), (1, 2, 5, 8), (3, 5, 3, 12), (2, 32, 6, 20)) for b in _BIASES)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _gen(*vals):
    s = 31
    for v in vals:
        v = sum(ord(ch) for ch in v) if isinstance(v, str) else int(v)
        s = (s * 1000003 + v) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _bias(n, kind, g):
    if kind is None:
        return None
    b = (0.5 * torch.randn(n, generator=g)).bfloat16()
    return b.float() if kind == "f32" else b


def make_pw_inputs(c):
    """-> dict(x bf16 [B,K,1,HW], a bf16 [M,K] (the matrix; `a_arg` is what the entry point takes: a, or At [K,M] for a
    transposed row), bias None | [M] fp32 / bf16, aux bf16 [B,M,1,HW] with values out to +-6 (EPI 2), and the EPI 5 operands)."""
    g = _gen(c.B, c.M, c.K, c.HW)                            # rows of one shape share x and a (and so the cached products)
    x = torch.randn(c.B, c.K, 1, c.HW, generator=g).bfloat16()
    a = (torch.randn(c.M, c.K, generator=g) / c.K ** 0.5).bfloat16()
    g = _gen(c.name, c.B, c.M, c.K, c.HW, c.epi)
    inp = dict(x=x, a=a, a_arg=a.t().contiguous() if c.ta else a, bias=_bias(c.M, c.bias, g), aux=None, key=(c.B, c.M, c.K, c.HW))
    if c.epi == 2:
        aux = (2.0 * torch.randn(c.B, c.M, 1, c.HW, generator=g)).clamp(-DGELU_RANGE, DGELU_RANGE)
        aux.view(-1)[::7] = torch.tensor([-6.0, 6.0, -5.5, 5.0, -4.0])[torch.arange(aux.view(-1)[::7].numel()) % 5]
        inp["aux"] = aux.bfloat16()
    if c.epi == 5:
        inp.update(s=torch.rand(c.M, generator=g) + 0.5, o=0.3 * torch.randn(c.M, generator=g), s2=torch.rand(c.M, generator=g) + 0.5,
                   o2=0.3 * torch.randn(c.M, generator=g), r1=torch.randn(c.B, c.M, 1, c.HW, generator=g).bfloat16(),
                   r2=torch.randn(c.B, c.M, 1, c.HW, generator=g).bfloat16(), r2_scale=0.75, act=INFER_ACTS.get(c.arm[2:4], 0))
    return inp


def shift_taps(g):
    """The adjoint of the tap sum written as a gather: dT[b][t * Ch + m][y][x] = g[b][m][y - dy][x - dx], t = 3 (dy + 1) + (dx + 1),
    zero outside the plane.  Exact in any dtype."""
    B, Ch, H, W = g.shape
    gp = F.pad(g, (1, 1, 1, 1))
    return torch.cat([gp[:, :, 1 - dy:1 - dy + H, 1 - dx:1 - dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 1).contiguous()


def make_into_inputs(c):
    """-> dict(p bf16 [B, taps Ch, H, W], q bf16 [B, N, H, W], g: p's source for taps = 9)."""
    g = _gen(c.name, c.B, c.Ch, c.N, c.H, c.W, c.taps)
    src = torch.randn(c.B, c.Ch, c.H, c.W, generator=g).bfloat16()
    q = torch.randn(c.B, c.N, c.H, c.W, generator=g).bfloat16()
    return dict(p=shift_taps(src) if c.taps == 9 else src, q=q, g=src)


def make_pwgrad_inputs(c):
    g = _gen(c.name, c.B, c.M, c.N, c.H, c.W)
    return dict(p=torch.randn(c.B, c.M, c.H, c.W, generator=g).bfloat16(), q=torch.randn(c.B, c.N, c.H, c.W, generator=g).bfloat16())


def make_tapsum_inputs(c):
    g = _gen(c.name, c.B, c.Ch, c.H, c.W)
    return dict(T=torch.randn(c.B, 9 * c.Ch, c.H, c.W, generator=g).bfloat16(), bias=_bias(c.Ch, c.bias, g),
                g=torch.randn(c.B, c.Ch, c.H, c.W, generator=g).bfloat16())


# ---------------------------------------------------------------------------------------------
# float64 references with bounds: dicts name -> (ref, bound)
# ---------------------------------------------------------------------------------------------
_R2 = 0.70710678118654752440


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x * _R2))


def dgelu64(x):
    return 0.5 * (1 + torch.erf(x * _R2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


_PRODUCTS = collections.OrderedDict()        # (shape, device) -> (acc, A) of the last two shapes: computed once, never changed


def _acc_and_mag(inp):
    key = (inp.get("key"), str(inp["x"].device))
    if key[0] is not None and key in _PRODUCTS:
        return _PRODUCTS[key]
    a, x = inp["a"].double(), inp["x"].double()
    res = torch.einsum("mk,bkhw->bmhw", a, x), torch.einsum("mk,bkhw->bmhw", a.abs(), x.abs())
    if key[0] is not None:
        _PRODUCTS[key] = res
        while len(_PRODUCTS) > 2:
            _PRODUCTS.popitem(last=False)
    return res


def infer_reference(acc, s, o, act, r1, r2, r2_scale, s2=None, o2=None):
    """The float64 reference of ppea_pwconv_infer_bf16 on the double product `acc` [B,M,H,W] (tests/test_inference_gpu.py's):
    t = act(s acc + o), Y = t (+ r1) (+ r2_scale r2), Y2 = s2 Y + o2 -> (Y, Y2 or None); held to INFER_TOL of the maximum."""
    v = lambda t: t.double().view(1, -1, 1, 1)               # noqa: E731
    t = acc if s is None else v(s) * acc + v(o)
    t = torch.relu(t) if act == 1 else (F.gelu(t) if act == 2 else t)
    ref = t + (r1.double() if r1 is not None else 0) + (r2_scale * r2.double() if r2 is not None else 0)
    return ref, (None if s2 is None else v(s2) * ref + v(o2))


def pw_reference(c, inp, y_stored=None):
    """-> dict of name -> (ref, bound): y for every epilogue but 5; y2 (EPI 1) from `y_stored`, the first output as the kernel
    under test stored it.  Runs on the device its inputs are on."""
    acc, A = _acc_and_mag(inp)
    n = c.K
    if c.epi == 2:
        d = dgelu64(inp["aux"].double())
        ref = acc * d
        return dict(y=(ref, U_BF16 * ref.abs() + (1 + U_BF16) * (n + 1) * U_ACC * A * d.abs() + D_DGELU * acc.abs()))
    if inp["bias"] is not None:
        b = inp["bias"].double().view(1, -1, 1, 1)
        acc, A, n = acc + b, A + b.abs(), n + 1
    out = dict(y=(acc, U_BF16 * acc.abs() + (1 + U_BF16) * n * U_ACC * A))
    if c.epi == 1 and y_stored is not None:
        pre = y_stored.double()
        r2 = gelu64(pre)
        out["y2"] = (r2, U_BF16 * r2.abs() + G_GELU * pre.abs())
    return out


def stats_check(y_stored, sums, WN):
    """EPI 4: per channel, the double sum over the partials [M][P][2] against the double sum / sum of squares of the stored
    output -> (worst ratio of the sum, of the squares, entries outside)."""
    y = y_stored.double()
    m = 128 // WN + 1
    s, q = sums[:, :, 0].double().sum(1), sums[:, :, 1].double().sum(1)
    ws_, wq = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
    r1, o1 = worst(s, ws_, m * U_ACC * y.abs().sum((0, 2, 3)))
    r2, o2 = worst(q, wq, m * U_ACC * wq)
    return r1, r2, o1 + o2 + int((~torch.isfinite(sums)).sum())


def pwgrad_reference(p, q):
    """C[m][n] = sum_{b, pixels} p q and the row sums of p, float64, fp32-output bounds -> dict(w, rowsum)."""
    B, M, H, W = p.shape
    pd, qd = p.double().flatten(2), q.double().flatten(2)
    n = B * H * W
    k = (1 + U_BF16) * n * U_ACC
    return dict(w=(torch.einsum("bmp,bnp->mn", pd, qd), k * torch.einsum("bmp,bnp->mn", pd.abs(), qd.abs())),
                rowsum=(pd.sum((0, 2)), k * pd.abs().sum((0, 2))))


def into_reference(c, inp):
    """The parameter-layout outputs of ppea_pwgrad_ex_bf16: dw [taps Ch, N] or, taps = 9, the weight gradient of
    F.conv2d(x, w, padding=1) in double ([Ch, N, 3, 3]; the tap-major operand is not involved); db = the row sums of the bias
    window.  -> dict(dw, db (with a bias))."""
    ref = pwgrad_reference(inp["p"], inp["q"])
    w, wb = ref["w"]
    if c.taps == 9:
        x = inp["q"].double()
        wz = torch.zeros(c.Ch, c.N, 3, 3, dtype=torch.float64, device=x.device, requires_grad=True)
        (F.conv2d(x, wz, padding=1) * inp["g"].double()).sum().backward()
        re_indexed = w.view(9, c.Ch, c.N).permute(1, 2, 0).reshape(c.Ch, c.N, 3, 3)          # the plain [M][N] result re-indexed
        assert float((wz.grad - re_indexed).abs().max()) <= 1e-9 * max(float(re_indexed.abs().max()), 1.0)
        w, wb = wz.grad, wb.view(9, c.Ch, c.N).permute(1, 2, 0).reshape(c.Ch, c.N, 3, 3)
    out = dict(dw=(w, wb + (U_BF16 * w.abs() if c.wdt == "bf16" else 0.0)))
    if c.bdt is not None:
        r0, rn = bias_window(c)
        b, bb = ref["rowsum"][0][r0:r0 + rn], ref["rowsum"][1][r0:r0 + rn]
        out["db"] = (b, bb + (U_BF16 * b.abs() if c.bdt == "bf16" else 0.0))
    return out


def tapsum_reference(c, inp, pre_stored=None):
    """-> dict(pre, h (from `pre_stored`), dT (bound 0: bit equality))."""
    T = inp["T"].double().view(c.B, 9, c.Ch, c.H, c.W)
    Tp, Ta = F.pad(T, (1, 1, 1, 1)), F.pad(T.abs(), (1, 1, 1, 1))
    pre = torch.zeros(c.B, c.Ch, c.H, c.W, dtype=torch.float64, device=T.device)
    A = torch.zeros_like(pre)
    for t, (dy, dx) in enumerate((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)):
        pre += Tp[:, t, :, 1 + dy:1 + dy + c.H, 1 + dx:1 + dx + c.W]
        A += Ta[:, t, :, 1 + dy:1 + dy + c.H, 1 + dx:1 + dx + c.W]
    if inp["bias"] is not None:
        b = inp["bias"].double().view(1, -1, 1, 1)
        pre, A = pre + b, A + b.abs()
    out = dict(pre=(pre, U_BF16 * pre.abs() + (1 + U_BF16) * 10 * U_ACC * A))
    if pre_stored is not None:
        ps = pre_stored.double()
        h = gelu64(ps)
        out["h"] = (h, U_BF16 * h.abs() + G_GELU * ps.abs())
    dT = shift_taps(inp["g"]).double()
    out["dT"] = (dT, torch.zeros_like(dT))
    return out


# ---------------------------------------------------------------------------------------------
# a correct kernel emulated in torch (fp32 matmul of the bf16 operands, one rounding to the output type, the kernels' rounding
# points) and its index faults: what tests/test_pw_arms_cpu.py holds the references and bounds against
# ---------------------------------------------------------------------------------------------
def _gelu32(x):
    return 0.5 * x * (1 + torch.erf(x * 0.70710678118654752))


def _dgelu32(x):
    return 0.5 * (1 + torch.erf(x * 0.70710678118654752)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


def emulate_pw(c, inp, WN=2, fault=None):
    """-> dict(y [, y2, sums [M][P][2]]).  fault: drop_kstep | swap_chunk | row_above | drop_bias."""
    a, x = inp["a"].float().clone(), inp["x"].float()
    if fault == "drop_kstep":
        a[:, 32 * ((c.K // 32) // 2):][:, :32] = 0
    acc = torch.einsum("mk,bkhw->bmhw", a, x)
    if c.epi == 2:
        y = (acc * _dgelu32(inp["aux"].float())).bfloat16()
    else:
        if inp["bias"] is not None:
            b = inp["bias"].float().clone()
            if fault == "drop_bias":
                b[c.M // 2] = 0
            acc = acc + b.view(1, -1, 1, 1)
        y = acc.bfloat16()
    if fault == "swap_chunk":
        y = y.clone()
        y[-1, -1, 0, :16] = torch.cat([y[-1, -1, 0, 8:16], y[-1, -1, 0, :8]])
    if fault == "row_above":
        y = y.clone()
        y[:, 16] = y[:, 0]
    out = dict(y=y)
    if c.epi == 1:
        out["y2"] = _gelu32(y.float()).bfloat16()
    if c.epi == 4:
        nb = (c.HW + 127) // 128
        yp = F.pad(y.float(), (0, nb * 128 - c.HW)).view(c.B, c.M, nb * WN, 128 // WN)
        out["sums"] = torch.stack([yp.sum(3), (yp * yp).sum(3)], -1).permute(1, 0, 2, 3).reshape(c.M, c.B * nb * WN, 2).contiguous()
    return out


def emulate_pwgrad(p, q, plan, fault=None):
    """The split of `plan` (ops.pwgrad_plan): one fp32 partial per split, summed in fp32 -> (w [M,N], rowsum [M]) fp32.
    fault: drop_split."""
    B, M, H, W = p.shape
    tk = plan["step"] or 64
    spi, sps, S = plan["steps_per_image"], plan["steps_per_split"], plan["S"]
    pf = F.pad(p.float().flatten(2), (0, spi * tk - H * W)).view(B, M, spi, tk).permute(0, 2, 1, 3).reshape(B * spi, M, tk)
    qf = F.pad(q.float().flatten(2), (0, spi * tk - H * W)).view(B, -1, spi, tk).permute(0, 2, 1, 3).reshape(B * spi, -1, tk)
    w = torch.zeros(M, qf.shape[1])
    r = torch.zeros(M)
    for s in range(S):
        if fault == "drop_split" and s == S - 1:
            continue
        sl = slice(s * sps, min((s + 1) * sps, B * spi))
        w = w + torch.einsum("smk,snk->mn", pf[sl], qf[sl])
        r = r + pf[sl].sum((0, 2))
    return w, r


def emulate_into(c, inp, plan, fault=None):
    """ppea_pwgrad_ex_bf16 in torch.  fault: drop_split | scatter_tn (t and n exchanged in the tap scatter) | window_shift."""
    w, r = emulate_pwgrad(inp["p"], inp["q"], plan, fault)
    if c.taps == 9:
        M, N = 9 * c.Ch, c.N
        i = torch.arange(M * N)
        m, n = i // N, i % N
        tp, mo = m // c.Ch, m % c.Ch
        o = (mo * 9 + tp) * N + n if fault == "scatter_tn" else (mo * N + n) * 9 + tp
        flat = torch.empty(M * N)
        flat[o] = w.reshape(-1)
        w = flat.view(c.Ch, c.N, 3, 3)
    out = dict(dw=w.bfloat16() if c.wdt == "bf16" else w)
    if c.bdt is not None:
        r0, rn = bias_window(c)
        if fault == "window_shift":                          # every row of the window one further (the last wraps)
            r = r.roll(-1)
        b = r[r0:r0 + rn]
        out["db"] = b.bfloat16() if c.bdt == "bf16" else b
    return out


def emulate_tapsum(c, inp, fault=None):
    """fault: col_inside (the dx = -1 tap at x = 0 reads the plane's own column 0 instead of the zero outside it)."""
    T = inp["T"].float().view(c.B, 9, c.Ch, c.H, c.W)
    Tp = F.pad(T, (1, 1, 1, 1))
    if fault == "col_inside":
        Tp[..., 0] = Tp[..., 1]
    acc = torch.zeros(c.B, c.Ch, c.H, c.W) if inp["bias"] is None else inp["bias"].float().view(1, -1, 1, 1).expand(c.B, c.Ch, c.H, c.W).clone()
    for t, (dy, dx) in enumerate((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)):
        acc = acc + Tp[:, t, :, 1 + dy:1 + dy + c.H, 1 + dx:1 + dx + c.W]
    pre = acc.bfloat16()
    return dict(pre=pre, h=_gelu32(pre.float()).bfloat16(), dT=shift_taps(inp["g"]))


def pw_cases():
    return TILE_CASES + EDGE_CASES
