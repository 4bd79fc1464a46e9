"""TEST INFRASTRUCTURE ONLY -- case tables, seeded inputs, float64 references and per-element error bounds for the
large-kernel depthwise kernels: csrc/dwconv_mfma.hip (row-band, window-sharing and batch-major MFMA kernels), csrc/dwconv_wgrad.hip
(filter gradient) and csrc/dwconv_lk.hip (fp32 vector kernel).  Pure torch; everything is a function of its arguments and the seed.
Which kernel a row reaches is NOT restated here: every row names the arm it is there for and tests/test_dwconv_arms_cpu.py asks
the library's own plan calls (ops.dwconv_lk_plan and friends, answered by the functions the launches go by) whether it does.

THE BOUND (the dense-conv pin's, oracle/conv_inputs.py, derived there).  bf16 operands multiply exactly into fp32; n products
with magnitude sum A = sum |x_i w_i| added in fp32 in any order stay within n * 2^-23 * A of the exact sum; one rounding to bf16
adds 2^-8 of the value:

    bf16 output:  |got - ref| <= 2^-8 |ref| + (1 + 2^-8) * n * 2^-23 * A
    fp32 output:  |got - ref| <=                           n * 2^-23 * A

n = K*K (forward), K*K + 25 (data gradient of the pair), N*H*W (filter gradient).  Bias + activation rows: |bias| joins A, the
activation is applied in float64 (ReLU is 1-Lipschitz, so the bound on the pre-activation carries over).  NaN / Inf are outside
every bound and no element is excluded.

INPUTS THAT MAKE INDEX ERRORS VISIBLE.  Planes alternate in scale by 64 along n and along c (a checkerboard over (n, c)), the
first / last row and column of every plane are 8 x the interior, filters are randn / K with the four corner taps and the
centre tap at +-1: a row leaked from a neighbouring plane or a stale LDS image, a dropped or mirrored tap, a shifted store all
land far outside the bound (tests/test_dwconv_arms_cpu.py applies such faults to a torch evaluation of every row)."""
import collections

import torch
import torch.nn.functional as F

from oracle.conv_inputs import U_ACC, U_BF16, worst  # noqa: F401  (worst: re-exported for the tests)

KS_ALL = (31, 29, 27, 13)
LDS_LIMIT = 160 * 1024
GUARD = 64                         # guard elements on each side of an output
GUARD_BITS = {torch.bfloat16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A)}
CPU_MACS = 6e8                     # rows above elements * K * K of this run their numerics on the GPU only (seconds per conv here)

Row = collections.namedtuple("Row", "name N C H W K KS mode variant relu arm claims")
# mode 0 forward / 1 data gradient; variant "plain" | "stats" | "bn" | "bias_act"; arm: rb(...) | bm(...) | None (refused);
# claims: plan field -> value or predicate the plan must meet


def rb(K, KS, mode, NSEG, BN=0, WS=0, BA=0):
    """dwconv_mfma_kernel<K, KS, mode, NSEG, BN, WS, BA>"""
    return ("rb", K, KS, mode, NSEG, BN, WS, BA)


def bm(K, mode, H, NTX, BN=0):
    """dwconv_bm_kernel<K, 5, mode, H, NY, NTX, RS, BN>  (NY = 6, RS = 1; the 48-row arm: NY = 12, RS = 4)"""
    return ("bm", K, 5, mode, H, NTX, BN)


def arm_of_plan(p, K, KS, mode):
    if p["family"] == 1:
        return rb(K, KS, mode, p["NSEG"], p["BN"], p["WS"], p["BA"])
    if p["family"] == 2:
        return bm(K, mode, p["H"], p["NTX"], p["BN"])
    return None


_BM_HN = {29: ((24, 4), (24, 5)), 27: ((12, 1), (12, 2), (12, 3)), 13: ((6, 1), (6, 2), (6, 3))}
# every instantiation csrc/dwconv_mfma.hip builds: 74 row-band + 25 batch-major
ALL_ARMS = frozenset(
    [rb(K, KS, m, s) for K in KS_ALL for KS in (0, 5) for m in (0, 1) for s in (2, 3, 5)]
    + [rb(K, 5, 0, s, BN=1) for K in KS_ALL for s in (2, 3, 5)]
    + [rb(K, 0, 0, s, BA=1) for K in KS_ALL for s in (2, 3, 5)]
    + [rb(31, 5, 0, 5, WS=1), rb(31, 5, 0, 5, BN=1, WS=1)]
    + [bm(K, m, H, n, BN) for K, hn in _BM_HN.items() for H, n in hn for m, BN in ((0, 0), (0, 1), (1, 0))]
    + [bm(31, 1, 48, 2)])
# built but never launched: nothing (the kernel asserts that the data gradient has no window-sharing instantiation)
UNREACHABLE = {}
# launch outcomes of the host plan that no shape of the sweep reaches: none (the plans assert that their searches end
# at band 32 and at groups of 12 images)
UNREACHED_OUTCOMES = {"band": (), "gi": ()}


def _r(name, shape, K, KS=5, mode=0, variant="plain", relu=False, arm=None, **claims):
    N, C, H, W = shape
    return Row(name, N, C, H, W, K, KS, mode, variant, relu, arm, claims)


def ge(v):
    f = lambda x: x >= v            # noqa: E731
    f.__doc__ = f">= {v}"
    return f


# ---------------------------------------------------------------------------------------------
# row-band kernel.  NSEG by width (K >= 27): W <= 32 -> 2, 33..48 and 81..96 -> 3, 49..80 and >= 97 -> 5.
# ---------------------------------------------------------------------------------------------
# (N, C, H, W) per NSEG, cycled over (K, KS, mode): stacked short planes with a ragged last group, tall planes with a ragged
# last band, odd W, W % 8 == 4, W % 8 == 0, ragged last segment / tile; none is a batch-major shape
_RB_SHAPES = {
    2: ((5, 3, 20, 20), (2, 2, 50, 9), (3, 5, 7, 32), (1, 3, 33, 24)),
    3: ((3, 2, 20, 36), (1, 3, 50, 37), (5, 2, 10, 40), (2, 3, 17, 96)),
    5: ((3, 2, 20, 52), (1, 2, 50, 75), (2, 3, 9, 64), (1, 2, 35, 104)),
}


def _rowband_cases():
    rows, i = [], 0
    for K in KS_ALL:
        for KS in (0, 5):
            for mode in (0, 1):
                for nseg in (2, 3, 5):
                    shape = _RB_SHAPES[nseg][i % 4]
                    i += 1
                    rows.append(_r(f"rb_k{K}_ks{KS}_{'dgrad' if mode else 'fwd'}_nseg{nseg}", shape, K, KS, mode,
                                   arm=rb(K, KS, mode, nseg)))
    return rows


ROWBAND_CASES = tuple(_rowband_cases()) + (
    # band 32: the data gradient of the pair stages two inputs, 48-row bands no longer fit (K >= 27)
    # at NSEG 5, whose rows are the widest; bands of 32 with a ragged last one
    _r("rb_band32_k31", (1, 2, 70, 52), 31, 5, 1, arm=rb(31, 5, 1, 5), band=32, bands=3, G=1, fast=0),
    _r("rb_band32_k27", (2, 1, 96, 64), 27, 5, 1, arm=rb(27, 5, 1, 5), band=32, bands=3, G=1),
    _r("rb_band48_k31_nseg3", (1, 2, 70, 40), 31, 5, 1, arm=rb(31, 5, 1, 3), band=48, bands=2),
    # stacked (G > 1) with a ragged last group; tall (bands > 1) with a ragged last band
    _r("rb_stack_ragged", (5, 3, 20, 24), 31, 5, 0, arm=rb(31, 5, 0, 2), band=48, G=2, bands=1, items_per_channel=3, fast=1),
    _r("rb_tall_ragged", (1, 3, 100, 40), 29, 5, 0, arm=rb(29, 5, 0, 3), band=48, G=1, bands=3, fast=0),
    # prefetched staging both ways on one plane size: W % 8 == 0 against W % 8 == 4 and odd W
    _r("rb_fast_w24", (3, 3, 16, 24), 27, 5, 0, arm=rb(27, 5, 0, 2), fast=1, G=3),
    _r("rb_slow_w20", (3, 3, 16, 20), 27, 5, 0, arm=rb(27, 5, 0, 2), fast=0, G=3),
    _r("rb_slow_w21", (3, 3, 16, 21), 27, 5, 1, arm=rb(27, 5, 1, 2), fast=0),
    # too many pieces for the prefetch slots although W % 8 == 0 and one band (24 stacked planes of 2 rows), and just enough
    _r("rb_slow_pieces", (30, 2, 2, 24), 13, 5, 0, arm=rb(13, 5, 0, 2), fast=0, bands=1, G=24),
    _r("rb_fast_pieces", (12, 2, 4, 24), 13, 5, 0, arm=rb(13, 5, 0, 2), fast=1, bands=1, G=12),
    # the smallest tensors: fewer than 8 elements are refused, 8 are served
    _r("rb_refused_1x1", (1, 1, 1, 1), 31, 5, 0, arm=None),
    _r("rb_1x8", (1, 1, 1, 8), 31, 5, 0, arm=rb(31, 5, 0, 2)),
    _r("rb_1x8_dgrad", (1, 1, 1, 8), 13, 5, 1, arm=rb(13, 5, 1, 2)),
    # several items per wave: 3 items over 2 waves (the channel's last wave gets one), 4 over 2 (even), 3 over 1; short, narrow
    # planes the batch-major variant refuses; the last group of each is ragged (a stale LDS image under the next item)
    _r("rb_ipw2_ragged_k13", (13, 512, 7, 20), 13, 5, 0, arm=rb(13, 5, 0, 2), ipw=2, wpc=2, items_per_channel=3, G=6),
    _r("rb_ipw2_even_k13", (19, 512, 7, 20), 13, 5, 1, arm=rb(13, 5, 1, 2), ipw=2, wpc=2, items_per_channel=4, G=6),
    _r("rb_ipw2_fast_k13", (13, 512, 7, 24), 13, 5, 0, arm=rb(13, 5, 0, 2), ipw=2, wpc=2, fast=1),
    _r("rb_ipw3_k27", (19, 1024, 5, 8), 27, 5, 0, arm=rb(27, 5, 0, 2), ipw=ge(2), wpc=1, fast=1),
    _r("rb_ipw2_k31", (19, 512, 5, 8), 31, 5, 0, arm=rb(31, 5, 0, 2), ipw=2, wpc=2, items_per_channel=3, fast=1),
    _r("rb_ipw2_k31_dgrad", (19, 512, 5, 8), 31, 5, 1, arm=rb(31, 5, 1, 2), ipw=ge(2)),
    _r("rb_ipw2_k29_segs", (1, 1024, 3, 100), 29, 0, 0, arm=rb(29, 0, 0, 5), ipw=2, wpc=1, segs=2, fast=0),
    # the four maps of a 384 x 640 frame (RepLKNet-31B: 128 / 256 / 512 / 1024 channels, batch 12), on the row-band kernel today;
    # reduced N and C where the tensor would pass 3 M elements
    _r("ddad_96x160_k31_fwd", (2, 4, 96, 160), 31, 5, 0, arm=rb(31, 5, 0, 5, WS=1), band=48, bands=2),
    _r("ddad_96x160_k31_dgrad", (2, 4, 96, 160), 31, 5, 1, arm=rb(31, 5, 1, 5), band=32, bands=3),
    _r("ddad_48x80_k29_fwd", (2, 8, 48, 80), 29, 5, 0, arm=rb(29, 5, 0, 5), band=48, bands=1),
    _r("ddad_48x80_k29_dgrad", (2, 8, 48, 80), 29, 5, 1, arm=rb(29, 5, 1, 5), band=32, bands=2),
    _r("ddad_24x40_k27_fwd", (12, 16, 24, 40), 27, 5, 0, arm=rb(27, 5, 0, 3), G=2),
    _r("ddad_24x40_k27_dgrad", (12, 16, 24, 40), 27, 5, 1, arm=rb(27, 5, 1, 3)),
    _r("ddad_12x20_k13_fwd", (12, 1024, 12, 20), 13, 5, 0, arm=rb(13, 5, 0, 2), ipw=ge(2), wpc=1, G=4),
    _r("ddad_12x20_k13_dgrad", (12, 1024, 12, 20), 13, 5, 1, arm=rb(13, 5, 1, 2), ipw=ge(2)),
)

# window sharing (k = 31 with the 5 x 5 branch, forward, NSEG 5, every item one 48-row band): 4 (even) and 5 (odd) column
# tiles, a ragged last tile, two bands, a second segment of 2 tiles, several items per wave
WS_CASES = (
    _r("ws_48x64_even", (1, 2, 48, 64), 31, arm=rb(31, 5, 0, 5, WS=1), bands=1, segs=1),
    _r("ws_48x80_odd", (2, 3, 48, 80), 31, arm=rb(31, 5, 0, 5, WS=1), bands=1, segs=1, fast=1),
    _r("ws_96x72_ragged_tile", (1, 2, 96, 72), 31, arm=rb(31, 5, 0, 5, WS=1), bands=2, fast=0),
    _r("ws_48x104_two_segs", (2, 1, 48, 104), 31, arm=rb(31, 5, 0, 5, WS=1), segs=2),
    _r("ws_48x75_odd_w", (1, 2, 48, 75), 31, arm=rb(31, 5, 0, 5, WS=1), fast=0),
    _r("ws_ipw2", (1, 1024, 48, 104), 31, arm=rb(31, 5, 0, 5, WS=1), ipw=2, wpc=1),
    _r("ws_48x64_stats", (1, 2, 48, 64), 31, variant="stats", arm=rb(31, 5, 0, 5, WS=1)),
    _r("ws_96x80_stats", (2, 2, 96, 80), 31, variant="stats", arm=rb(31, 5, 0, 5, WS=1), bands=2),
    # not window sharing: H % 48 != 0, and the data gradient (its band is 32: see the static_assert in the kernel)
    _r("ws_refused_h50", (1, 2, 50, 64), 31, arm=rb(31, 5, 0, 5), bands=2),
    _r("ws_refused_dgrad", (1, 2, 96, 64), 31, 5, 1, arm=rb(31, 5, 1, 5), band=32),
)


# batch-major: every (K, H, NTX) of choose_bm in both modes + the 48-row data gradient; N < gi, N % gi != 0, C % CPW != 0
# (CPW = 4, 2, 1, 1 channels per workgroup at H = 6, 12, 24, 48), VEC 8 / 4, gi 16 / 12
def _bm_cases():
    rows = []
    widths = {(24, 4): (64, 52), (24, 5): (80, 68), (12, 1): (16, 12), (12, 2): (32, 20), (12, 3): (40, 44),
              (6, 1): (8, 4), (6, 2): (24, 20), (6, 3): (48, 36)}
    i = 0
    for K, hn in _BM_HN.items():
        for H, ntx in hn:
            for mode in (0, 1):
                W = widths[(H, ntx)][(i + mode) % 2]
                N, C = ((3, 5), (17, 3), (16, 2), (13, 1))[i % 4]
                i += 1
                rows.append(_r(f"bm_k{K}_h{H}_ntx{ntx}_{'dgrad' if mode else 'fwd'}", (N, C, H, W), K, 5, mode,
                               arm=bm(K, mode, H, ntx), VEC=8 if W % 8 == 0 else 4))
    return rows


BM_CASES = tuple(_bm_cases()) + (
    _r("bm_k29_gi12", (14, 1, 24, 80), 29, 5, 1, arm=bm(29, 1, 24, 5), gi=12, ngroups=2),
    _r("bm_k27_vec4_idle_wave", (5, 3, 12, 20), 27, 5, 0, arm=bm(27, 0, 12, 2), VEC=4, gi=16),
    _r("bm_k13_two_groups", (33, 2, 6, 44), 13, 5, 0, arm=bm(13, 0, 6, 3), ngroups=3, VEC=4),
    # the 48-row arm: the N threshold 10 N >= 7 * 16 * ceil(N / 16) from both sides (N = 11 | 12, 22 | 23), wgpc > 1
    _r("bm48_n12", (12, 2, 48, 56), 31, 5, 1, arm=bm(31, 1, 48, 2), gi=16, wgpc=ge(2)),
    _r("bm48_n11_rowband", (11, 2, 48, 56), 31, 5, 1, arm=rb(31, 5, 1, 5)),
    _r("bm48_n23", (23, 1, 48, 24), 31, 5, 1, arm=bm(31, 1, 48, 2), gi=12, ngroups=2),
    _r("bm48_n22_rowband", (22, 1, 48, 24), 31, 5, 1, arm=rb(31, 5, 1, 2)),
    _r("bm48_w160", (12, 1, 48, 160), 31, 5, 1, arm=bm(31, 1, 48, 2), wgpc=10, cpw=1),
    # two workgroups per channel of two column tiles and one (the full-size shape [12,128,48,160] walks 5 + 5)
    _r("bm48_cpw2", (12, 128, 48, 40), 31, 5, 1, arm=bm(31, 1, 48, 2), wgpc=2, cpw=2),
    _r("bm48_w60_rowband", (12, 2, 48, 60), 31, 5, 1, arm=rb(31, 5, 1, 5)),          # W % 8 != 0
    # W % 4 != 0 and other heights stay on the row-band kernel
    _r("bm_refused_w42", (12, 2, 12, 42), 27, 5, 0, arm=rb(27, 5, 0, 3)),
    _r("bm_refused_ks0", (12, 2, 12, 40), 27, 0, 0, arm=rb(27, 0, 0, 3)),
)


# epilogue statistics, fused input BatchNorm, bias + activation
def _variant_cases():
    rows = []
    for K, nseg, shape in ((31, 2, (5, 3, 20, 24)), (29, 3, (2, 3, 50, 37)), (27, 5, (3, 2, 20, 52)), (13, 2, (13, 512, 7, 20))):
        rows.append(_r(f"stats_rb_k{K}_nseg{nseg}", shape, K, variant="stats", arm=rb(K, 5, 0, nseg)))
    for K, hn in _BM_HN.items():
        H, ntx = hn[-1]
        rows.append(_r(f"stats_bm_k{K}_h{H}", (17, 3, H, 16 * ntx), K, variant="stats", arm=bm(K, 0, H, ntx)))
    i = 0
    for K in KS_ALL:
        for nseg in (2, 3, 5):
            shape = _RB_SHAPES[nseg][(i + 1) % 4]
            i += 1
            rows.append(_r(f"bn_rb_k{K}_nseg{nseg}", shape, K, variant="bn", arm=rb(K, 5, 0, nseg, BN=1)))
    rows.append(_r("bn_ws_48x80", (2, 3, 48, 80), 31, variant="bn", arm=rb(31, 5, 0, 5, BN=1, WS=1)))
    rows.append(_r("bn_ws_96x75", (1, 2, 96, 75), 31, variant="bn", arm=rb(31, 5, 0, 5, BN=1, WS=1)))
    rows.append(_r("bn_rb_ipw2", (13, 512, 7, 20), 13, variant="bn", arm=rb(13, 5, 0, 2, BN=1), ipw=2))
    for K, hn in _BM_HN.items():
        for H, ntx in hn:
            W = 16 * ntx - (4 if (ntx + H) % 2 else 0)
            rows.append(_r(f"bn_bm_k{K}_h{H}_ntx{ntx}", (17 if ntx % 2 else 5, 3, H, W), K, variant="bn", arm=bm(K, 0, H, ntx, BN=1)))
    i = 0
    for K in KS_ALL:
        for nseg in (2, 3, 5):
            for relu in (False, True):
                shape = _RB_SHAPES[nseg][i % 4]
                i += 1
                rows.append(_r(f"ba_k{K}_nseg{nseg}_{'relu' if relu else 'linear'}", shape, K, 0, 0, "bias_act", relu,
                               arm=rb(K, 0, 0, nseg, BA=1)))
    return tuple(rows)


VARIANT_CASES = _variant_cases()

# filter gradient (csrc/dwconv_wgrad.hip): (row, claims on ops.dwconv_lk_bwd_filter_plan).  parts > 1 with a ragged last part,
# a last round of fewer than four rows, N * H < 4, W % 8 != 0, W % 16 != 0
FILTER_CASES = (
    (_r("wg_ragged_part", (3, 4, 7, 20), 13, 5), dict(parts=ge(2), vec=0, ragged_part=True)),
    (_r("wg_short_round", (1, 2, 6, 24), 27, 5), dict(vec=1, short_round=True)),
    (_r("wg_nh3", (1, 3, 3, 16), 31, 5), dict(parts=1, rounds=1, short_round=True)),
    (_r("wg_nh1_ks0", (1, 2, 1, 8), 13, 0), dict(parts=1, rounds=1)),
    (_r("wg_w37", (2, 3, 10, 37), 29, 5), dict(vec=0)),
    (_r("wg_one_part_5_rounds", (2, 2048, 9, 40), 13, 5), dict(parts=1, vec=1, rounds=5, short_round=True)),
    (_r("wg_two_parts_3_rounds", (2, 1024, 9, 104), 13, 5), dict(vec=1, parts=2, rounds=3, short_round=True)),
    (_r("wg_w104_k31", (2, 2, 50, 104), 31, 5), dict(vec=1, parts=ge(2), rounds=1)),
)

# fp32 vector kernel (csrc/dwconv_lk.hip): one plane size per CFGS_<K> entry, and the generic kernel (K = 9, and KS = 3)
# (K, index, (H, W)); io in {"f32", "bf16"}, mode, KS cycled over the rows
_F32_PICKS = ((31, 0, (25, 31)), (31, 1, (13, 37)), (29, 0, (13, 37)), (29, 1, (25, 31)), (27, 0, (11, 39)), (27, 2, (13, 43)),
              (13, 0, (11, 19)), (13, 2, (13, 9)), (9, -1, (7, 9)), (13, -1, (6, 20)))
# CFGS entries `pick_cfg` never returns: their tile is as tall as the entry before them and narrower, so their cover cost is
# never the smaller one and the first of equals wins
F32_UNREACHABLE = ((27, 1), (13, 1))
F32_CONFIGS = {31: 2, 29: 2, 27: 3, 13: 3}
F32Row = collections.namedtuple("F32Row", "row io index")


def _f32_cases():
    rows = []
    for i, (K, idx, (H, W)) in enumerate(_F32_PICKS):
        KS = 3 if (idx == -1 and K == 13) else (0 if K == 9 else (0, 5)[i % 2])
        for j, io in enumerate(("f32", "bf16")):
            mode = (i + j) % 2
            rows.append(F32Row(_r(f"f32_k{K}_cfg{idx}_{io}_{'dgrad' if mode else 'fwd'}_ks{KS}", (2, 3, H, W), K, KS, mode),
                               io, idx))
    return tuple(rows)


F32_CASES = _f32_cases()


def mfma_rows():
    """Every row that goes through ops.dwconv_lk_plan."""
    return ROWBAND_CASES + WS_CASES + BM_CASES + VARIANT_CASES


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _seed(r):
    s = 31
    for v in (r.N, r.C, r.H, r.W, r.K, r.KS, r.mode, sum(ord(ch) for ch in r.name)):
        s = (s * 1000003 + v) % (2 ** 31 - 1)
    return s


def elements(r):
    return r.N * r.C * r.H * r.W


def cpu_sized(r):
    return elements(r) * r.K * r.K <= CPU_MACS


def _activation(r, g):
    """Seeded normal values on the bf16 grid; planes alternate in scale by 64 over (n, c), edges 8 x the interior."""
    x = torch.randn(r.N, r.C, r.H, r.W, generator=g)
    edge = torch.ones(r.H, r.W)
    edge[0, :] = edge[-1, :] = 8.0
    edge[:, 0] = edge[:, -1] = 8.0
    n, c = torch.arange(r.N)[:, None], torch.arange(r.C)[None, :]
    plane = torch.where((n + c) % 2 == 1, 64.0, 1.0)
    return (x * edge * plane[:, :, None, None]).bfloat16()


def _filter(C, K, g):
    """randn / K with the corner taps and the centre at +-1 (TL, BR = s; TR, BL = -s; centre s; s alternates over c)."""
    w = torch.randn(C, 1, K, K, generator=g) / K
    s = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    w[:, 0, 0, 0] = w[:, 0, K - 1, K - 1] = w[:, 0, K // 2, K // 2] = s
    w[:, 0, 0, K - 1] = w[:, 0, K - 1, 0] = -s
    return w.bfloat16().float()


def make_inputs(r):
    """-> dict(x, gb, gs bf16 [N,C,H,W]; wb [C,1,K,K], ws [C,1,KS,KS] or None, fp32 on the bf16 grid; bias fp32 [C]; gamma,
    beta fp32 [C]).  Forward rows convolve x, data-gradient rows gb (and gs through the small filter)."""
    g = torch.Generator().manual_seed(_seed(r))
    inp = dict(x=_activation(r, g), gb=_activation(r, g), gs=_activation(r, g), wb=_filter(r.C, r.K, g),
               ws=_filter(r.C, r.KS, g) if r.KS else None)
    inp["bias"] = 0.5 * torch.randn(r.C, generator=g)
    inp["gamma"] = torch.rand(r.C, generator=g) + 0.5
    inp["beta"] = 0.2 * torch.randn(r.C, generator=g)
    return inp


# ---------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------
def dw64(x, w):
    return F.conv2d(x, w, None, 1, w.shape[-1] // 2, 1, x.shape[1])


def direct_sum(x, w):
    """The depthwise convolution written out (for the tiny shapes the CPU test checks dw64 against)."""
    N, C, H, W = x.shape
    K = w.shape[-1]
    P = K // 2
    y = torch.zeros(N, C, H, W, dtype=torch.float64)
    for ky in range(K):
        for kx in range(K):
            for yy in range(H):
                iy = yy + ky - P
                if not 0 <= iy < H:
                    continue
                for xx in range(W):
                    ix = xx + kx - P
                    if 0 <= ix < W:
                        y[:, :, yy, xx] += x[:, :, iy, ix].double() * w[:, 0, ky, kx].double()
    return y


def _dgrad64(gb, gs, wb, ws):
    """d/dx sum(dw(x, wb) * gb + dw(x, ws) * gs) by autograd in double."""
    x = torch.zeros_like(gb, requires_grad=True)
    out = (dw64(x, wb) * gb).sum()
    if ws is not None:
        out = out + (dw64(x, ws) * gs).sum()
    return torch.autograd.grad(out, x)[0]


def bf16_bound(ref, A, n):
    return U_BF16 * ref.abs() + (1 + U_BF16) * n * U_ACC * A


def reference(r, inp, x=None, device="cpu"):
    """float64 outputs of one row on the operands as given -> dict name -> (ref, bound), float64 tensors on `device`:
    forward y_big (and y_small with KS), data gradient dx.  `x`: the activation to convolve instead of inp["x"] (the
    fused-BatchNorm rows pass the device's own relu(BN(z)))."""
    d = lambda t: None if t is None else t.to(device).double()        # noqa: E731
    wb, ws = d(inp["wb"]), d(inp["ws"])
    if r.mode == 1:
        gb, gs = d(inp["gb"]), d(inp["gs"])
        dx = _dgrad64(gb, gs, wb, ws)
        A = _dgrad64(gb.abs(), gs.abs(), wb.abs(), None if ws is None else ws.abs())
        return dict(dx=(dx, bf16_bound(dx, A, r.K * r.K + r.KS * r.KS)))
    xin = d(inp["x"] if x is None else x)
    z, A = dw64(xin, wb), dw64(xin.abs(), wb.abs())
    if r.variant == "bias_act":
        b = d(inp["bias"])[None, :, None, None]
        z, A = z + b, A + b.abs()
        if r.relu:
            z = torch.relu(z)
    out = dict(y_big=(z, bf16_bound(z, A, r.K * r.K)))
    if ws is not None:
        zs = dw64(xin, ws)
        out["y_small"] = (zs, bf16_bound(zs, dw64(xin.abs(), ws.abs()), r.KS * r.KS))
    return out


def reference_filter(r, inp, device="cpu"):
    """float64 filter gradients of the pair by autograd -> dict(dw_big, dw_small) of (ref [C,K,K], bound), n = N*H*W."""
    d = lambda t: t.to(device).double()                               # noqa: E731
    x, n = d(inp["x"]), r.N * r.H * r.W
    out = {}
    for key, K, go in (("dw_big", r.K, d(inp["gb"])),) + ((("dw_small", r.KS, d(inp["gs"])),) if r.KS else ()):
        w = torch.zeros(r.C, 1, K, K, dtype=torch.float64, device=device, requires_grad=True)
        wa = torch.zeros_like(w, requires_grad=True)
        dw = torch.autograd.grad((dw64(x, w) * go).sum(), w)[0]
        A = torch.autograd.grad((dw64(x.abs(), wa) * go.abs()).sum(), wa)[0]
        out[key] = (dw[:, 0], n * U_ACC * A[:, 0])
    return out


def reference_f32(fr, inp, device="cpu"):
    """The fp32 vector kernel's row: as `reference` with the fp32-output bound n * 2^-23 * A (+ 2^-8 |ref| for bf16 I/O)."""
    r = fr.row
    out = {}
    for key, (ref, bound) in reference(r, inp, device=device).items():
        acc = (bound - U_BF16 * ref.abs()) / (1 + U_BF16)
        out[key] = (ref, acc if fr.io == "f32" else bound)
    return out


# ---------------------------------------------------------------------------------------------
# a torch evaluation of a row, and the faults the bound has to catch
# ---------------------------------------------------------------------------------------------
FAULTS = ("drop_tap", "mirror_x", "shift_column", "last_tile_unwritten", "halo_row_from_neighbour", "small_branch_row_offset", "nan")


def fault_applies(r, fault):
    if fault == "halo_row_from_neighbour":
        return r.N * r.C > 1
    if fault == "small_branch_row_offset":
        return r.KS == 5 and r.H > 1
    if fault == "shift_column":
        return r.W > 1
    return True


def evaluate(r, inp, fault=None, round_bf16=False):
    """fp32 torch evaluation of the row (what a correct fp32-accumulating kernel computes, in another order) -> dict as
    `reference`'s keys -> tensor; `fault`: one of FAULTS, a wrong kernel's output.  round_bf16: rounded to bf16 as stored."""
    K, P = r.K, r.K // 2
    wb, ws = inp["wb"].clone(), None if inp["ws"] is None else inp["ws"].clone()
    src = (inp["gb"] if r.mode else inp["x"]).float().clone()
    src_s = (inp["gs"] if r.mode else inp["x"]).float().clone()
    if r.mode:                                                          # the data gradient is the convolution with the flipped filters
        wb, ws = wb.flip(-1, -2), None if ws is None else ws.flip(-1, -2)
    if fault == "drop_tap":
        # a corner tap meets the plane only where both extents pass K / 2; smaller planes lose the centre tap instead
        if min(r.H, r.W) > P:
            wb[:, 0, 0, 0] = 0
        else:
            wb[:, 0, P, P] = 0
    if fault == "mirror_x":
        wb = wb.flip(-1)
    if fault == "halo_row_from_neighbour":
        flat = src.reshape(r.N * r.C, r.H, r.W)
        flat[:, 0, :] = flat.roll(-1, 0)[:, 0, :].clone()
        src = flat.reshape(r.N, r.C, r.H, r.W)
    if fault == "small_branch_row_offset" and r.mode:
        src_s = src_s.roll(1, 2)
    yb = F.conv2d(src, wb, None, 1, P, 1, r.C)
    ys = None if ws is None else F.conv2d(src_s, ws, None, 1, r.KS // 2, 1, r.C)
    if fault == "small_branch_row_offset" and not r.mode:
        ys = ys.roll(1, 2)
    if r.variant == "bias_act":
        yb = yb + inp["bias"][None, :, None, None]
        if r.relu:
            yb = torch.relu(yb)
    out = dict(dx=yb + ys if ys is not None else yb) if r.mode else dict(y_big=yb, **({} if ys is None else dict(y_small=ys)))
    first = next(iter(out))
    if fault == "shift_column":
        out[first] = out[first].roll(1, 3)
    if fault == "last_tile_unwritten":
        out[first] = out[first].clone()
        out[first][..., 16 * ((r.W - 1) // 16):] = float("nan")
    if fault == "nan":
        out[first] = out[first].clone()
        out[first].view(-1)[out[first].numel() // 2] = float("nan")
    if round_bf16:
        out = {k: v.bfloat16() for k, v in out.items()}
    return out


# ---------------------------------------------------------------------------------------------
# guarded outputs
# ---------------------------------------------------------------------------------------------
def guarded(shape, dtype, device):
    """-> (buffer, tensor): `tensor` a NaN-filled view of `shape` into a longer buffer with GUARD elements of a fixed bit
    pattern on each side."""
    idt, bits = GUARD_BITS[dtype]
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + 2 * GUARD,), bits, dtype=idt, device=device)
    body = buf[GUARD:GUARD + numel].view(dtype)
    body.fill_(float("nan"))
    return buf, body.view(shape)


def guards_intact(buf, dtype):
    bits = GUARD_BITS[dtype][1]
    return bool((buf[:GUARD] == bits).all()) and bool((buf[-GUARD:] == bits).all())
