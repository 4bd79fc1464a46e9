"""CPU proofs behind tests/test_dwconv_arms_gpu.py: the float64 reference of oracle/dwconv_inputs.py agrees with a written-out
sum, every table row reaches the kernel arm it names according to the library's own plan calls (answered by the functions the
launches go by), the rows reach every arm that any shape of a grid reaches (the instantiations no shape reaches are listed by
name), a torch evaluation of every row stays inside the per-element bound, and seven synthetic kernel faults leave it on every row."""
import functools

import pytest
import torch

from oracle import dwconv_inputs as D

MFMA_ROWS = D.mfma_rows()
NUMERIC_ROWS = [r for r in MFMA_ROWS if r.arm is not None and D.cpu_sized(r)]
# rows whose float64 convolution takes too long here (elements * K * K > D.CPU_MACS): their numerics run on the GPU only
GPU_ONLY_NUMERICS = sorted(r.name for r in MFMA_ROWS if r.arm is not None and not D.cpu_sized(r))
SWEEP = dict(Nmax=33, Cs=(1, 3, 64, 512, 1024), Hmax=130, Wmax=260)
# (KS, mode, variant) combinations that have kernels; "stats" launches what "plain" launches
COMBOS = ((5, 0, "plain"), (5, 1, "plain"), (5, 0, "bn"), (0, 0, "plain"), (0, 1, "plain"), (0, 0, "bias_act"))


def _ids(rows):
    return [r.name for r in rows]


def _plan(r):
    from ppeadepth import ops
    return ops.dwconv_lk_plan(r.N, r.C, r.H, r.W, r.K, r.KS, r.mode, r.variant)


@functools.lru_cache(maxsize=None)
def _sweep():
    """-> (arms reached, every distinct plan with its (K, KS, mode), summaries) over the grid."""
    from ppeadepth import ops
    arms, plans, summaries = set(), [], []
    for K in D.KS_ALL:
        for KS, mode, variant in COMBOS:
            ps, summ = ops.dwconv_lk_plan_sweep(K, KS, mode, variant, SWEEP["Nmax"], SWEEP["Cs"], SWEEP["Hmax"], SWEEP["Wmax"])
            summaries.append(summ)
            for p in ps:
                plans.append((K, KS, mode, p))
                arms.add(D.arm_of_plan(p, K, KS, mode))
    return frozenset(arms), plans, summaries


@functools.lru_cache(maxsize=None)
def _numerics(name):
    r = {x.name: x for x in MFMA_ROWS}[name]
    inp = D.make_inputs(r)
    return r, inp, D.reference(r, inp)


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K,KS,mode", [((2, 3, 4, 9), 13, 5, 0), ((3, 2, 5, 3), 13, 5, 1)])
def test_reference_is_the_written_out_sum(shape, K, KS, mode):
    r = D._r("tiny", shape, K, KS, mode)
    inp = D.make_inputs(r)
    ref = D.reference(r, inp)
    if mode == 0:
        assert torch.allclose(ref["y_big"][0], D.direct_sum(inp["x"], inp["wb"]), rtol=0, atol=1e-9)
        assert torch.allclose(ref["y_small"][0], D.direct_sum(inp["x"], inp["ws"]), rtol=0, atol=1e-9)
    else:       # the data gradient of a correlation is the correlation of the gradient with the filter turned by 180 degrees
        want = D.direct_sum(inp["gb"], inp["wb"].flip(-1, -2)) + D.direct_sum(inp["gs"], inp["ws"].flip(-1, -2))
        assert torch.allclose(ref["dx"][0], want, rtol=0, atol=1e-9)
    for ref_t, bound in ref.values():
        assert bool((bound >= 0).all()) and bound.shape == ref_t.shape


def test_inputs_expose_neighbours_edges_and_taps():
    r = D._r("probe", (2, 3, 9, 11), 13)
    inp = D.make_inputs(r)
    x = inp["x"].float().abs()
    interior = x[:, :, 1:-1, 1:-1].mean((2, 3))
    assert float(interior[0, 1] / interior[0, 0]) > 20 and float(interior[1, 0] / interior[0, 0]) > 20      # planes alternate by 64
    assert float(x[0, 0, 0].mean() / interior[0, 0]) > 4 and float(x[0, 0, :, -1].mean() / interior[0, 0]) > 4
    w = inp["wb"]
    assert set(w[:, 0, 0, 0].abs().tolist()) == {1.0} and set(w[:, 0, 6, 6].abs().tolist()) == {1.0}
    assert torch.equal(w[:, 0, 0, 0], -w[:, 0, 0, 12]) and torch.equal(w[:, 0, 12, 12], -w[:, 0, 12, 0])
    assert torch.equal(w, w.bfloat16().float()) and torch.equal(inp["ws"], inp["ws"].bfloat16().float())


# ---------------------------------------------------------------------------------------------
# the tables against the plan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", MFMA_ROWS, ids=_ids(MFMA_ROWS))
def test_row_reaches_the_arm_it_names(r):
    p = _plan(r)
    assert D.arm_of_plan(p, r.K, r.KS, r.mode) == r.arm, p
    for field, want in r.claims.items():
        assert want(p[field]) if callable(want) else p[field] == want, (field, p[field], getattr(want, "__doc__", want))
    if p["family"]:
        assert 0 < p["lds_bytes"] <= D.LDS_LIMIT
    if p["family"] == 1:
        assert p["ipw"] * p["wpc"] >= p["items_per_channel"] > p["ipw"] * (p["wpc"] - 1)
    if r.mode == 0 and r.variant != "bias_act":
        from ppeadepth import _abi
        assert _abi.lib.ppea_dwconv_lk_stats_partials(r.N, r.C, r.H, r.W, r.K, r.KS) == p["partials"]
    if r.arm is not None:
        assert D.elements(r) <= 8_000_000


def test_stats_rows_launch_what_plain_rows_launch():
    from ppeadepth import ops
    for r in MFMA_ROWS:
        if r.variant == "stats":
            assert _plan(r) == ops.dwconv_lk_plan(r.N, r.C, r.H, r.W, r.K, r.KS, r.mode, "plain")


def test_rows_reach_every_arm_that_exists():
    """"Exists" = some shape of the grid N 1..33 x C in {1, 3, 64, 512, 1024} x H 1..130 x W 1..260 launches it."""
    reachable, _, summaries = _sweep()
    table = {r.arm for r in MFMA_ROWS}
    assert table - {None} == reachable
    assert D.ALL_ARMS - reachable == set(D.UNREACHABLE)
    assert reachable <= D.ALL_ARMS and len(D.ALL_ARMS) == 99
    for s in summaries:
        assert s["max_lds_bytes"] <= D.LDS_LIMIT and s["bad_item_split"] == 0 and s["served"] > 0


def test_unreachable_window_sharing_data_gradient_is_an_lds_fact():
    """The reason behind the kernel's static_assert(!WS || MODE == 0), from the plan: where window sharing would apply (k = 31,
    pair, NSEG 5, H % 48 == 0) the data gradient's band is 32 on every grid shape, and the forward's is 48."""
    _, plans, _ = _sweep()
    dg = [p for K, KS, mode, p in plans if K == 31 and KS == 5 and mode == 1 and p["family"] == 1 and p["NSEG"] == 5]
    assert dg and all(p["WS"] == 0 for p in dg)
    assert {p["band"] for p in dg if p["multiband"]} == {32}
    fw = [p for K, KS, mode, p in plans if K == 31 and KS == 5 and mode == 0 and p["family"] == 1 and p["WS"]]
    assert fw and {p["band"] for p in fw} == {48}
    assert 2 * 78 * 288 * 4 == 179712 > D.LDS_LIMIT


def test_rows_reach_every_outcome_of_the_host_plans():
    """band, stacking, banding, staging, items per wave (row-band); gi, vector width, workgroups per channel (batch-major):
    the table meets every value the grid meets, and the values no grid shape meets are the listed ones."""
    _, plans, _ = _sweep()
    rows = [(r, _plan(r)) for r in MFMA_ROWS if r.arm is not None]
    for field, of_row in (("band", lambda p: p["band"]), ("stacked", lambda p: int(p["G"] > 1)), ("multiband", lambda p: int(p["bands"] > 1)),
                          ("fast", lambda p: p["fast"]), ("multi_item", lambda p: int(p["ipw"] > 1))):
        grid = {p[field] for _, _, _, p in plans if p["family"] == 1}
        assert {of_row(p) for _, p in rows if p["family"] == 1} == grid, field
    assert {p["band"] for _, _, _, p in plans if p["family"] == 1} == {32, 48} - set(D.UNREACHED_OUTCOMES["band"])
    for field, of_row in (("gi", lambda p: p["gi"]), ("VEC", lambda p: p["VEC"]), ("multi_wg", lambda p: int(p["wgpc"] > 1))):
        grid = {p[field] for _, _, _, p in plans if p["family"] == 2}
        assert {of_row(p) for _, p in rows if p["family"] == 2} == grid, field
    assert {p["gi"] for _, _, _, p in plans if p["family"] == 2} == {16, 12} - set(D.UNREACHED_OUTCOMES["gi"])
    # what the issue lists beyond single fields
    plans_of = lambda f: [r.name for r, p in rows if p["family"] == 1 and f(r, p)]      # noqa: E731
    assert plans_of(lambda r, p: p["G"] > 1 and r.N % p["G"])                           # ragged last group
    assert plans_of(lambda r, p: p["bands"] > 1 and r.H % p["band"])                    # ragged last band
    assert plans_of(lambda r, p: r.W % (16 * p["NSEG"]) and p["segs"] > 1)              # ragged last segment
    assert plans_of(lambda r, p: r.W % 16)                                              # ragged last tile
    assert plans_of(lambda r, p: r.W % 8 == 4) and plans_of(lambda r, p: r.W % 2 == 1)
    assert plans_of(lambda r, p: p["ipw"] > 1 and p["items_per_channel"] % p["ipw"] == 0)
    assert plans_of(lambda r, p: p["ipw"] > 1 and p["items_per_channel"] % p["ipw"] != 0)
    assert plans_of(lambda r, p: (r.C * p["wpc"]) % 4)                                  # an idle wave in the last workgroup
    assert plans_of(lambda r, p: p["WS"] and p["ipw"] > 1)
    bmr = [(r, p) for r, p in rows if p["family"] == 2]
    assert any(r.N < p["gi"] for r, p in bmr) and any(r.N > p["gi"] and r.N % p["gi"] for r, p in bmr)
    assert any(r.C % (4 * 6 // p["H"]) for r, p in bmr if p["H"] in (6, 12))           # C % CPW != 0


def test_filter_gradient_rows_meet_their_claims():
    from ppeadepth import ops
    for r, claims in D.FILTER_CASES:
        p = ops.dwconv_lk_bwd_filter_plan(r.N, r.C, r.H, r.W, r.K, r.KS)
        assert p is not None and p["lds_bytes"] <= 64 * 1024
        assert p["rounds"] == -(-p["rows_per_part"] // 4) and (p["parts"] - 1) * p["rows_per_part"] + p["last_rows"] == r.N * r.H
        for field, want in claims.items():
            if field == "ragged_part":
                assert p["parts"] > 1 and p["last_rows"] < p["rows_per_part"]
            elif field == "short_round":
                assert p["last_rows"] % 4 != 0 or p["rows_per_part"] % 4 != 0
            else:
                assert want(p[field]) if callable(want) else p[field] == want, (r.name, field, p)
    assert any(r.N * r.H < 4 for r, _ in D.FILTER_CASES) and any(r.W % 8 for r, _ in D.FILTER_CASES)
    assert any(r.W % 16 and r.W % 8 == 0 for r, _ in D.FILTER_CASES)
    assert ops.dwconv_lk_bwd_filter_plan(1, 1, 4, 5000, 31, 5) is None                 # W > 4096: not served


def test_fp32_vector_kernel_rows_pick_every_tile_that_can_be_picked():
    from ppeadepth import ops
    for fr in D.F32_CASES:
        r = fr.row
        got = ops.dwconv_lk_f32_plan(r.H, r.W, r.K) if r.KS in (0, 5) else -1
        assert got == fr.index, (r.name, got)
    reached = {(K, ops.dwconv_lk_f32_plan(H, W, K)) for K in D.KS_ALL for H in range(1, 131) for W in range(1, 261)}
    every = {(K, i) for K, n in D.F32_CONFIGS.items() for i in range(n)}
    assert every - reached == set(D.F32_UNREACHABLE)
    assert {(fr.row.K, fr.index) for fr in D.F32_CASES if fr.index >= 0} == reached
    assert ops.dwconv_lk_f32_plan(12, 40, 9) == -1
    assert {(fr.io, fr.row.mode) for fr in D.F32_CASES} == {("f32", 0), ("f32", 1), ("bf16", 0), ("bf16", 1)}


# ---------------------------------------------------------------------------------------------
# the bound: not too tight for a correct kernel, and the faults leave it
# ---------------------------------------------------------------------------------------------
def test_only_a_few_named_rows_keep_their_numerics_for_the_gpu():
    assert GPU_ONLY_NUMERICS == ["bm48_cpw2", "ws_ipw2"]


@pytest.mark.parametrize("r", NUMERIC_ROWS, ids=_ids(NUMERIC_ROWS))
def test_fp32_evaluation_stays_inside_the_bound_and_faults_leave_it(r):
    _, inp, ref = _numerics(r.name)
    for rounded in (False, True):
        got = D.evaluate(r, inp, round_bf16=rounded)
        for key, (ref_t, bound) in ref.items():
            ratio, outside = D.worst(got[key], ref_t, bound)
            assert outside == 0, (key, rounded, ratio)
    for fault in D.FAULTS:
        if not D.fault_applies(r, fault):
            continue
        got = D.evaluate(r, inp, fault=fault, round_bf16=True)
        outside = sum(D.worst(got[key], ref_t, bound)[1] for key, (ref_t, bound) in ref.items())
        assert outside > 0, fault


def test_filter_gradient_and_vector_kernel_references():
    """The filter-gradient reference is the correlation of x with the output gradient; an fp32 evaluation stays inside the
    fp32-output bound.  The fp32 vector kernel's rows take the same reference with the fp32-output bound."""
    r, _ = D.FILTER_CASES[0]
    inp = D.make_inputs(r)
    ref = D.reference_filter(r, inp)
    x, gb = inp["x"].double(), inp["gb"].double()
    P = r.K // 2
    xp = torch.nn.functional.pad(x, (P, P, P, P))
    want = torch.stack([torch.stack([(xp[:, :, ky:ky + r.H, kx:kx + r.W] * gb).sum((0, 2, 3)) for kx in range(r.K)], -1)
                        for ky in range(r.K)], -2)
    assert torch.allclose(ref["dw_big"][0], want, rtol=0, atol=1e-6 * float(want.abs().max()))
    got32 = torch.stack([torch.stack([(xp[:, :, ky:ky + r.H, kx:kx + r.W].float() * gb.float()).sum((0, 2, 3)) for kx in range(r.K)], -1)
                         for ky in range(r.K)], -2)
    assert D.worst(got32, *ref["dw_big"])[1] == 0
    fr = D.F32_CASES[0]
    inp = D.make_inputs(fr.row)
    for key, (ref_t, bound) in D.reference_f32(fr, inp).items():
        assert D.worst(D.evaluate(fr.row, inp)[key], ref_t, bound)[1] == 0
