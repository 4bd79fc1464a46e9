"""What tests/test_pw_arms_gpu.py relies on, proved without a device: every row of oracle/pw_inputs.py reaches the arm it
claims according to the library's own plan queries (ops.pwconv_plan / pwgrad_plan / pwgrad_pair_plan, the functions the launches
go by); the claimed arms are the whole census and every arm the dispatch picks with no switch set has a natural row; moving the
transposed-A decision into pw_choose changed no plan (a transcription of the rules as they stood, over a shape sweep); the split
plans keep their invariants; a correct kernel emulated in torch stays inside every bound and index faults do not; the guards
see an unwritten element and an overrun."""
import pytest
import torch
import torch.nn.functional as F

from oracle import pw_inputs as P

SWEEP = dict(Bmax=12, Mstep=8, nM=144, nK=36, nHW=960)       # B 1..12 x M 8..1152 x K 32..1152 x HW 8..7680, both A modes
WORST = {}


def _setenv(monkeypatch, env):
    for k in ("PPEA_PW_TILE", "PPEA_PW_V2", "PPEA_PWGRAD_V2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _ids(rows):
    return [r.name for r in rows]


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"PWARM-CPU {family}: worst err / bound of the emulation {ratio:.3f} (so far {WORST[family]:.3f})")


def _family(c):
    v, ta = c.claims["family"]
    return f"pwconv v{v} {'transposed' if ta else 'row-major'}"


# ---------------------------------------------------------------------------------------------
# plan reach and census
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.pw_cases(), ids=_ids(P.pw_cases()))
def test_every_pwconv_row_reaches_the_arm_it_claims(monkeypatch, c):
    from ppeadepth import _abi, ops
    _setenv(monkeypatch, c.env)
    p = ops.pwconv_plan(c.B, c.M, c.K, c.HW, c.ta)
    assert p is not None
    assert (p["version"], int(c.ta)) == c.claims["family"], p
    if c.arm is not None:
        assert P.arm_of_plan(p, c.ta, c.epi) == c.arm, p
    if "steps" in c.claims:
        assert -(-c.K // p["BK"]) == c.claims["steps"]
    if "total" in c.claims:
        assert p["grid_x"] * p["grid_y"] * p["grid_z"] == c.claims["total"], p
    nb = -(-c.HW // 128)
    assert p["partials"] == c.B * nb * p["WN"] and p["WN"] == (4 if p["BM"] == 32 else 2)
    if not c.ta:
        assert _abi.lib.ppea_pwconv_stats_partials(c.B, c.M, c.K, c.HW) == p["partials"]
    if p["version"] == 2:
        assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (nb * -(-c.M // p["BM"]) * c.B, 1, 1) and c.K % p["BK"] == 0
    else:
        assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (nb, -(-c.M // p["BM"]), c.B)
    if c.epi == 5:
        assert p["version"] == 2                              # ppea_pwconv_infer_bf16 serves the LDS-DMA kernel only
    if c.epi == 4:
        assert c.bias in (None, "f32") and not c.ta
    if c.epi == 2:
        assert c.bias is None


def test_unsupported_shapes_have_no_plan(monkeypatch):
    from ppeadepth import ops
    _setenv(monkeypatch, {})
    for c in P.UNSUPPORTED_PW:
        assert ops.pwconv_plan(c.B, c.M, c.K, c.HW, c.ta) is None, c.name
    assert ops.pwconv_plan(1, 12, 32, 64, False) is not None            # M % 8 matters to the transposed matrix only
    assert ops.pwconv_plan(65536, 8, 32, 8) is None and ops.pwconv_plan(65535, 8, 32, 8) is not None
    assert ops.pwconv_plan(0, 8, 32, 8) is None and ops.pwgrad_plan(1, 8, 8, 12) is None
    assert ops.pwgrad_pair_plan(1, (8, 8), (8, 8), 40) is None and ops.pwgrad_pair_plan(1, (8, 0), (8, 8), 64) is None


def _parent_rules(B, M, K, HW, ta):
    """The dispatch as it stood before the transposed-A decision moved into pw_choose (pw_choose + launch_pw of the parent
    commit, no hook set), vectorised -> the sweep's packed key."""
    nb = (HW + 127) // 128
    b128, b64 = nb * ((M + 127) // 128) * B, nb * ((M + 63) // 64) * B
    w = torch.where
    c = lambda v: torch.full_like(M, v)                                            # noqa: E731
    # pw_choose, the v1 tile
    bm1 = w((M >= 128) & (b128 >= 512), c(128), w((M > 32) & (b64 >= 256), c(64), c(32)))
    bk1 = w((bm1 != 128) & (K >= 512), c(64), c(32))
    if not ta:
        # pw_choose, the v2 tile: taken whenever K % BK == 0
        first, second = (M >= 128) & (b128 >= 256), (M > 32) & (b64 >= 256)
        bm2 = w(first, c(128), w(second, c(64), w(K % 64 == 0, c(32), c(64))))
        bk2 = w(first, c(32), w(second, w((K >= 512) & (K % 64 == 0), c(64), c(32)), w(K % 64 == 0, c(64), c(32))))
        v2 = (K % bk2) == 0
        bm, bk = w(v2, bm2, bm1), w(v2, bk2, bk1)
    else:
        # launch_pw<., true>: the ring where M >= 128, >= 128 tiles of 128 rows, M % 8 == 0, K % 32 == 0; else v1's tile
        v2 = (M >= 128) & (b128 >= 128) & (M % 8 == 0) & (K % 32 == 0)
        bm, bk = w(v2, c(128), bm1), w(v2, c(32), bk1)
    key = v2.to(M.dtype) + 2 * w(bm == 128, c(2), w(bm == 64, c(1), c(0))) + 8 * (bk == 64).to(M.dtype)
    served = (K % 32 == 0) & (HW % 8 == 0) & (M % 8 == 0 if ta else torch.ones_like(v2))
    return w(served, key, c(255)).to(torch.uint8)


@pytest.fixture(scope="module")
def sweep():
    """ops.pwconv_plan_sweep over SWEEP with no hook set -> {ta: (set of keys met, shapes whose plan differs from the
    transcription, partials mismatches)}."""
    import os
    from ppeadepth import ops
    saved = {k: os.environ.pop(k) for k in ("PPEA_PW_TILE", "PPEA_PW_V2") if k in os.environ}
    try:
        S = SWEEP
        M = (S["Mstep"] * torch.arange(1, S["nM"] + 1, dtype=torch.int32)).view(-1, 1, 1)
        K = (32 * torch.arange(1, S["nK"] + 1, dtype=torch.int32)).view(1, -1, 1)
        HW = (8 * torch.arange(1, S["nHW"] + 1, dtype=torch.int32)).view(1, 1, -1)
        M, K, HW = torch.broadcast_tensors(M, K, HW)
        res = {}
        for ta in (False, True):
            keys, differ, mismatch = set(), 0, 0
            for B in range(1, S["Bmax"] + 1):
                got, summ = ops.pwconv_plan_sweep(B, ta, S["Mstep"], S["nM"], S["nK"], S["nHW"])
                differ += int((got != _parent_rules(B, M, K, HW, ta)).sum())
                mismatch += summ["partials_mismatch"]
                assert summ["served"] == got.numel()
                keys |= set(int(k) for k in got.unique())
            res[ta] = (keys, differ, mismatch)
        return res
    finally:
        os.environ.update(saved)


def test_dispatch_refactor_changed_no_plan_and_the_partial_count_is_the_plans(sweep):
    for ta in (False, True):
        keys, differ, mismatch = sweep[ta]
        assert differ == 0 and mismatch == 0, (ta, differ, mismatch)
        assert 255 not in keys


def test_census_is_covered_and_every_natural_arm_has_a_natural_row(sweep):
    rows = P.pw_cases()
    claimed = {c.arm for c in rows if c.arm is not None}
    assert claimed == P.ALL_PW_ARMS, (claimed ^ P.ALL_PW_ARMS)
    natural = set()
    for ta in (False, True):
        for key in sweep[ta][0]:
            a = P.arm_of_key(key, ta, 0)
            epis = P.epis_of(ta) if a[0] == 2 else ((0, 1, 2) if ta else (0, 1, 2, 4))
            natural |= {P.arm_of_key(key, ta, e) for e in epis}
    assert natural <= P.ALL_PW_ARMS
    with_natural_row = {c.arm for c in rows if c.arm is not None and not c.env}
    assert natural <= with_natural_row, sorted(natural - with_natural_row)
    hook_only = P.ALL_PW_ARMS - natural
    print("PWARM-CPU natural arms (version, transposed, BM, BK):", sorted({a[:4] for a in natural}))
    print("PWARM-CPU hook-only arms (version, transposed, BM, BK):", sorted({a[:4] for a in hook_only}))
    # as the dispatch reads today: v2 128/64, all of row-major v1, v1 transposed 128/32
    assert {a[:4] for a in hook_only} == {(2, 0, 128, 64), (1, 1, 128, 32)} | {(1, 0, bm, bk) for bm, bk in P.V1_TILES}
    assert all(not c.env for c in rows if c.arm in natural and c in P.TILE_CASES)


# ---------------------------------------------------------------------------------------------
# pwgrad plans
# ---------------------------------------------------------------------------------------------
def _cut_kinds(p):
    cuts = [s * p["steps_per_split"] for s in range(1, p["S"])]
    return {("image" if c % p["steps_per_image"] == 0 else "inside") for c in cuts}


def _check_claims(p, claims):
    assert p["step"] == claims["step"], p
    if "S" in claims:
        assert p["S"] == claims["S"], p
    if claims.get("short"):
        assert p["total_steps"] % p["steps_per_split"] != 0, p
    if "cut" in claims:
        assert claims["cut"] in _cut_kinds(p), p


@pytest.mark.parametrize("c", P.PWGRAD_CASES, ids=_ids(P.PWGRAD_CASES))
def test_every_pwgrad_row_reaches_the_plan_it_claims(monkeypatch, c):
    from ppeadepth import ops
    _setenv(monkeypatch, c.env)
    _check_claims(ops.pwgrad_plan(c.B, c.M, c.N, c.H * c.W), c.claims)


@pytest.mark.parametrize("c", P.INTO_CASES, ids=_ids(P.INTO_CASES))
def test_every_pwgrad_into_row_reaches_the_plan_it_claims(monkeypatch, c):
    from ppeadepth import ops
    _setenv(monkeypatch, c.env)
    _check_claims(ops.pwgrad_plan(c.B, c.taps * c.Ch, c.N, c.H * c.W), c.claims)
    r0, rn = P.bias_window(c)
    assert 0 <= r0 and rn >= 1 and r0 + rn <= c.taps * c.Ch


def test_pwgrad_tables_cover_what_the_issue_lists():
    rows = P.PWGRAD_CASES
    assert {c.claims["step"] for c in rows} == {0, 32}
    assert {c.H * c.W for c in rows if c.claims["step"] == 0 and not c.env} >= {8, 24, 40, 72}
    assert any(c.env and c.claims["step"] == 0 and (c.H * c.W) % 32 == 0 for c in rows)
    assert {1, 2, 3, 34, 130, 514} <= {c.M for c in rows} and {1, 2, 3, 34, 130, 514} <= {c.N for c in rows}
    assert any(c.rowsum and c.N > 128 for c in rows) and any(not c.rowsum for c in rows)
    assert any(c.claims.get("S") == 1 for c in rows) and any(c.claims.get("short") for c in rows)
    assert {c.claims.get("cut") for c in rows} >= {"inside", "image"}
    into = P.INTO_CASES
    assert {(c.wdt, c.taps) for c in into} == {("f32", 1), ("bf16", 1), ("f32", 9), ("bf16", 9)}
    assert {c.bdt for c in into} == {None, "f32", "bf16"} and {c.bwin for c in into if c.bdt} == {"all", "centre", "one", "end"}
    assert any(c.taps == 9 and c.bwin == "centre" and P.bias_window(c) == (4 * c.Ch, c.Ch) for c in into)
    assert any(P.bias_window(c)[0] + P.bias_window(c)[1] == c.taps * c.Ch and c.bwin == "end" for c in into)
    assert {(b, ch, h, w) for (_n, b, ch, h, w, _b) in P.TAPSUM_CASES} == {(1, 1, 1, 4), (2, 3, 2, 4), (1, 2, 5, 8), (3, 5, 3, 12), (2, 32, 6, 20)}


@pytest.mark.parametrize("row", P.PAIR_CASES, ids=[r[0] for r in P.PAIR_CASES])
def test_every_pair_row_is_served_as_it_claims(monkeypatch, row):
    from ppeadepth import _abi, ops
    name, a, b, env, served = row
    _setenv(monkeypatch, env)
    assert (a.B, a.H, a.W) == (b.B, b.H, b.W)
    Ms, Ns = (a.taps * a.Ch, b.taps * b.Ch), (a.N, b.N)
    p = ops.pwgrad_pair_plan(a.B, Ms, Ns, a.H * a.W)
    assert (p is not None) == served
    import ctypes
    nbytes = _abi.lib.ppea_pwgrad_pair_workspace_bytes(a.B, (ctypes.c_int * 2)(*Ms), (ctypes.c_int * 2)(*Ns), a.H * a.W)
    assert (nbytes > 0) == served
    if served:
        assert p["workspace_bytes"] == nbytes and p["step"] == 32
    tiles = lambda c: -(-c.taps * c.Ch // 128) * -(-c.N // 128)                     # noqa: E731
    if name == "pair_many_one":
        assert tiles(a) > 1 and tiles(b) == 1 and (p["tiles_m"], p["tiles_n"]) == (tiles(a), 1)
    if name == "pair_one_many":
        assert tiles(a) == 1 and tiles(b) > 1 and (p["tiles_m"], p["tiles_n"]) == (1, tiles(b))


def test_pwgrad_plan_invariants_over_a_sweep(monkeypatch):
    from ppeadepth import _abi, ops
    import ctypes
    i2 = ctypes.c_int * 2
    widths = (1, 2, 3, 34, 130, 514, 1152)
    seen_S = set()
    for env in ({}, {"PPEA_PWGRAD_V2": "0"}):
        _setenv(monkeypatch, env)
        for B in (1, 2, 3, 5, 8, 12):
            for HW in list(range(8, 2049, 8)) + [7680]:
                for M in widths:
                    for N in (1, 34, 130, 514):
                        p = ops.pwgrad_plan(B, M, N, HW)
                        v2 = not env and HW % 32 == 0
                        tk = 32 if v2 else 64
                        assert p["step"] == (32 if v2 else 0) and p["steps_per_image"] == -(-HW // tk)
                        assert p["total_steps"] == B * p["steps_per_image"] and p["S"] >= 1
                        assert p["S"] * p["steps_per_split"] >= p["total_steps"] > (p["S"] - 1) * p["steps_per_split"]
                        assert (p["tiles_m"], p["tiles_n"]) == (-(-M // 128), -(-N // 128))
                        assert p["workspace_bytes"] == p["S"] * (M * N + M) * 4 == _abi.lib.ppea_pwgrad_workspace_bytes(B, M, N, HW)
                        seen_S.add(p["S"])
                    if M > 130:
                        continue
                    Ms, Ns = (M, 130), (34, M)
                    pp = ops.pwgrad_pair_plan(B, Ms, Ns, HW)
                    nbytes = _abi.lib.ppea_pwgrad_pair_workspace_bytes(B, i2(*Ms), i2(*Ns), HW)
                    assert (pp is not None) == v2 == (nbytes > 0)
                    if pp is not None:
                        assert pp["S"] >= 1 and pp["S"] * pp["steps_per_split"] >= pp["total_steps"] > (pp["S"] - 1) * pp["steps_per_split"]
                        assert pp["workspace_bytes"] == nbytes == pp["S"] * ((Ms[0] * Ns[0] + Ms[0]) + (Ms[1] * Ns[1] + Ms[1])) * 4
                        assert pp["total_steps"] == B * HW // 32
    assert 1 in seen_S and max(seen_S) >= 64
    _setenv(monkeypatch, {})
    # grid limits: 65535 tiles along an axis are launched, 65536 are refused (the entry point returns PPEA_ERR_UNSUPPORTED)
    assert ops.pwgrad_plan(1, 128 * 65535, 1, 8)["tiles_m"] == 65535 and ops.pwgrad_plan(1, 128 * 65535 + 1, 1, 8) is None
    assert ops.pwgrad_plan(1, 1, 128 * 65535 + 1, 8) is None
    assert ops.pwgrad_pair_plan(1, (128 * 65535, 1), (1, 1), 32) is None            # 65536 tiles on the pair's y axis
    assert ops.pwgrad_pair_plan(1, (128 * 65534, 1), (1, 1), 32)["tiles_m"] == 65534


# ---------------------------------------------------------------------------------------------
# references, bounds, emulation
# ---------------------------------------------------------------------------------------------
def test_einsum_reference_equals_conv2d_in_double():
    c = P.EDGE_CASES[4]
    inp = P.make_pw_inputs(c)
    ref = P.pw_reference(c, inp)["y"][0]
    want = F.conv2d(inp["x"].double(), inp["a"].double().view(c.M, c.K, 1, 1), inp["bias"].double())
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(inp["a_arg"], inp["a"]) and inp["x"].dtype == torch.bfloat16
    ct = next(r for r in P.EDGE_CASES if r.ta)
    it = P.make_pw_inputs(ct)
    assert torch.equal(it["a_arg"], it["a"].t()) and it["a_arg"].is_contiguous() and tuple(it["a_arg"].shape) == (ct.K, ct.M)
    aux = P.make_pw_inputs(next(r for r in P.EDGE_CASES if r.epi == 2))["aux"].float()
    assert float(aux.abs().max()) == P.DGELU_RANGE and float((aux.abs() >= 5).float().mean()) > 0.05        # the tails are there


def test_activation_terms_are_the_measured_ones():
    """The measurement the docstring of oracle/pw_inputs.py records: torch's float32 evaluation of the kernels' two formulas
    against float64 over every bf16 value of the range, times the margin of 4."""
    b = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    x = b[torch.isfinite(b) & (b.abs() <= P.GELU_RANGE) & (b != 0)]
    g = float(((P._gelu32(x).double() - P.gelu64(x.double())).abs() / x.double().abs()).max())
    x = x[x.abs() <= P.DGELU_RANGE]
    d = float((P._dgelu32(x).double() - P.dgelu64(x.double())).abs().max())
    print(f"PWARM-CPU activation terms: GELU {g:.3e} per |x| on 0 < |x| <= {P.GELU_RANGE}, GELU' {d:.3e} on |x| <= {P.DGELU_RANGE}; margin 4")
    assert g <= P.G_GELU / 4 * 1.001 and d <= P.D_DGELU / 4 * 1.001
    assert P.G_GELU / 4 <= 1.5 * g and P.D_DGELU / 4 <= 1.5 * d             # and not padded
    xs = torch.tensor([0.25, 1.0, 4.0], dtype=torch.float64)
    assert bool((P.G_GELU * xs <= 2e-4 * P.U_BF16 * P.gelu64(xs).abs()).all())    # small against 2^-8 |ref| where GELU is not


def _hold_emulation(family, got, ref):
    worst_ratio = 0.0
    for key, (r, bound) in ref.items():
        ratio, outside = P.worst(got[key], r, bound)
        assert outside == 0, (family, key, ratio, outside)
        worst_ratio = max(worst_ratio, ratio)
    _note(family, worst_ratio)


def _emulated(monkeypatch, c, fault=None):
    from ppeadepth import ops
    _setenv(monkeypatch, c.env)
    p = ops.pwconv_plan(c.B, c.M, c.K, c.HW, c.ta)
    inp = P.make_pw_inputs(c)
    return inp, p, P.emulate_pw(c, inp, p["WN"], fault)


@pytest.mark.parametrize("c", [r for r in P.pw_cases() if r.epi != 5], ids=_ids([r for r in P.pw_cases() if r.epi != 5]))
def test_emulated_pwconv_kernel_stays_inside_every_bound(monkeypatch, c):
    inp, p, got = _emulated(monkeypatch, c)
    ref = P.pw_reference(c, inp, got["y"])
    _hold_emulation(_family(c), got, ref)
    assert (c.epi == 1) == ("y2" in ref)
    if c.epi == 4:
        assert got["sums"].shape == (c.M, p["partials"], 2)
        r1, r2, outside = P.stats_check(got["y"], got["sums"], p["WN"])
        _note("pwconv statistics", max(r1, r2))
        assert outside == 0


@pytest.mark.parametrize("c", [r for r in P.pw_cases() if r.epi == 5], ids=_ids([r for r in P.pw_cases() if r.epi == 5]))
def test_emulated_inference_epilogue_stays_inside_the_shared_bound(c):
    inp = P.make_pw_inputs(c)
    acc, _ = P._acc_and_mag(inp)
    ref, ref2 = P.infer_reference(acc, inp["s"], inp["o"], inp["act"], inp["r1"], inp["r2"], inp["r2_scale"], inp["s2"], inp["o2"])
    t = inp["s"].view(1, -1, 1, 1) * acc.float() + inp["o"].view(1, -1, 1, 1)
    t = torch.relu(t) if inp["act"] == 1 else (P._gelu32(t) if inp["act"] == 2 else t)
    y = (t + inp["r1"].float() + inp["r2_scale"] * inp["r2"].float()).bfloat16()
    y2 = (inp["s2"].view(1, -1, 1, 1) * y.float() + inp["o2"].view(1, -1, 1, 1)).bfloat16()
    assert float((y.double() - ref).abs().max()) <= P.INFER_TOL * float(ref.abs().max())
    assert float((y2.double() - ref2).abs().max()) <= P.INFER_TOL * float(ref2.abs().max())


FAULT_ROWS = ("v2_gelu_m65", "v1_gelu_m65", "v2t_hw136", "v1t_m24_hw192")


@pytest.mark.parametrize("name", FAULT_ROWS)
@pytest.mark.parametrize("fault", ("drop_kstep", "swap_chunk", "row_above", "drop_bias"))
def test_pwconv_bound_catches_index_faults(monkeypatch, name, fault):
    c = next(r for r in P.pw_cases() if r.name == name)
    assert c.bias is not None and c.M > 16 and c.HW >= 16 and c.K >= 64
    inp, p, got = _emulated(monkeypatch, c, fault)
    ref, bound = P.pw_reference(c, inp)["y"]
    ratio, outside = P.worst(got["y"], ref, bound)
    assert outside >= 1, (name, fault, ratio)
    assert {r.claims["family"] for r in P.pw_cases() if r.name in FAULT_ROWS} == {(1, 0), (1, 1), (2, 0), (2, 1)}


@pytest.mark.parametrize("c", P.PWGRAD_CASES, ids=_ids(P.PWGRAD_CASES))
def test_emulated_pwgrad_stays_inside_every_bound(monkeypatch, c):
    from ppeadepth import ops
    _setenv(monkeypatch, c.env)
    p = ops.pwgrad_plan(c.B, c.M, c.N, c.H * c.W)
    inp = P.make_pwgrad_inputs(c)
    w, r = P.emulate_pwgrad(inp["p"], inp["q"], p)
    _hold_emulation("pwgrad", dict(w=w, rowsum=r), P.pwgrad_reference(inp["p"], inp["q"]))
    if p["S"] > 1:
        w, r = P.emulate_pwgrad(inp["p"], inp["q"], p, "drop_split")
        ref = P.pwgrad_reference(inp["p"], inp["q"])
        assert P.worst(w, *ref["w"])[1] >= 1 and P.worst(r, *ref["rowsum"])[1] >= 1


@pytest.mark.parametrize("c", P.INTO_CASES + tuple(x for row in P.PAIR_CASES for x in row[1:3]),
                         ids=_ids(P.INTO_CASES) + [f"{row[0]}_{x.name}" for row in P.PAIR_CASES for x in row[1:3]])
def test_emulated_pwgrad_into_stays_inside_every_bound_and_faults_do_not(monkeypatch, c):
    from ppeadepth import ops
    _setenv(monkeypatch, c.env)
    p = ops.pwgrad_plan(c.B, c.taps * c.Ch, c.N, c.H * c.W)
    inp = P.make_into_inputs(c)
    ref = P.into_reference(c, inp)
    assert tuple(ref["dw"][0].shape) == ((c.Ch, c.N, 3, 3) if c.taps == 9 else (c.Ch, c.N)) and ("db" in ref) == (c.bdt is not None)
    _hold_emulation("pwgrad into", P.emulate_into(c, inp, p), ref)
    if c.taps == 9 and c.N > 1:
        assert P.worst(P.emulate_into(c, inp, p, "scatter_tn")["dw"], *ref["dw"])[1] >= 1
    if c.bdt is not None and c.taps * c.Ch > 1:
        assert P.worst(P.emulate_into(c, inp, p, "window_shift")["db"], *ref["db"])[1] >= 1
    if p["S"] > 1:
        assert P.worst(P.emulate_into(c, inp, p, "drop_split")["dw"], *ref["dw"])[1] >= 1


@pytest.mark.parametrize("c", P.TAPSUM_CASES, ids=_ids(P.TAPSUM_CASES))
def test_emulated_tapsum_stays_inside_every_bound_and_a_column_fault_does_not(c):
    inp = P.make_tapsum_inputs(c)
    got = P.emulate_tapsum(c, inp)
    _hold_emulation("tapsum", got, P.tapsum_reference(c, inp, got["pre"]))
    bad = P.emulate_tapsum(c, inp, "col_inside")
    assert P.worst(bad["pre"], *P.tapsum_reference(c, inp)["pre"])[1] >= 1
    # the gather equals the adjoint of the tap sum: <tapsum(T), g> == <T, shift_taps(g)> in double
    pre64 = P.tapsum_reference(c._replace(bias=None), dict(inp, bias=None))["pre"][0]
    lhs, rhs = float((pre64 * inp["g"].double()).sum()), float((inp["T"].double() * P.shift_taps(inp["g"]).double()).sum())
    assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), 1.0)


def test_guards_detect_an_unwritten_element_and_an_overrun():
    for dtype in (torch.bfloat16, torch.float32):
        buf, t = P.guarded((3, 5, 8), dtype, "cpu")
        assert bool(torch.isnan(t).all()) and P.guards_intact(buf, dtype) and buf.numel() == t.numel() + 2 * P.GUARD
        ref = torch.ones(3, 5, 8, dtype=torch.float64)
        t.fill_(1.0)
        assert P.worst(t, ref, torch.full_like(ref, 1e-3)) == (0.0, 0) and P.guards_intact(buf, dtype)
        t.view(-1)[17] = float("nan")                                               # never stored
        ratio, outside = P.worst(t, ref, torch.full_like(ref, 1e-3))
        assert outside == 1 and ratio == float("inf")
        buf.view(dtype)[P.GUARD + t.numel()] = 1.0                                  # one element past the end
        assert not P.guards_intact(buf, dtype)
        buf, t = P.guarded((4,), dtype, "cpu")
        buf.view(dtype)[P.GUARD - 1] = 0.0                                          # one before the start
        assert not P.guards_intact(buf, dtype)
