"""CPU proofs behind tests/test_cv_arms_gpu.py: the float64 plane-sweep reference of oracle/cv_inputs.py agrees with the
project's CPU composite and the recorded goldens, the table names all 16 instantiations of cost_volume_fwd<F, DB, PK, RING> and
every bin tail, the exact rows are exact and sit on all four edge-mask boundaries, the share of undecided and left-out entries
stays under the cap, the fp32 emulation of the kernel is inside the per-element bound on every row, twelve synthetic kernel
faults leave it on every row where they apply, and no sample of any row or of a pose sweep reaches the kernel's
last-column / last-row branch."""
import functools

import pytest
import torch

from conftest import rel_err
from oracle import cv_inputs as V

FWD_TOL = 2e-5      # the project's fp32 forward bound against the reference (tests/test_kernels_gpu.py)
ROWS = V.ROWS
EXACT = [r for r in ROWS if r.opts.get("exact")]
# maps whose interior (h - 4)(w - 4) is under a fifth of the map cannot have a non-zero share of 0.2: held by their interior
NARROW = [r for r in ROWS if (r.h - 4) * (r.w - 4) < 0.25 * r.h * r.w]


def _ids(rows):
    return [r.name for r in rows]


@functools.lru_cache(maxsize=None)
def _numerics(name):
    r = V.BY_NAME[name]
    inp = V.make_inputs(r)
    return r, inp, V.reference(r, inp)


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
def test_reference_is_the_cpu_composite_and_the_goldens(golden):
    """Measured: single frame vs composite 1.6e-06, vs golden 1.6e-06; three frames vs composite 1.2e-06, vs golden 1.5e-06."""
    from ppeadepth.inference import cost_volume_cpu, cost_volume_reduce_cpu
    for name in ("cost_volume", "cost_volume_multi"):
        g = golden(name)
        r, inp = V.from_tensors(name, g["cur"], g["lookup"], g["poses"], g["K"], g["inv_K"], g["bins"])
        ref = V.reference(r, inp)
        cost = ref.cost.reshape(r.B, r.D, r.h, r.w)
        comp = cost_volume_cpu(g["cur"], g["lookup"], g["poses"], g["K"], g["inv_K"], g["bins"])
        e_comp = rel_err(comp, cost)
        assert torch.equal(comp == 0, cost == 0)
        masked, conf, _idx, low = cost_volume_reduce_cpu(cost.float(), g["bins"])
        assert torch.equal(conf, g["confidence"])
        e_gold = rel_err(masked, g["cost"] * g["confidence"].unsqueeze(1))
        keep = ~g["near_tie"] if "near_tie" in g else torch.ones_like(conf, dtype=torch.bool)
        e_low = rel_err(low[keep], g["lowest_cost"][keep])
        print(f"float64 reference on {name}: vs CPU composite {e_comp:.3e}, vs golden {e_gold:.3e}, lowest cost {e_low:.3e}")
        assert e_comp < FWD_TOL and e_gold < FWD_TOL and e_low < FWD_TOL
        assert float(cost[2].abs().max()) == 0.0                         # item 2: every pose zeroed


def test_reference_bilinear_is_grid_sample():
    """The written-out zero-fill bilinear sample against F.grid_sample in double, positions on and off the map."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    h, w = 7, 9
    maps = torch.randn(3, h, w, generator=g, dtype=torch.float64)
    ix = torch.rand(4, h * w, generator=g, dtype=torch.float64) * (w + 3) - 2
    iy = torch.rand(4, h * w, generator=g, dtype=torch.float64) * (h + 3) - 2
    ix[0, :w], iy[0, :w] = torch.arange(w, dtype=torch.float64), float(h - 1)        # on the last row, on texels
    got, _, _ = V._bilinear64(maps, ix, iy, h, w)
    grid = torch.stack([ix / (w - 1) * 2 - 1, iy / (h - 1) * 2 - 1], -1).reshape(4, h * w, 1, 2)
    want = F.grid_sample(maps[None].expand(4, 3, h, w), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    assert float((got - want[..., 0].permute(1, 0, 2)).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
def test_table_names_every_instantiation_and_bin_tail():
    assert {V.instantiation(r) for r in ROWS} == V.ALL_INSTANTIATIONS and len(V.ALL_INSTANTIATIONS) == 16
    for inst in V.ALL_INSTANTIATIONS:                                    # a generic row each
        assert any(V.instantiation(r) == inst and r.name.startswith("gen_") for r in ROWS), inst
    for F, Ds in V.REQUIRED_TAILS.items():
        have = {r.D for r in ROWS if r.F == F}
        assert set(Ds) <= have, (F, Ds, have)
        tails = {min(V.DB_OF[F], r.D - (r.D - 1) // V.DB_OF[F] * V.DB_OF[F]) for r in ROWS if r.F == F}
        assert tails == set(range(1, V.DB_OF[F] + 1)), (F, tails)
    assert any(r.F == 1 and r.D < 4 for r in ROWS) and any(r.F == 2 and r.D == 1 for r in ROWS)              # D < DB
    shapes = {(r.h, r.w) for r in ROWS}
    assert {(5, 5), (5, 37), (21, 5)} <= shapes
    assert any(r.h * r.w < 256 and min(r.h, r.w) > 5 for r in ROWS)
    assert any(256 < r.h * r.w < 272 for r in ROWS)
    assert {1, 3} <= {r.C for r in ROWS if r.dtype == "f32"} and {2, 30} <= {r.C for r in ROWS if r.dtype == "bf16"}
    ring = [r for r in ROWS if r.form == "ring"]
    assert {-1, V.INT32_MAX} <= {r.opts["head"] for r in ring} and {0, 2} <= {r.opts["head"] - r.F for r in ring}
    seen = [(s, r.F) for r in ROWS if r.form == "ring" for s in r.opts["seen"]]
    assert any(s == 0 for s, _ in seen) and any(s < 0 for s, _ in seen) and any(s > F for s, F in seen)
    assert any(r.opts.get("skipnull") for r in ROWS) and any(r.form == "ring" and r.opts.get("skip") for r in ROWS)
    for r in ROWS:
        assert r.B <= 4 and r.C <= 32 and r.h <= 21 and r.w <= 37 and r.D <= 13, r.name
        assert r.what


def test_skip_rows_are_what_they_say():
    r, inp, ref = _numerics("skip_all_frames")
    assert inp["skip"][1].tolist() == [1, 1, 1] and float(ref.cost[1].abs().max()) == 0.0 and float(ref.cost[0].max()) > 0
    r, inp, ref = _numerics("skip_each_in_turn")
    assert [inp["skip"][b].tolist() for b in range(3)] == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    r, inp, ref = _numerics("skip_off_the_map")                          # frames in use that contribute nowhere
    for b, f in r.opts["off"]:
        assert int(inp["skip"][b, f]) == 0 and not bool(ref.edge[b, f].any())
    n = ref.edge.sum(1)
    assert bool((n[0] == 2).any()) and bool((n[1] == 1).any())             # the divisor is the other frames'
    r, inp, ref = _numerics("equal_frames")                              # two equal frames: the single-frame cost
    assert torch.equal(ref.diff[0, 0], ref.diff[0, 1]) and torch.equal(ref.edge[0, 0], ref.edge[0, 1])
    single = torch.where(ref.edge[0, 0], ref.diff[0, 0], torch.zeros_like(ref.diff[0, 0]))
    single = single / ((single > 0).double() + V.EPS7)
    assert float(single.max()) > 0 and float((ref.cost[0] - single).abs().max()) <= 1e-7 * float(single.max())
    r, inp, ref = _numerics("behind_camera")
    assert V.no_degenerate_depth(r, inp)
    behind = [bool((ref.pos[(b, f)]["iz"].v < 0).any()) for b in range(r.B) for f in range(r.F)]
    assert all(behind) and any(bool((ref.pos[k]["iz"].v < 0)[ref.edge[k[0], k[1]]].any()) for k in ref.pos)
    for row in ROWS:
        assert V.no_degenerate_depth(row, _numerics(row.name)[1]), row.name
    for name in ("ring_skip_null", "ring_skip_array"):
        r, inp, ref = _numerics(name)
        assert (inp["skip_arg"] is None) == (name == "ring_skip_null")
    assert _numerics("ring_skip_array")[1]["skip"].tolist() == [[0, 1], [0, 1]]
    assert _numerics("ring_skip_null")[1]["skip"].tolist() == [[0, 0], [0, 1]]
    r, inp, ref = _numerics("ring_seen_edges")
    assert inp["skip"].tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 0], [0, 1, 1]]


# ---------------------------------------------------------------------------------------------
# exact rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", EXACT, ids=_ids(EXACT))
def test_exact_rows_are_exact_and_on_the_boundaries(r):
    """Every fp32 intermediate equals the double chain's; no entry is undecided or left out; the integer rows hit each of the
    four mask boundaries at interior pixels (measured: x = 31 at 13 and y = 15 at 29 interior pixels of every bin for the
    translation (+2, +1), x = 2 and y = 2 likewise for (-2, -1)); the half-pixel row's weights are 0.25 and 0.5."""
    _, inp, ref = _numerics(r.name)
    assert r.eps == 0.0 and V.exact_positions_hold(r, inp)
    assert ref.n_undecided == 0 and ref.n_left_out == 0 and not bool(ref.undecided.any())
    hits = V.boundary_hits(r, ref)
    print(f"{r.name}: boundary hits per bin {hits}")
    if r.name == "exact_half":
        for b, want in ((0, {0.25}), (1, {0.5})):
            for f in range(r.F):
                p = ref.pos[(b, f)]
                tx, ty = p["ix"].v - torch.floor(p["ix"].v), p["iy"].v - torch.floor(p["iy"].v)
                ws = torch.stack([(1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty])
                assert set(ws[ws > 0].unique().tolist()) == want, (b, f)
        return
    for key, v in hits.items():
        assert max(v) > 0, key                                          # at an interior pixel, for at least one bin
    for p in ref.pos.values():
        for q in ("xv", "yv", "ix", "iy"):
            assert bool((p[q].v == p[q].v.round()).all())


# ---------------------------------------------------------------------------------------------
# cap, emulation, faults
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", ROWS, ids=_ids(ROWS))
def test_cap_and_non_zero_share(r):
    """Undecided + left-out entries <= 2 % of the row (from the reference alone); a non-zero share above 0.2 in some item."""
    _, inp, ref = _numerics(r.name)
    n = r.B * r.D * r.h * r.w
    print(f"CVCAP {r.name}: undecided {ref.n_undecided} + left out {ref.n_left_out} of {n} (cap {V.CAP:.0%})")
    assert ref.n_undecided + ref.n_left_out <= V.CAP * n
    nz = (ref.cost != 0).double()
    if r in NARROW:
        inner = V.inner_mask(r)
        assert max(float(nz[b][:, inner].mean()) for b in range(r.B)) > 0.5
    elif not r.opts.get("exact"):
        assert max(float(nz[b].mean()) for b in range(r.B)) > 0.2
    assert ref.mean_cost > 0.5 and bool(torch.isfinite(ref.cost).all())


@pytest.mark.parametrize("r", ROWS, ids=_ids(ROWS))
def test_emulation_is_inside_the_bound(r):
    _, inp, ref = _numerics(r.name)
    s = V.hold(r, ref, V.evaluate(r, inp))
    print(f"CVEMU {V.instantiation(r)} | {r.name}: worst err / bound {s['ratio']:.3f}, largest error {s['max_err']:.2e}")
    assert s["outside"] == 0 and s["ratio"] <= 1.0


@pytest.mark.parametrize("fault", V.FAULTS)
def test_every_fault_leaves_the_bound(fault):
    rows = [r for r in ROWS if V.fault_applies(r, fault)]
    assert len(rows) >= 3, fault
    if fault in ("gt_for_ge", "lt_for_le"):
        assert {r.name for r in rows} == {"exact_f1", "exact_f2", "exact_f2_bf16_ring"}
    caught = {}
    for r in rows:
        _, inp, ref = _numerics(r.name)
        caught[r.name] = V.hold(r, ref, V.evaluate(r, inp, fault))["outside"]
    print(f"CVFAULT {fault}: {len(rows)} rows, entries outside min {min(caught.values())} max {max(caught.values())}")
    assert all(v > 0 for v in caught.values()), {k: v for k, v in caught.items() if v == 0}


def test_ring_advance_reference():
    assert V.ring_advance_ref([-1, 0, -5, 9, 2], 3) == [0, 1, 1, 3, 3]
    assert V.ring_advance_ref([V.INT32_MAX, -V.INT32_MAX - 1, V.INT32_MAX], 4) == [0, 1, 4]
    assert [V.slot_of(-1, f, 3) for f in range(3)] == [1, 0, 2] and V.slot_of(V.INT32_MAX, 0, 3) == 0


# ---------------------------------------------------------------------------------------------
# the kernel's last-column / last-row branch (`off = -2`)
# ---------------------------------------------------------------------------------------------
def test_the_last_column_branch_is_not_reached():
    """Samples inside the edge mask with floor(ix) + 1 >= w or floor(iy) + 1 >= h, by the kernel's fp32 chain, over every row
    and a sweep of 160 poses x 4 frames on the 5 x 5 and the 21 x 37 map.  Measured: 0 of 2 684 045 masked samples.
    Why: xv = (gx / 2 + 0.5)(w - 1) and ix = ((gx + 1) / 2)(w - 1) round the same real number twice, each within a few ulps
    of w; xv <= w - 2 and ix >= w - 1 would put them 1 apart."""
    n = hit = 0
    for r in list(ROWS) + V.pose_sweep_rows():
        inp = _numerics(r.name)[1] if r.name in V.BY_NAME else V.make_inputs(r)
        a, b = V.rare_branch_count(r, inp)
        n, hit = n + a, hit + b
    print(f"last-column / last-row branch: {hit} of {n} masked samples")
    assert n > 100000 and hit == 0
