"""The references and seeded inputs of tests/test_loss_warp_edges_gpu.py are fit to judge a kernel: on the cases
that file runs, fp32 and fp64 ATen agree where the GPU test compares tightly, the points left out of a gradient
comparison are few, and every planted edge (ties, black frames, NaNs, missing bins, flat disparity) is really there.
No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import edge_inputs as E
from oracle import ref_ops as R

MODES = ["border", "zeros"]


def _sample(src, grid, mode):
    return F.grid_sample(src, grid, mode="bilinear", padding_mode=mode, align_corners=True)


def _fwd_and_grid_grad(src, grid, go, mode, dtype):
    g = grid.to(dtype).clone().requires_grad_(True)
    out = _sample(src.to(dtype), g, mode)
    (out * go.to(dtype)).sum().backward()
    return out.detach(), g.grad


def _grid_case(shape):
    Hi, Wi, Ho, Wo, C = shape
    grid = E.grid_cases(Hi, Wi, Ho, Wo, E.GRID_SEEDS[shape])
    src = E.grid_source(grid.shape[0], C, Hi, Wi, E.GRID_SEEDS[shape])
    go = torch.randn(grid.shape[0], C, Ho, Wo, generator=torch.Generator().manual_seed(5))
    return grid, src, go, E.grid_blocks(Hi, Wi)


def test_grid_blocks_hold_what_they_promise():
    lat = E.lattice_points(5, 9)
    assert lat.shape == (45, 2)
    ix, iy = (lat[:, 0] + 1) / 2 * 8, (lat[:, 1] + 1) / 2 * 4
    assert torch.equal(ix, ix.round()) and torch.equal(iy, iy.round())              # exact pixel centres in fp32
    assert torch.equal(ix.double(), (lat[:, 0].double() + 1) / 2 * 8)                # ... and the same in fp64
    assert sorted(set(ix.tolist())) == list(range(9)) and sorted(set(iy.tolist())) == list(range(5))
    with pytest.raises(ValueError):
        E.lattice_points(5, 8)
    rim = E.rim_points()
    assert rim.shape == (100, 2)
    vals = set(rim[:, 0].tolist())
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    assert {-1.0, 1.0, f32(-1 + 2.0 ** -20), f32(1 - 2.0 ** -20), f32(1 + E.RIM_OFFSETS[2]), f32(-1 - E.RIM_OFFSETS[2])} <= vals
    far = E.far_points()
    assert far.shape == (36, 2) and float(far.abs().max()) == f32(1e30) and float(far.abs().min()) == 3.0
    for shape in E.GRID_SHAPES:
        Hi, Wi, Ho, Wo, C = shape
        grid, _, _, blocks = _grid_case(shape)
        assert grid.shape == (len(blocks), Ho, Wo, 2) and grid.dtype == torch.float32
        assert ("lattice" in blocks) == (Hi > 1 and Wi > 1)
        assert torch.isfinite(grid).all()
        rnd = grid[blocks.index("random")]
        assert float(rnd.abs().max()) <= 1.3
        assert torch.equal(grid, E.grid_cases(Hi, Wi, Ho, Wo, E.GRID_SEEDS[shape]))         # seeded
    # the first shape's lattice block holds every pixel centre
    grid, _, _, blocks = _grid_case(E.GRID_SHAPES[0])
    assert len({tuple(p) for p in grid[blocks.index("lattice")].reshape(-1, 2).tolist()}) == 45


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", E.GRID_SHAPES, ids=str)
def test_grid_sample_fp32_and_fp64_agree_on_lattice_and_rim(shape, mode):
    grid, src, go, blocks = _grid_case(shape)
    keep = [i for i, n in enumerate(blocks) if n in ("lattice", "rim")]
    grid, src, go = grid[keep], src[keep], go[keep]
    o32, g32 = _fwd_and_grid_grad(src, grid, go, mode, torch.float32)
    o64, g64 = _fwd_and_grid_grad(src, grid, go, mode, torch.float64)
    assert rel_err(o32, o64) < 1e-6
    assert rel_err(g32, g64) < 1e-5
    man = R.grid_sample_manual(src, grid, mode == "border")
    assert rel_err(man, o32) < 1e-6 and rel_err(man, o64) < 1e-6


@pytest.mark.parametrize("shape", E.GRID_SHAPES, ids=str)
def test_grid_random_block_has_few_points_near_a_cell_boundary(shape):
    """Left out of the GPU test's gradient comparison only (fp32 and fp64 may pick different cells there)."""
    Hi, Wi = shape[:2]
    grid, _, _, blocks = _grid_case(shape)
    bad = E.near_integer(grid[blocks.index("random")][None], Hi, Wi)
    assert float(bad.float().mean()) <= 0.01
    # the rule itself: a coordinate 1e-5 from a pixel centre is caught, one 1e-3 away is not, a one-pixel axis never
    probe = torch.tensor([[[[-1 + 2 * (3 + 1e-5) / 8, 0.3], [-1 + 2 * (3 + 1e-3) / 8, 0.3]]]], dtype=torch.float32)
    assert E.near_integer(probe, 1, 9).reshape(-1).tolist() == [True, False]
    assert E.near_integer(probe.flip(-1), 9, 1).reshape(-1).tolist() == [True, False]
    assert not E.near_integer(probe, 1, 1).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", E.GRID_SHAPES, ids=str)
def test_grid_fp32_reference_has_no_nan_and_far_points_behave(shape, mode):
    grid, src, go, blocks = _grid_case(shape)
    o32, g32 = _fwd_and_grid_grad(src, grid, go, mode, torch.float32)
    assert torch.isfinite(o32).all() and torch.isfinite(g32).all()
    o64, g64 = _fwd_and_grid_grad(src, grid, go, mode, torch.float64)
    far = blocks.index("far")
    if mode == "zeros":
        assert not o64[far].any() and not g64[far].any() and not o32[far].any() and not g32[far].any()
    else:
        assert not g64[far].any() and float(o64[far].abs().max()) > 0


def test_smooth_cases_mix_plateaus_and_noise():
    for i, (B, C, H, W) in enumerate(E.SMOOTH_SHAPES):
        disp, img = E.smooth_cases(B, C, H, W, 300 + i)
        assert disp.shape == (B, 1, H, W) and img.shape == (B, C, H, W)
        eqx = disp[..., :, 1:] == disp[..., :, :-1]
        eqy = disp[..., 1:, :] == disp[..., :-1, :]
        assert eqx.any() or eqy.any()                        # sgn(0) occurs
        assert (~eqx).any() and (~eqy).any()                 # ... and so does a real step, along both axes
        if H * W >= 1000:
            flat = E.flat_pixels(disp)
            assert 0.01 < float(flat.float().mean()) < 0.5
            assert eqx.any() and eqy.any()
            # the fp64 reference's gradient is exactly 0 there
            d = disp.double().requires_grad_(True)
            R.smooth_loss(d, img.double()).backward()
            assert not d.grad[flat].any() and d.grad[~flat].any()


@pytest.mark.parametrize("shape", E.SELECT_SHAPES, ids=str)
def test_select_cases_cover_every_source_code_and_plant_real_ties(shape):
    B, C, H, W = shape
    c = E.select_cases(B, C, H, W, E.SELECT_SEEDS[shape])
    rp, idl = c["reproj"], c["identity"]
    assert rp.shape == (B, 2, H, W) and c["warped_m1"].shape == (B, C, H, W)
    assert torch.equal(rp[:, :1][c["tie_reproj"]], rp[:, 1:][c["tie_reproj"]])
    assert torch.equal(idl[:, :1][c["tie_identity"]], idl[:, 1:][c["tie_identity"]])
    sel, fidx = R.select_reprojection(rp, c["warped_m1"], c["warped_p1"])
    plain = rp.min(1, keepdim=True)[0]
    assert torch.equal(idl.min(1, keepdim=True)[0][c["tie_auto"]], plain[c["tie_auto"]])
    assert not fidx[c["tie_reproj"]].any()                  # first minimum wins on the CPU reference
    code = E.select_source_code(fidx, c["warped_m1"], c["warped_p1"], True)
    # the code names where `sel` came from
    assert torch.equal(sel, torch.where(code == 0, rp[:, :1], torch.where(code == 1, rp[:, 1:], torch.zeros_like(sel))))
    s0, s1 = c["warped_m1"].sum(1), c["warped_p1"].sum(1)
    for s in (s0, s1, c["warped_m1"].double().sum(1), c["warped_p1"].double().sum(1)):
        assert float(((s - 0.1).abs() / 0.1).min()) > 5e-4   # no channel sum within rounding of the threshold
    assert torch.equal(s0 < 0.1, c["warped_m1"].double().sum(1) < 0.1)
    if B * H * W >= 64:
        n = float(B * H * W)
        assert c["tie_reproj"].sum() >= 3 and c["tie_identity"].sum() >= 3 and c["tie_auto"].sum() >= 3
        for k in (0, 1, 2):
            assert float((code == k).sum()) / n >= 0.05, k
        near = (s0 < 0.15) | (s1 < 0.15)
        assert ((s0 > 0.1) & (s0 < 0.15)).any() and ((s1 > 0.1) & (s1 < 0.15)).any() and near.any()
        # the overwrite changes something the plain minimum would not have given
        assert (sel != plain).any() and (code[code < 2].long() != fidx[code < 2]).any()


def test_select_nan_layer_and_the_cpu_min_rule():
    shape = E.SELECT_SHAPES[-1]
    c = E.select_cases(*shape, E.SELECT_SEEDS[shape], nan_layer=True)
    for t in (c["reproj"], c["identity"]):
        n0, n1 = torch.isnan(t[:, 0]), torch.isnan(t[:, 1])
        assert (n0 & ~n1).sum() >= 2 and (n1 & ~n0).sum() >= 2 and (n0 & n1).sum() >= 2
        # torch.min on the CPU: NaN propagates, the first NaN's index is returned
        v, i = torch.min(t, 1)
        assert torch.equal(torch.isnan(v), n0 | n1)
        assert torch.equal(i[n0 | n1], (~n0 & n1)[n0 | n1].long())
    assert not (torch.isnan(c["reproj"]).any(1) & torch.isnan(c["identity"]).any(1)).any()
    a = torch.tensor([[float("nan"), 1.0], [1.0, float("nan")], [2.0, 1.0]])
    assert torch.argmin(a, 1).tolist() == [0, 1, 1]


@pytest.mark.parametrize("is_multi", [False, True])
def test_tail_all_masked_reference_is_zero_with_finite_gradients(is_multi):
    for B, H, W in E.TAIL_SHAPES[:3]:
        c = E.tail_cases(B, H, W, 5, is_multi, all_masked=True)
        ref = E.tail_reference(c, is_multi)
        assert float(ref["rl"]) == 0.0 and not ref["mask"].any()
        assert torch.isfinite(ref["d_reproj"]).all() and not ref["d_reproj"].any()
        if is_multi:
            assert torch.isfinite(ref["d_multi"]).all() and torch.isfinite(ref["target"]).all()
            assert float(ref["cl"]) > 0 or B * H * W == 1
    # the ordinary variant is not degenerate: both mask values occur, every source code occurs
    c = E.tail_cases(3, 3, 5, 5, is_multi)
    ref = E.tail_reference(c, is_multi)
    assert ref["mask"].any() and not ref["mask"].all() and float(ref["rl"]) > 0
    assert set(c["src"].reshape(-1).tolist()) == {0, 1, 2}


def test_reduce_cases_hold_all_four_pixel_kinds():
    for B, D, h, w in E.REDUCE_SHAPES:
        raw = E.reduce_cases(B, D, h, w)
        assert raw.shape == (B, D, h, w) and float(raw.min()) >= 0 and float(raw.max()) < 100
        if B * h * w < 4:
            continue
        k = E.reduce_pixel_kinds(raw)
        for name in ("all_positive", "some_zero", "all_zero", "tie", "tie_with_zero"):
            if name == "tie_with_zero" and D < 4:
                continue
            assert k[name].any(), (name, D)
        assert (k["all_positive"] & ~k["tie"]).any()
        # the reference takes the first of tied minima, and bin 0 where every bin is missing
        bins = R.depth_bins_log(0.37, 14.5, D)
        masked, conf, idx, low = E.reduce_reference(raw, bins, R)
        miss = raw == 0
        filled = torch.where(miss, raw.max(1, keepdim=True)[0].expand_as(raw), raw)
        viz = torch.where(filled == 0, torch.full_like(filled, 100.0), filled)
        hit = viz == viz.min(1, keepdim=True)[0]
        first = (hit & (hit.cumsum(1) == 1)).float().argmax(1)
        assert torch.equal(idx, first)
        assert (hit.sum(1) >= 2)[k["tie"]].all() and (idx[k["tie"]] < D - 1).all()
        assert not idx[k["all_zero"]].any()
        assert torch.equal(conf, k["all_positive"].float())
        assert torch.equal(masked, filled * conf[:, None])
