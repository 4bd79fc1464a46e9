"""Video streaming on the host: `DepthPredictor.stream()` with `device="cpu"` (torch composites, host-side ring) against
`predict` on the same frames, and `predict`'s `keep` (missing lookup frames).  64 x 96, B = 2, RepLKNet-31B with conditioned
synthetic weights, as tests/test_multiframe_gpu.py; the clip is the four rendered frames -2, -1, 0, +1 in time order."""
import os
import re

import pytest
import torch

from conftest import ROOT, rel_err

from oracle import synth

FOLD_TOL = 1e-4      # same schedule, different batching, both fp32 (tests/test_inference_gpu.py)
TIE_CAP = 5e-3       # share of quarter-resolution pixels whose winning bin may differ (tests/test_inference_gpu.py)
H, W, B = 64, 96, 2
CLIP = (-2, -1, 0, 1)
_cache = {}


def _setup(Fr, **extra):
    """(model, opt, clip [4][B,3,H,W] in time order, K2, inv_K2, CPU predictor): built once per configuration."""
    key = (Fr, tuple(sorted(extra.items())))
    if key not in _cache:
        from ppeadepth import networks, options
        from ppeadepth.inference import DepthPredictor
        opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, num_matching_frames=Fr, **extra)
        torch.manual_seed(0)
        model = networks.RepDepth(opt)
        synth.fill_state_dict(model, conditioned=True)
        model.train()
        data = synth.make_rendered_inputs(B, H, W, frame_ids=(0, -1, 1, -2))
        clip = [data[("color", f, 0)] for f in CLIP]
        _cache[key] = (model, opt, clip, data[("K", 2)], data[("inv_K", 2)], DepthPredictor(model, opt, device="cpu"))
    return _cache[key]


def _differ(low, ref):
    return float(((low - ref).abs() > 1e-5 * ref.abs().clamp_min(1e-6)).float().mean())


def _oracle(p, clip, t, present, K2, inv_K2, gen):
    """`predict` on frame t with its lookups t-1 .. t-F; a slot that `present` marks absent holds a random image."""
    Fr = present.shape[1]
    looks = torch.stack([clip[t - 1 - j] if t - 1 - j >= 0 else torch.rand(B, 3, H, W, generator=gen) for j in range(Fr)], 1)
    for b in range(B):
        for j in range(Fr):
            if not bool(present[b, j]):
                looks[b, j] = torch.rand(3, H, W, generator=gen)
    keep = None if bool(present.all()) else present.float()
    return p.predict(clip[t], looks, K2, inv_K2, 0.1, 10.0, keep=keep)


def _compare(tag, out, ref, worst):
    e, e_pose, differ = rel_err(out["disp"], ref["disp"]), rel_err(out["pose"], ref["pose"]), \
        _differ(out["lowest_cost"], ref["lowest_cost"])
    print(f"[{tag}] stream vs predict: disp {e:.3e} pose {e_pose:.3e} lowest_cost differs at {differ:.4%}")
    for k, v in (("disp", e), ("pose", e_pose), ("differ", differ)):
        worst[k] = max(worst.get(k, 0.0), v)
    assert e <= FOLD_TOL and e_pose <= FOLD_TOL
    assert differ <= TIE_CAP


def test_predict_keep_ignores_the_missing_slots():
    """(a) keep [B,F] with zeros: two different garbage images in the missing slots give the same bits and exact-zero poses
    there and behind them in the chain; keep=None is the call without the argument."""
    _model, _opt, clip, K2, inv_K2, p = _setup(2)
    keep = torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    outs = []
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        looks = torch.stack([clip[1], clip[0]], 1).clone()
        looks[0, 1] = torch.rand(3, H, W, generator=g)
        looks[1, 0] = torch.rand(3, H, W, generator=g) * 5 - 2
        outs.append(p.predict(clip[2], looks, K2, inv_K2, 0.1, 10.0, keep=keep))
    for k in ("disp", "lowest_cost", "pose"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    pose = outs[0]["pose"]
    assert float(pose[0, 1].abs().sum()) == 0 and float(pose[1].abs().sum()) == 0        # item 1: -2 is chained behind -1
    assert float(pose[0, 0].abs().sum()) > 0
    looks = torch.stack([clip[1], clip[0]], 1)
    plain = p.predict(clip[2], looks, K2, inv_K2, 0.1, 10.0)
    none = p.predict(clip[2], looks, K2, inv_K2, 0.1, 10.0, keep=None)
    for k in ("disp", "lowest_cost", "pose"):
        assert torch.equal(plain[k], none[k]), k
    assert not torch.equal(plain["disp"], outs[0]["disp"])


@pytest.mark.parametrize("Fr", [1, 2])
def test_cpu_stream_matches_predict(Fr):
    """(b) every push of the clip against `predict` on the same frames (clip start: `keep=present`, random images in the
    absent slots).  Measured, worst over the four pushes: F = 1 disp 0.0e+00 pose 0.0e+00, F = 2 disp 0.0e+00 pose 0.0e+00;
    lowest_cost equal at every pixel (eval BatchNorm and every host convolution are per sample: the host gives the same
    bits for a B and a (1 + F) B batch)."""
    _model, _opt, clip, K2, inv_K2, p = _setup(Fr)
    s = p.stream(B)
    gen = torch.Generator().manual_seed(3)
    worst = {}
    for t in range(len(clip)):
        out = s.push(clip[t], K2, inv_K2, 0.1, 10.0)
        want = torch.tensor([[t > j for j in range(Fr)]] * B)
        assert out["present"].dtype == torch.bool and torch.equal(out["present"], want)
        assert out["disp"].shape == (B, 1, H, W) and out["pose"].shape == (B, Fr, 4, 4)
        assert out["lowest_cost"].shape == (B, H // 4, W // 4)
        assert float(out["pose"][~out["present"]].abs().sum()) == 0
        _compare(f"F={Fr} t={t}", out, _oracle(p, clip, t, want, K2, inv_K2, gen), worst)
        if t >= Fr:
            assert float((out["lowest_cost"] < 9.9).float().mean()) > 0.2      # the sweep found minima past bin 0 (1 / 0.1)
    print(f"F = {Fr} worst: {worst}")


def test_reset_mask_and_refresh():
    """(c) reset(mask) restarts only the masked cameras, the others keep their history; refresh() resets every stream."""
    _model, _opt, clip, K2, inv_K2, p = _setup(2)
    s, other = p.stream(B), p.stream(B)
    for t in (0, 1):
        s.push(clip[t], K2, inv_K2, 0.1, 10.0)
        other.push(clip[t], K2, inv_K2, 0.1, 10.0)
    s.reset(torch.tensor([True, False]))
    out = s.push(clip[2], K2, inv_K2, 0.1, 10.0)
    want = torch.tensor([[False, False], [True, True]])
    assert torch.equal(out["present"], want)
    _compare("masked reset", out, _oracle(p, clip, 2, want, K2, inv_K2, torch.Generator().manual_seed(4)), {})
    out = s.push(clip[3], K2, inv_K2, 0.1, 10.0)
    assert torch.equal(out["present"], torch.tensor([[True, False], [True, True]]))
    p.refresh()
    fresh = p.stream(B).push(clip[3], K2, inv_K2, 0.1, 10.0)
    for st in (s, other):
        out = st.push(clip[3], K2, inv_K2, 0.1, 10.0)
        assert not bool(out["present"].any()) and float(out["pose"].abs().sum()) == 0
        for k in ("disp", "lowest_cost"):
            assert torch.equal(out[k], fresh[k]), k


def test_refusals():
    """(d) a future lookup frame, a wrong batch size and a wrong image size are errors, as is capture on the host."""
    from ppeadepth._abi import PpeaKernelError
    _model, _opt, clip, K2, inv_K2, p = _setup(1)
    s = p.stream(B)
    with pytest.raises(PpeaKernelError):
        s.push(torch.cat([clip[0], clip[0][:1]], 0), K2, inv_K2, 0.1, 10.0)
    with pytest.raises(PpeaKernelError):
        s.push(clip[0][:, :, :-8], K2, inv_K2, 0.1, 10.0)
    with pytest.raises(PpeaKernelError):
        s.capture()
    with pytest.raises(PpeaKernelError):
        s.reset(torch.tensor([True]))
    with pytest.raises(PpeaKernelError):
        p.predict(clip[1], clip[0], K2, inv_K2, 0.1, 10.0, keep=torch.ones(B, 2))
    p_future = _setup(1, use_future_frame=True)[5]
    with pytest.raises(PpeaKernelError):
        p_future.stream(B)


def test_stream_entry_points_are_declared_and_bound():
    from ppeadepth import _abi
    header = open(os.path.join(ROOT, "include", "ppea_depth.h")).read()
    nargs = {"ppea_cost_volume_ring_fwd_f32": 16, "ppea_cost_volume_ring_fwd_bf16": 16, "ppea_cv_ring_store_f32": 9,
             "ppea_cv_ring_store_bf16": 9, "ppea_cv_ring_advance": 4, "ppea_pose_chain_ring_fwd_f32": 10}
    for name, n in nargs.items():
        assert re.search(r"\bint " + name + r"\(", header), name
        assert len(_abi.SIGNATURES[name]) == n, name
        assert hasattr(_abi.lib, name), name
    assert _abi.lib.ppea_abi_version() == _abi.ABI_VERSION >= 18
