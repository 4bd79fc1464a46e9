"""Video streaming on the GPU: the ring kernels against their plain siblings bit for bit, and `DepthPredictor.stream()` against
`predict` on the same frames (64 x 96, B = 2, RepLKNet-31B with conditioned synthetic weights, as
tests/test_multiframe_gpu.py; the clip is the four rendered frames -2, -1, 0, +1 in time order)."""
import pytest
import torch

from conftest import rel_err

from oracle import synth

pytestmark = pytest.mark.gpu

FOLD_TOL = 1e-4      # same schedule, different batching, both fp32 (tests/test_inference_gpu.py)
TIE_CAP = 5e-3       # share of quarter-resolution pixels whose winning bin may differ (tests/test_inference_gpu.py)
H, W, B = 64, 96, 2
CLIP = (-2, -1, 0, 1)
_cache = {}


def _setup(device, Fr):
    """(model in train mode, opt, clip [4][B,3,H,W] in time order, K2, inv_K2): built once per F, never modified."""
    if Fr not in _cache:
        from ppeadepth import networks, options
        opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, num_matching_frames=Fr)
        torch.manual_seed(0)
        model = networks.RepDepth(opt)
        synth.fill_state_dict(model, conditioned=True)
        model.to(device).train()
        data = {k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W, frame_ids=(0, -1, 1, -2)).items()}
        _cache[Fr] = (model, opt, [data[("color", f, 0)] for f in CLIP], data[("K", 2)], data[("inv_K", 2)])
    return _cache[Fr]


def _differ(low, ref):
    return float(((low - ref).abs() > 1e-5 * ref.abs().clamp_min(1e-6)).float().mean())


def _state(device, head, seen):
    return torch.tensor([head] + list(seen), device=device, dtype=torch.int32)


# ---- kernels ----------------------------------------------------------------------------------------------------------
SB, SC, Sh, Sw, SD = 2, 30, 12, 20, 7      # odd number of channel pairs, hw no multiple of the block, D no multiple of any DB


def _sweep_inputs(device, Fr, dtype):
    g = torch.Generator().manual_seed(10 + Fr)
    cur = torch.randn(SB, SC, Sh, Sw, generator=g).to(device, dtype)
    feats = [torch.randn(SB, SC, Sh, Sw, generator=g).to(device, dtype) for _ in range(Fr)]
    K = torch.eye(4).repeat(SB, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = Sw / 2, Sh / 2, Sw / 2, Sh / 2
    inv_K = torch.linalg.inv(K)
    poses = torch.eye(4).repeat(SB, Fr, 1, 1)
    for b in range(SB):
        for j in range(Fr):                 # shifts of at most one column and a quarter row towards the inside: every
            poses[b, j, 0, 3] = 0.02 * (j + 1) + 0.005 * b          # sample of an inner pixel stays inside the edge mask
            poses[b, j, 1, 3] = 0.01 * (j + 1)
    return cur, feats, poses.to(device), K.to(device), inv_K.to(device), torch.linspace(1.0, 5.0, SD, device=device)


def _ring_of(feats, head, ops):
    """Ring with lookup j in slot (head - 1 - j) mod F, in the layout `ring_store` writes."""
    Fr = len(feats)
    slots = [None] * Fr
    for j, f in enumerate(feats):
        slots[(head - 1 - j) % Fr] = ops.pack_pairs(f) if f.dtype == torch.bfloat16 else f
    return torch.stack(slots, 0).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Fr", [1, 2, 4])
def test_ring_sweep_is_the_sweep(device, Fr, dtype):
    """(e) every head position; then the oldest frame of item 1 absent by its seen count, against that pose zeroed."""
    from ppeadepth import ops
    cur, feats, poses, K, inv_K, bins = _sweep_inputs(device, Fr, dtype)
    ref = ops.cost_volume_multi(cur, torch.stack(feats, 1), poses, K, inv_K, bins)
    share = float((ref != 0).float().mean())
    print(f"F = {Fr} {dtype}: {share:.1%} of the cost entries are non-zero")
    assert share >= 0.5
    zeroed = poses.clone()
    zeroed[1, Fr - 1] = 0
    ref_absent = ops.cost_volume_multi(cur, torch.stack(feats, 1), zeroed, K, inv_K, bins)
    assert not torch.equal(ref, ref_absent)
    for head in range(Fr):
        ring = _ring_of(feats, head, ops)
        assert ring.dtype == (torch.int32 if dtype == torch.bfloat16 else torch.float32)
        full = ops.cost_volume_ring(cur, ring, _state(device, head, [Fr] * SB), poses, K, inv_K, bins)
        assert torch.equal(full, ref), head
        noflags = ops.cost_volume_ring(cur, ring, _state(device, head, [Fr] * SB), poses, K, inv_K, bins, zero_pose_skip=False)
        assert torch.equal(noflags, ref), head
        absent = ops.cost_volume_ring(cur, ring, _state(device, head, [Fr, Fr - 1]), poses, K, inv_K, bins)
        assert torch.equal(absent, ref_absent), head
        flagged = ops.cost_volume_ring(cur, ring, _state(device, head, [Fr] * SB), zeroed, K, inv_K, bins)
        assert torch.equal(flagged, ref_absent), head


@pytest.mark.parametrize("Fr", [1, 3])
def test_ring_store(device, Fr):
    """(f) the head's slot holds the source (bf16: cv_pack_pairs' dwords, channel 2c low, 2c + 1 high), the others are
    untouched; the counter advance wraps the head and clamps the seen counts."""
    from ppeadepth import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(SB, SC, Sh, Sw, generator=g).to(device)
    xb = x.to(torch.bfloat16)
    bits = xb.view(torch.int16).to(torch.int32) & 0xffff
    pairs = bits[:, 0::2] | (bits[:, 1::2] << 16)                       # int32 wrap-around = the dword's bit pattern
    assert torch.equal(ops.pack_pairs(xb), pairs)
    for head in range(Fr):
        st = _state(device, head, [0] * SB)
        ring = torch.full((Fr, SB, SC, Sh, Sw), -7.0, device=device)
        ops.ring_store(x, ring, st)
        ringp = torch.full((Fr, SB, SC // 2, Sh, Sw), -7, device=device, dtype=torch.int32)
        ops.ring_store(xb, ringp, st)
        for s in range(Fr):
            assert torch.equal(ring[s], x if s == head else torch.full_like(x, -7.0)), (head, s)
            assert torch.equal(ringp[s], pairs if s == head else torch.full_like(pairs, -7)), (head, s)
        assert torch.equal(st, _state(device, head, [0] * SB))
    st = _state(device, 0, [0, Fr])
    for n in range(1, Fr + 2):
        ops.ring_advance(st, Fr)
        assert st.tolist() == [n % Fr, min(n, Fr), Fr]


@pytest.mark.parametrize("Fr", [1, 3])
def test_ring_pose_chain(device, Fr):
    """(g) every head position, item b with seen count b = 0 .. F, against `ops.pose_chain` with the matching `keep`."""
    from ppeadepth import ops
    nb = Fr + 1
    g = torch.Generator().manual_seed(6)
    pairs = [(torch.randn(nb, 1, 3, generator=g).to(device) * 0.1, torch.randn(nb, 1, 3, generator=g).to(device))
             for _ in range(Fr)]
    present = torch.arange(nb, device=device)[:, None] > torch.arange(Fr, device=device)[None]
    ref = ops.pose_chain(pairs, [(j, True, j - 1) for j in range(Fr)], keep=present.float())
    assert float(ref[~present].abs().sum()) == 0 and float(ref[present].abs().sum()) > 0
    for head in range(Fr):
        ring = torch.full((Fr, nb, 2, 3), float("nan"), device=device)
        for j, (aa, tr) in enumerate(pairs):
            ring[(head - j) % Fr, :, 0], ring[(head - j) % Fr, :, 1] = aa[:, 0], tr[:, 0]
        st = _state(device, head, range(nb))
        T, pr = ops.pose_chain_ring(ring, st)
        assert torch.equal(T, ref) and torch.equal(pr, present), head
        want = ring.clone()
        ring[head] = float("nan")                                        # the newest pair arrives with the call
        T, pr = ops.pose_chain_ring(ring, st, new=pairs[0])
        assert torch.equal(T, ref) and torch.equal(pr, present), head
        assert torch.equal(ring, want)
        assert torch.equal(st, _state(device, head, range(nb)))


# ---- the stream -------------------------------------------------------------------------------------------------------
def _oracle(p, clip, t, present, K2, inv_K2, gen):
    """`predict` on frame t with its lookups t-1 .. t-F; a slot that `present` marks absent holds a random image."""
    Fr = present.shape[1]
    looks = torch.stack([clip[t - 1 - j].clone() if t - 1 - j >= 0 else torch.zeros_like(clip[0]) for j in range(Fr)], 1)
    for b in range(B):
        for j in range(Fr):
            if not bool(present[b, j]):
                looks[b, j] = torch.rand(3, H, W, generator=gen).to(looks.device)
    keep = None if bool(present.all()) else present.float()
    return p.predict(clip[t], looks, K2, inv_K2, 0.1, 10.0, keep=keep)


@pytest.mark.parametrize("Fr", [1, 2])
def test_fp32_stream_matches_predict(device, Fr):
    """(h) every push of the clip against `predict` on the same frames (clip start: `keep=present`, random images in the
    absent slots), then a masked reset.  Measured, F = 1 and F = 2, all four pushes: disp 0.0e+00, pose 0.0e+00, lowest_cost
    equal at every pixel (the kernels on this path are per sample: a B and a (1 + F) B batch give the same bits)."""
    from ppeadepth.inference import DepthPredictor
    model, opt, clip, K2, inv_K2 = _setup(device, Fr)
    p = DepthPredictor(model, opt, amp_dtype=None)
    s = p.stream(B)
    gen = torch.Generator().manual_seed(3)

    def check(tag, out, t, want):
        assert out["present"].dtype == torch.bool and torch.equal(out["present"].cpu(), want)
        assert float(out["pose"][~out["present"]].abs().sum()) == 0
        ref = _oracle(p, clip, t, want, K2, inv_K2, gen)
        e, e_pose = rel_err(out["disp"], ref["disp"]), rel_err(out["pose"], ref["pose"])
        differ = _differ(out["lowest_cost"], ref["lowest_cost"])
        print(f"[F={Fr} {tag}] fp32 stream vs predict: disp {e:.3e} pose {e_pose:.3e} lowest_cost differs at {differ:.4%}")
        assert e <= FOLD_TOL and e_pose <= FOLD_TOL
        assert differ <= TIE_CAP

    for t in range(len(clip)):
        out = s.push(clip[t], K2, inv_K2, 0.1, 10.0)
        assert out["disp"].shape == (B, 1, H, W) and out["pose"].shape == (B, Fr, 4, 4)
        check(f"t={t}", out, t, torch.tensor([[t > j for j in range(Fr)]] * B))
        if t >= Fr:
            assert float((out["lowest_cost"] < 9.9).float().mean()) > 0.2      # the sweep found minima past bin 0 (1 / 0.1)
    s.reset(torch.tensor([True, False]))
    out = s.push(clip[3], K2, inv_K2, 0.1, 10.0)               # item 1 goes on: frame +1 again, after -1, 0, +1
    want = torch.tensor([[False] * Fr, [True] * Fr])
    assert torch.equal(out["present"].cpu(), want)
    looks = torch.stack([clip[3 - j] for j in range(Fr)], 1)
    ref = p.predict(clip[3], looks, K2, inv_K2, 0.1, 10.0, keep=want.float().to(device))
    assert rel_err(out["disp"], ref["disp"]) <= FOLD_TOL and rel_err(out["pose"], ref["pose"]) <= FOLD_TOL
    assert _differ(out["lowest_cost"], ref["lowest_cost"]) <= TIE_CAP
    p.refresh()
    assert not bool(s.push(clip[0], K2, inv_K2, 0.1, 10.0)["present"].any())


def test_bf16_stream_is_no_worse_than_bf16_predict(device):
    """(i) per frame with full history: error of the bf16 stream against the fp32 stream <= 1.5 x the error of bf16 `predict`
    against fp32 `predict` (the rule of test_bf16_predictor_is_no_worse_than_the_bf16_module_path).
    Measured: frame 0 stream 6.4e-03 predict 6.4e-03, frame +1 stream 6.0e-03 predict 6.0e-03 (bf16 stream == bf16 predict)."""
    from ppeadepth.inference import DepthPredictor
    Fr = 2
    model, opt, clip, K2, inv_K2 = _setup(device, Fr)
    p32, p16 = DepthPredictor(model, opt, amp_dtype=None), DepthPredictor(model, opt)
    s32, s16 = p32.stream(B), p16.stream(B)
    for t in range(len(clip)):
        o32, o16 = s32.push(clip[t], K2, inv_K2, 0.1, 10.0), s16.push(clip[t], K2, inv_K2, 0.1, 10.0)
        assert torch.equal(o32["present"], o16["present"])
        if t < Fr:
            continue
        assert s16.ring.dtype == torch.int32 and s32.ring.dtype == torch.float32
        looks = torch.stack([clip[t - 1 - j] for j in range(Fr)], 1)
        r32, r16 = (q.predict(clip[t], looks, K2, inv_K2, 0.1, 10.0) for q in (p32, p16))
        e_s, e_p = rel_err(o16["disp"], o32["disp"]), rel_err(r16["disp"], r32["disp"])
        print(f"t={t} bf16 vs fp32: stream {e_s:.3e} predict {e_p:.3e}; bf16 stream vs bf16 predict "
              f"{rel_err(o16['disp'], r16['disp']):.3e}")
        assert e_s <= 1.5 * e_p


def test_captured_stream_is_bitwise_the_eager_stream(device):
    """(j) clip, reset, clip again: one graph replay per push, the bits of the eager stream."""
    from ppeadepth.inference import DepthPredictor
    model, opt, clip, K2, inv_K2 = _setup(device, 2)
    p = DepthPredictor(model, opt)

    def run(s):
        outs = []
        for _ in range(2):
            outs += [s.push(c, K2, inv_K2, 0.1, 10.0) for c in clip]
            s.reset()
        return outs

    eager = run(p.stream(B))
    s = p.stream(B).capture()
    replays = []
    inner = s._graph["graph"]
    s._graph["graph"] = type("Counted", (), {"replay": (lambda self: (replays.append(1), inner.replay())[1])})()
    replay = run(s)
    for i, (r, e) in enumerate(zip(replay, eager)):
        for k in ("disp", "lowest_cost", "pose", "present"):
            assert torch.equal(r[k], e[k]), (i, k)
    assert len(replays) == len(replay) == 8
    assert not torch.equal(replay[2]["disp"], replay[3]["disp"])
    assert bool(replay[2]["present"].all()) and not bool(replay[4]["present"].any())


def test_a_push_launches_fewer_kernels_than_predict(device):
    """(k) F = 2, bf16, eager: device kernels of one push with full history against one `predict`.  Measured: push 541,
    predict 547."""
    from torch.profiler import ProfilerActivity, profile
    from ppeadepth.inference import DepthPredictor
    model, opt, clip, K2, inv_K2 = _setup(device, 2)
    p = DepthPredictor(model, opt)
    s = p.stream(B)
    looks = torch.stack([clip[1], clip[0]], 1)

    def kernels(fn):
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name
                and not e.name.startswith(("Memcpy", "Memset"))]

    for c in clip[:2]:
        s.push(c, K2, inv_K2, 0.1, 10.0)
    n_push = len(kernels(lambda: s.push(clip[2], K2, inv_K2, 0.1, 10.0)))
    n_predict = len(kernels(lambda: p.predict(clip[2], looks, K2, inv_K2, 0.1, 10.0)))
    print(f"device kernels, F = 2, bf16, eager: push {n_push}, predict {n_predict}")
    assert n_push > 20, "the profiler recorded no device kernels"
    assert n_push < n_predict
