"""DepthPredictor on the GPU: the inference epilogue of the 1x1-conv GEMM against an fp64 composite, the fp32 and bf16
predictors against the reference golden (tests/golden/infer.npz) and the eval-mode module path, graph replay, and the
library-kernel census of one prediction."""
import json
import os
import re

import pytest
import torch

from conftest import rel_err

from oracle import pw_inputs as PW
from oracle import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3
# predictor vs the eval-mode module path, both fp32 on the same kernels' arithmetic: only the affine maps and the merged
# k x k + 5 x 5 sum re-associate (the bound the issue sets for this comparison; it cannot run on the CPU, where the module
# path's depthwise and cost-volume operators do not exist, so it is asserted here)
FOLD_TOL = 1e-4
PW_TOL = PW.INFER_TOL     # 2^-7: bound of test_pwconv_mfma / test_pwconv_v2_lds_dma_ring_every_tile for the same main loop


def _g(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _infer(a, x, s, o, act, r1, r2, r2s, s2, o2, want2):
    """`ops.pwconv_table` (the operator the predictor launches `ppea_pwconv_infer_bf16` through) -> (served, y, y2)."""
    from ppeadepth import ops
    out = ops.pwconv_table(x, a, None if s is None else torch.stack([s, o]), act, r1, r2, r2s,
                           torch.stack([s2, o2]) if want2 else None)
    torch.cuda.synchronize()
    return (False, None, None) if out is None else (True,) + out


# the trunk's 1x1 convs at 192 x 640, batch 12 (31B and 31L), and batch 1
SHAPES = [(12, 128, 128, 48, 160), (12, 512, 128, 48, 160), (12, 128, 512, 48, 160), (12, 256, 128, 24, 80),
          (12, 2048, 512, 12, 40), (12, 512, 2048, 12, 40), (12, 4096, 1024, 6, 20), (12, 1024, 4096, 6, 20),
          (12, 192, 192, 48, 160), (12, 1536, 6144, 6, 20), (1, 128, 128, 48, 160), (1, 1024, 1024, 6, 20)]
# (act, r1, r2, Y2) as the schedule uses them: pw1 of a RepLKBlock / stem / transition, pw1 of a ConvFFN, pw2 in the
# middle of a stage, pw2 of the stage's last block, pw2 of a block without an adapter, plain table
COMBOS = [(1, False, False, False), (2, False, False, False), (0, True, True, True), (0, True, True, False),
          (0, True, False, True), (0, False, False, False)]


@pytest.mark.parametrize("B,M,K,H,W", SHAPES)
def test_pwconv_inference_epilogue_against_fp64(device, B, M, K, H, W):
    g = _g(M + K + H + B)
    x = torch.randn(B, K, H, W, generator=g).bfloat16().to(device)
    a = (torch.randn(M, K, generator=g) / K ** 0.5).bfloat16().to(device)
    s, s2 = (torch.rand(M, generator=g) + 0.5).to(device), (torch.rand(M, generator=g) + 0.5).to(device)
    o, o2 = (0.3 * torch.randn(M, generator=g)).to(device), (0.3 * torch.randn(M, generator=g)).to(device)
    r1 = torch.randn(B, M, H, W, generator=g).bfloat16().to(device)
    r2 = torch.randn(B, M, H, W, generator=g).bfloat16().to(device)
    acc = torch.einsum("mk,bkhw->bmhw", a.double(), x.double())
    v = lambda t: t.double().view(1, -1, 1, 1)               # noqa: E731
    for act, use1, use2, want2 in COMBOS:
        ok, y, y2 = _infer(a, x, s, o, act, r1 if use1 else None, r2 if use2 else None, 0.75, s2, o2, want2)
        assert ok and (y2 is not None) == want2, (act, use1, use2, want2)
        # the float64 reference shared with tests/test_pw_arms_gpu.py
        ref, ref2 = PW.infer_reference(acc, s, o, act, r1 if use1 else None, r2 if use2 else None, 0.75, s2, o2)
        e = float((y.double() - ref).abs().max() / ref.abs().max())
        print(f"[{B},{M},{K},{H}x{W}] act {act} r1 {use1} r2 {use2}: Y {e:.3e}", end="")
        assert e <= PW_TOL, (act, use1, use2, want2, e)
        if want2:
            e2 = float((y2.double() - ref2).abs().max() / ref2.abs().max())
            print(f" Y2 {e2:.3e}", end="")
            assert e2 <= PW_TOL, (act, use1, use2, e2)
            # ... and it is the table applied to Y AS STORED (what the unfused BatchNorm would read)
            again = (v(s2) * y.double() + v(o2)).float().bfloat16()
            assert (y2.float() - again.float()).abs().max() <= 2 ** -7 * again.float().abs().max()
        print()
    # s = NULL is 1, o = NULL is 0
    ok, y, _ = _infer(a, x, None, None, 0, None, None, 1.0, None, None, False)
    assert ok and float((y.double() - acc).abs().max() / acc.abs().max()) <= PW_TOL


@pytest.mark.parametrize("B,M,K,H,W", [(2, 128, 128, 6, 21), (2, 128, 72, 12, 40)])
def test_pwconv_inference_epilogue_refuses_shapes_it_does_not_serve(device, B, M, K, H, W):
    x = torch.randn(B, K, H, W, generator=_g(1)).bfloat16().to(device)
    a = torch.randn(M, K, generator=_g(2)).bfloat16().to(device)
    s = torch.ones(M, device=device)
    ok, y, _ = _infer(a, x, s, s, 0, None, None, 1.0, None, None, False)
    assert not ok and y is None                              # PPEA_ERR_UNSUPPORTED: the operator has no result


# the large-kernel depthwise convs of the trunk at 192 x 640: 31B stages 0-3, 31L stage 0 / 3, batch 1
DW_SHAPES = [(12, 128, 48, 160, 31), (12, 256, 24, 80, 29), (12, 512, 12, 40, 27), (12, 1024, 6, 20, 13),
             (12, 192, 48, 160, 31), (12, 1536, 6, 20, 13), (1, 128, 48, 160, 31), (1, 512, 12, 40, 27)]


def _dw_ref(x, w, bias, relu):
    K = w.shape[-1]
    y = torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), bias.double().cpu(), 1, K // 2, 1, w.shape[0])
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("N,C,H,W,K", DW_SHAPES)
def test_merged_large_kernel_bias_relu_against_fp64(device, N, C, H, W, K):
    """`ppea_dwconv_lk_fwd_bias_act_bf16p` (MFMA) and `_bf16` / `_f32` (fp32 arithmetic) against an fp64 composite on the
    bf16-rounded operands, with and without ReLU.  Bounds: bf16 outputs as test_dwconv_bf16_mfma_full_size_vs_fp32_kernel
    (|err| <= |ref| 2^-7 + max|ref| 1e-3), fp32 as the fp32 kernel's FWD_TOL (2e-5 relative)."""
    from ppeadepth import ops
    g = _g(N + C + K)
    w = (torch.randn(C, 1, K, K, generator=g) / K).bfloat16().float().to(device)
    bias = (0.5 * torch.randn(C, generator=g)).to(device)
    x = torch.randn(N, C, H, W, generator=g).bfloat16().to(device)
    packed = ops.pack_dwconv_filter(w, False)
    for relu in (1, 0):
        ref = _dw_ref(x, w, bias, relu)
        # the operator's ladder: packed image + bf16 x -> the MFMA kernel; no image -> the plain kernel of x's dtype
        ys = {"bf16p": ops.dwconv_lk_bias_act(x, w, packed, bias, relu), "bf16": ops.dwconv_lk_bias_act(x, w, None, bias, relu)}
        y32 = ops.dwconv_lk_bias_act(x.float(), w, None, bias, relu)
        torch.cuda.synchronize()
        assert y32.dtype == torch.float32 and all(y.dtype == torch.bfloat16 for y in ys.values())
        for name, y in ys.items():
            err = (y.double().cpu() - ref).abs()
            print(f"[{N},{C},{H}x{W}] K {K} relu {relu} {name}: {float(err.max() / ref.abs().max()):.3e}")
            assert not bool((err > ref.abs() * 2 ** -7 + ref.abs().max() * 1e-3).any()), name
        e32 = rel_err(y32.cpu(), ref)
        print(f"    f32: {e32:.3e}")
        assert e32 <= 2e-5


def test_merged_large_kernel_bias_relu_refuses_kernel_sizes_without_a_tile(device):
    from ppeadepth import ops
    N, C, H, W, K = 2, 32, 12, 40, 7
    x = torch.randn(N, C, H, W, generator=_g(3)).bfloat16().to(device)
    w = torch.randn(C, 1, K, K, generator=_g(4)).to(device)
    bias = torch.zeros(C, device=device)
    # None = the packed MFMA kernel AND the plain bf16 kernel answered PPEA_ERR_UNSUPPORTED (any other status raises)
    assert ops.dwconv_lk_bias_act(x, w, ops.pack_dwconv_filter(w, False), bias, 1) is None
    assert ops.dwconv_lk_bias_act(x, w, None, bias, 1) is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,C,H,W,stride", [(12, 128, 96, 320, 1), (12, 128, 96, 320, 2), (12, 256, 48, 160, 2),
                                            (12, 1024, 12, 40, 2), (12, 192, 96, 320, 2), (1, 128, 96, 320, 1),
                                            (2, 128, 7, 13, 2)])
def test_depthwise3x3_affine_relu_against_fp64(device, N, C, H, W, stride):
    """`ppea_dwconv3x3_fwd_affine_*` (stem[1], stem[3], transitions[.][1] + eval BatchNorm + ReLU) against an fp64 composite.
    Bounds: bf16 one rounding of the output (2^-7 of the output scale, as the other bf16 kernels here), fp32 2e-5."""
    from ppeadepth import ops
    g = _g(N + C + H + stride)
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3).to(device)
    s, o = (torch.rand(C, generator=g) + 0.5).to(device), (0.3 * torch.randn(C, generator=g)).to(device)
    x = torch.randn(N, C, H, W, generator=g).bfloat16().to(device)
    tab, xf = torch.stack([s, o]), x.float()
    for relu in (1, 0):
        ref = torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), None, stride, 1, 1, C)
        ref = ref * s.double().cpu().view(1, -1, 1, 1) + o.double().cpu().view(1, -1, 1, 1)
        ref = torch.relu(ref) if relu else ref
        y16, y32 = ops.dwconv3x3_affine(x, w, tab, relu, stride), ops.dwconv3x3_affine(xf, w, tab, relu, stride)
        torch.cuda.synchronize()
        assert y16.dtype == torch.bfloat16 and y32.dtype == torch.float32 and y16.shape == y32.shape == ref.shape
        e16, e32 = rel_err(y16.cpu(), ref), rel_err(y32.cpu(), ref)
        print(f"[{N},{C},{H}x{W}] stride {stride} relu {relu}: bf16 {e16:.3e} f32 {e32:.3e}")
        assert e16 <= 2 ** -7 and e32 <= 2e-5
    assert ops.dwconv3x3_affine(xf, w, tab, 1, 3) is None      # stride 3: PPEA_ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ---- end to end ---------------------------------------------------------------------------------------------------
def _build(device, H, W, B, rep_size="b", dc=False):
    from ppeadepth import networks, options
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, rep_size=rep_size, dc=dc)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    if dc:
        model.dc_ft_init()
    synth.fill_state_dict(model, conditioned=True)
    return model.to(device).train(), opt


def _run(p, data, device):
    d = {k: v.to(device) for k, v in data.items()}
    r = p.predict(d[("color", 0, 0)], d[("color", -1, 0)], d[("K", 2)], d[("inv_K", 2)], 0.1, 10.0)
    return r, p.predict_mono(d[("color", 0, 0)])


def _module_path(model, opt, data, device, amp):
    """The parent's path: model.eval() + Trainer.predict_disps -> scaled disparities."""
    from ppeadepth.trainer import Trainer
    tr = Trainer(opt, model, device, amp_dtype=amp)
    model.eval()
    try:
        d, m = tr.predict_disps({k: v.to(device) for k, v in data.items()})
    finally:
        model.train()
    return d.float(), m.float()


def _scaled(r, dm, opt):
    from ppeadepth.layers import disp_to_depth
    return disp_to_depth(r["disp"], 1e-3, 80)[0][:, 0], disp_to_depth(dm, 1e-3, opt.max_depth)[0][:, 0]


# share of quarter-resolution pixels whose winning depth bin may differ from the reference's (near-tie costs): the rule and
# the cap of tests/test_e2e_gpu.py for `lowest_cost`.  The CPU predictor alone differs at 0 pixels on the 64 x 96 fixture
# (tests/test_inference_cpu.py asserts equality).
TIE_CAP = 5e-3


@pytest.mark.parametrize("H,W,stride", [(64, 96, 1), (192, 640, 4)])
def test_fp32_predictor_matches_reference_golden_and_module_path(device, golden, H, W, stride):
    from ppeadepth.inference import DepthPredictor
    g = golden("infer")
    model, opt = _build(device, H, W, 2)
    data = synth.make_rendered_inputs(2, H, W)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    p = DepthPredictor(model, opt, amp_dtype=None)
    r, dm = _run(p, data, device)
    tag = f"{H}x{W}:"
    sub = lambda t: t[..., ::stride, ::stride].cpu()          # noqa: E731
    errs = {"disp": rel_err(sub(r["disp"]), g[tag + "disp"]), "disp_mono": rel_err(sub(dm), g[tag + "disp_mono"]),
            "pose": rel_err(r["pose"].cpu(), g[tag + "pose"])}
    low, glow = sub(r["lowest_cost"]), g[tag + "lowest_cost"]
    differ = float(((low - glow).abs() > 1e-5 * glow.abs().clamp_min(1e-6)).float().mean())
    print(f"fp32 predictor vs reference golden {tag} {errs} lowest_cost differs at {differ:.4%}")
    assert all(e <= TOL for e in errs.values()), errs
    assert differ <= TIE_CAP
    assert model.training and all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    d_mod, m_mod = _module_path(model, opt, data, device, None)
    d_p, m_p = _scaled(r, dm, opt)
    e = (rel_err(d_p, d_mod), rel_err(m_p, m_mod))
    print("fp32 predictor vs eval-mode module path:", e)
    assert max(e) <= FOLD_TOL


@pytest.mark.parametrize("B", [2, 12])
def test_bf16_predictor_is_no_worse_than_the_bf16_module_path(device, golden, B):
    """Error against fp32 (B = 2: the reference golden; B = 12: the fp32 predictor) <= 1.5 x the error of the existing
    bf16 eval path on the same inputs (the comparator rule of tests/test_e2e_gpu.py)."""
    from ppeadepth.inference import DepthPredictor
    H, W = 192, 640
    model, opt = _build(device, H, W, B)
    data = synth.make_rendered_inputs(B, H, W)
    r, dm = _run(DepthPredictor(model, opt), data, device)
    d_p, m_p = _scaled(r, dm, opt)
    d_mod, m_mod = _module_path(model, opt, data, device, torch.bfloat16)
    if B == 2:
        from ppeadepth.layers import disp_to_depth
        g = golden("infer")
        d_ref = disp_to_depth(g["192x640:disp"], 1e-3, 80)[0][:, 0].to(device)
        m_ref = disp_to_depth(g["192x640:disp_mono"], 1e-3, opt.max_depth)[0][:, 0].to(device)
        cut = lambda t: t[..., ::4, ::4]                       # noqa: E731
    else:
        r32, dm32 = _run(DepthPredictor(model, opt, amp_dtype=None), data, device)
        d_ref, m_ref = _scaled(r32, dm32, opt)
        cut = lambda t: t                                      # noqa: E731
    rec = {"B": B, "multi": {"predictor": rel_err(cut(d_p), d_ref), "module_path": rel_err(cut(d_mod), d_ref)},
           "mono": {"predictor": rel_err(cut(m_p), m_ref), "module_path": rel_err(cut(m_mod), m_ref)}}
    print("bf16 parity:", rec)
    # PPEA_PARITY_OUT=profiles pytest tests/test_inference_gpu.py -m gpu -k bf16_predictor   writes profiles/infer_parity.json
    out = os.environ.get("PPEA_PARITY_OUT")
    if out and os.path.isdir(out):
        path = os.path.join(out, "infer_parity.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.update(command="PPEA_PARITY_OUT=profiles pytest tests/test_inference_gpu.py -m gpu -k bf16_predictor",
                   shape="192x640 RepLKNet-31B, conditioned synthetic weights, rendered frames",
                   metric="rel_err (max abs / max abs) of the scaled disparity against fp32 (B=2: tests/golden/infer.npz; "
                          "B=12: the fp32 predictor)",
                   rule="predictor <= 1.5 x eval-mode module path under bf16 autocast")
        doc.setdefault("runs", {})[f"B{B}"] = rec
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
    for k in ("multi", "mono"):
        assert rec[k]["predictor"] <= 1.5 * rec[k]["module_path"], rec


def test_graph_replay_is_bitwise_the_eager_predictor(device):
    from ppeadepth.inference import DepthPredictor
    H, W, B = 192, 640, 2
    model, opt = _build(device, H, W, B)
    batches = [synth.make_rendered_inputs(B, H, W, seed=s) for s in (7, 8)]
    p = DepthPredictor(model, opt)
    eager = [_run(p, b, device) for b in batches]
    p.capture(B)
    assert set(p._graphs) == {("mono", (B, 3, H, W)), ("multi", (B, 3, H, W))}
    replays = []
    for g in p._graphs.values():                                 # count the replays: an eager fall-through must not pass
        inner = g["graph"]
        g["graph"] = type("Counted", (), {"replay": (lambda self, inner=inner: (replays.append(1), inner.replay())[1])})()
    replay = [_run(p, b, device) for b in batches] + [_run(p, batches[0], device)]
    for (r, dm), (re_, dme) in zip(replay, eager + eager[:1]):
        assert torch.equal(dm, dme)
        for k in ("disp", "lowest_cost", "pose"):
            assert torch.equal(r[k], re_[k]), k
    assert not torch.equal(eager[0][1], eager[1][1])
    assert len(replays) == 6                                     # 3 x (predict + predict_mono), every one a graph replay


# the pattern of test_bf16_step_launches_no_library_convolution_or_gemm (tests/test_e2e_gpu.py), extended with batch_norm
LIBRARY = re.compile(r"Cijk_|igemm|ck::|ck_tile|miopen|MIOpen|naive_conv|SubTensorOp|gemm_|Gemm|wmma|batched_transpose|"
                     r"batch_norm|rocblas|hipblaslt")


@pytest.mark.parametrize("rep_size,dc", [("b", False), ("l", False), ("b", True)])
def test_bf16_prediction_launches_no_library_kernel_and_stays_inside_the_launch_budget(device, rep_size, dc):
    from torch.profiler import ProfilerActivity, profile
    from ppeadepth.inference import DepthPredictor
    H, W, B = 192, 640, 2
    model, opt = _build(device, H, W, B, rep_size, dc)
    data = synth.make_rendered_inputs(B, H, W)
    p = DepthPredictor(model, opt)
    _run(p, data, device)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        _run(p, data, device)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name]
    assert len(set(names)) > 20, "the profiler recorded no device kernels"
    hits = [n for n in names if LIBRARY.search(n)]
    gemms = [n for n in hits if "Cijk_" in n]
    others = sorted(set(n for n in hits if "Cijk_" not in n))
    print(f"[{rep_size}, dc={dc}] device kernels {len(names)}, pose-algebra GEMMs {len(gemms)}, other library {others}")
    assert not others, others
    assert len(gemms) <= 16, sorted(set(gemms))                  # pose algebra only
    # launch budget of the trunk: pw1, depthwise, pw2 (3) + conv adapter (3) + FFN pw1, pw2 (2) + MLP adapter (2) = 10 per
    # block pair, <= 12 asked.  Two encoder passes (teacher + multi-frame; the matching encoder's stem and stage 0 run once
    # on a 2B batch): 48 pairs.  Counted by kernel name (GEMM, depthwise, table-apply, tap-sum kernels); the count also holds
    # the stems' and transitions' 1x1 convs and table launches, so it is an upper bound per pair.  Floor: a name pattern that
    # stops matching must not pass.
    trunk = [n for n in names if re.search(r"pwconv|dwconv_mfma|dwconv_bm|dwconv_lk|dwconv_generic|bn_apply|tapsum", n)]
    print(f"    trunk kernels {len(trunk)} = {len(trunk) / 48:.2f} per block pair")
    assert 9 * 48 <= len(trunk) <= 12 * 48


def test_val_with_predictor_reproduces_the_absrel_golden(device, golden, tmp_path):
    """`Trainer.val(..., predictor=p)` fp32 on the synthetic eigen split of tests/golden/eval.npz: AbsRel within 1e-3."""
    from ppeadepth import networks, options
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.trainer import Trainer
    g = golden("eval")
    n, H, W, seed = [int(v) for v in g["val_meta"]]
    opt = options.default_options(height=H, width=W, batch_size=n, use_checkpoint=False)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model)
    model.to(device).train()
    synth.make_eval_split(str(tmp_path), n=n, height=H, width=W, seed=seed, split="eigen")
    ds = synth.SynthEigenDataset(str(tmp_path), split="eigen", height=H, width=W)
    batch, gt = synth.collate([ds[i] for i in range(n)]), ds.gt_depths()
    tr = Trainer(opt, model, device)
    errors, errors_mono = tr.val([batch], gt, "eigen", predictor=DepthPredictor(model, opt, amp_dtype=None))
    print("AbsRel", errors[0], float(g["val_errors"][0]), errors_mono[0], float(g["val_errors_mono"][0]))
    assert abs(errors[0] - float(g["val_errors"][0])) <= 1e-3
    assert abs(errors_mono[0] - float(g["val_errors_mono"][0])) <= 1e-3
    assert model.training


@pytest.mark.parametrize("rep_size,dc,extra", [("l", False, {}), ("b", True, {}),
                                               ("b", False, dict(trans=True, input=True, mono_trans=True, mono_input=True))])
def test_fp32_predictor_matches_module_path_for_other_configurations(device, rep_size, dc, extra):
    """--rep_size l, --dc and --trans / --input / --mono_trans / --mono_input: fp32 predictor vs the eval-mode module path."""
    from ppeadepth import networks, options
    from ppeadepth.inference import DepthPredictor
    H, W, B = 64, 96, 2
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=False, rep_size=rep_size, dc=dc, **extra)
    torch.manual_seed(0)
    model = networks.RepDepth(opt)
    if dc:
        model.dc_ft_init()
    synth.fill_state_dict(model, conditioned=True)
    model.to(device).train()
    if extra:
        assert model.encoder.replk.input_adpt and model.mono_encoder.trans_adpt is not False
    data = synth.make_rendered_inputs(B, H, W)
    r, dm = _run(DepthPredictor(model, opt, amp_dtype=None), data, device)
    d_mod, m_mod = _module_path(model, opt, data, device, None)
    d_p, m_p = _scaled(r, dm, opt)
    e = (rel_err(d_p, d_mod), rel_err(m_p, m_mod))
    print(f"[{rep_size}, dc={dc}, {sorted(extra)}] fp32 predictor vs module path: {e}")
    assert max(e) <= FOLD_TOL


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_training_step_still_runs_after_a_predictor_was_used(device, amp):
    """Build, refresh and run a predictor (and capture it for bf16) on a live training model: state_dict bit-identical,
    every module's mode unchanged, and a training-mode process_batch + backward afterwards runs and is finite."""
    from ppeadepth import rng
    from ppeadepth.inference import DepthPredictor
    from ppeadepth.trainer import Trainer
    H, W, B = 64, 96, 2
    model, opt = _build(device, H, W, B)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    modes = [m.training for m in model.modules()]
    data = synth.make_rendered_inputs(B, H, W)
    p = DepthPredictor(model, opt, amp_dtype=amp)
    p.refresh()
    _run(p, data, device)
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert [m.training for m in model.modules()] == modes and model.training
    rng.set_mode("device")
    tr = Trainer(opt, model, device, amp_dtype=amp)
    outputs, losses = tr.process_batch({k: v.to(device) for k, v in data.items()}, True)
    losses["loss"].backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses["loss"]))
    grads = [q.grad for q in model.parameters() if q.requires_grad and q.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    # ... and the predictor follows the step's new running statistics after refresh()
    p.refresh()
    r2, _ = _run(p, data, device)
    assert bool(torch.isfinite(r2["disp"]).all())
