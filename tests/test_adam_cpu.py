"""The Adam reference (oracle/ref_ops.py::adam_step, float64) against torch.optim.Adam, and the per-element error bounds
every fp32 Adam step of this repository is held to (tests/test_adam_gpu.py: the flat kernel; tests/test_optimizer_phase_gpu.py:
the engine's optimizer phase).  No GPU here: a plain fp32 evaluation of the formula with torch's CPU operators stands in for
the kernel and shows that a correct fp32 implementation meets the bounds.

Protocol (shared with the GPU tests).  ONE step at a time: the fp32 state (p, m, v) before the step, the fp32 gradient and the
host's t and lr go into the float64 reference; the fp32 state after the step is compared with it element by element.  Nothing
drifts between steps.  The hyper-parameters go in at the fp32 values the C ABI carries (float(0.999) differs from 0.999 by
1.3e-5 of 1 - b2).

Bounds.  First-order rounding analysis of the documented operation order (csrc/adam.hip, torch's order)

    g' = g * gscale
    m' = m + (1 - b1) * (g' - m)                             lerp(m, g', 1 - b1)
    v' = b2 * v + ((1 - b2) * g') * g'
    bc1 = 1 - powf(b1, t);  bc2 = 1 - powf(b2, t);  step = lr / bc1;  sq = sqrtf(bc2)
    p' = p - (step * m') / (sqrtf(v') / sq + eps)

with u = 2^-24 the relative error of one correctly rounded fp32 operation.  1 - b1 and 1 - b2 are exact for b in [0.5, 1]
(Sterbenz).  No accuracy table of the HIP math functions ships with the toolkit, so the figures ASSUMED here are those of the
public HIP math API documentation: powf and sqrtf within 1 ulp (a relative error of at most 2u); the division is IEEE
(correctly rounded, u): the library is built without fast-math.

  m:  u c1 |g'|  (rounding of g')  +  u c1 (|g'| + |m|)  (the difference)  +  u c1 (|g'| + |m|)  (the product)  +  u |m'|
      (the sum), with c1 = 1 - b1 and |m'| <= |m| + |g'|:  (1 + 3 c1) u (|m| + |g'|) = 1.3 u (|m| + |g'|) at b1 = 0.9.
      The form b1 m + c1 g' gives (1 + b1 + 2 c1) u at most.  K_M = 2 covers both and the second-order terms.
      (Relative to |m'| alone the error is unbounded: g' - m cancels.)
  v:  all terms are positive.  u on b2 v;  2u (g' enters twice) + 2u (two products) on the second term;  u on the sum:
      at most 5u v'.  K_V = 6 with the second-order terms.
  p:  u max(|p|, |p'|) for the final subtraction (half an ulp of p'), plus the error of the update U = step m' / D,
      D = sqrt(v') / sq + eps:
        |U| * [ 3u (lr, step * m', and the sum in D)  +  3u (three divisions)  +  2u (sqrtf(v'))  +  K_V u / 2 (v' under the
                root)  +  e_bc1  +  e_bc2 / 2 + 2u (sqrtf(bc2)) ]
      with e_bc = u + 2u b^t / (1 - b^t): powf's error 2u b^t is absolute in 1 - b^t, the cancellation multiplies it by
      b^t / (1 - b^t) ~ 1 / (t (1 - b)) at small t (999 for b2 at t = 1, 9 for b1).  In all
        |U| * (14.5 + 2 r1 + r2) u,   r_i = b_i^t / (1 - b_i^t),
      plus the error of m' carried through:  step * K_M u (|m| + |g'|) / D.
Every bound has the absolute floor 2^-126 (flushing a subnormal is not a finding) and the factor 1 + 2^-10 for the terms of
second order.  The multiples come from this analysis, not from any implementation's measured error; the fp32 evaluation
below measures at most 0.47 (m) and 0.45 (v) of them, and 0.996 for p: half an ulp of p is reached whenever p sits just above
a power of two and the update is far below its ulp, so that term has no slack by construction.
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import ref_ops as R

U = 2.0 ** -24
FLOOR = 2.0 ** -126
K_M, K_V = 2.0, 6.0
POW_ERR = SQRT_ERR = 2.0 * U         # 1 ulp (assumed, see above)
DIV_ERR = U                          # IEEE division


def f32(x):
    """The value an fp32 argument of the C ABI carries, as a Python float."""
    return float(np.float32(x))


HYPER = dict(b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8))          # torch.optim.Adam's defaults (trainer.py:142)
# (t, lr) of the launches of one run: a carried sequence, then step numbers written directly; every rate at a small t too
PLAN = [(1, 1e-3), (2, 1e-3), (3, 1e-4), (4, 1e-6), (10, 1e-3), (1000, 1e-4), (100000, 1e-6)]
SPECIALS = [0.0, 1e-40, -1e-40, 3e38, -3e38, math.inf, -math.inf, math.nan]


def initial_p(n, seed):
    """Magnitudes from 1e-8 to 1: where |p| is small the bound is the update's, not half an ulp of p."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * 10.0 ** (-8.0 * torch.rand(n, generator=g))


def gradient(n, seed, step):
    """randn * 10^U, U uniform in [-12, 4]: sqrt(v) from far below eps to far above it."""
    g = torch.Generator().manual_seed(1000 * seed + step)
    return torch.randn(n, generator=g) * 10.0 ** (16.0 * torch.rand(n, generator=g) - 12.0)


def plant_specials(g, n):
    """At most 8 special values, each in a float4 group of its own with ordinary lanes beside it -> their indices."""
    n4 = n // 4
    k = min(len(SPECIALS), n4)
    idx = []
    for j in range(k):
        i = 4 * (j * max(1, n4 // k)) + (j + n) % 4
        g[i] = SPECIALS[(j + n) % len(SPECIALS)]
        idx.append(i)
    return torch.tensor(idx, dtype=torch.long)


def adam_bounds(p0, g, m0, v0, t, lr, b1, b2, eps, gscale=1.0):
    """-> (p, m, v) of the float64 reference and the per-element bounds (bp, bm, bv) of the module docstring."""
    p, m, v = R.adam_step(p0, g, m0, v0, t, lr, b1, b2, eps, gscale)
    second = 1.0 + 2.0 ** -10
    ga = (g.double() * gscale).abs()
    bm = (second * K_M * U * (m0.double().abs() + ga)).clamp_min(FLOOR)
    bv = (second * K_V * U * v).clamp_min(FLOOR)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    r1, r2 = b1 ** t / bc1, b2 ** t / bc2
    rel_upd = (14.5 + 2.0 * r1 + r2) * U
    assert abs(rel_upd - (3 * U + 3 * DIV_ERR + SQRT_ERR + K_V * U / 2 + (U + POW_ERR * r1) + (U + POW_ERR * r2) / 2 + SQRT_ERR)) \
        < 1e-3 * rel_upd
    step = lr / bc1
    denom = v.sqrt() / math.sqrt(bc2) + eps
    upd = step * m / denom
    bp = second * (U * torch.maximum(p0.double().abs(), p.abs()) + upd.abs() * rel_upd + step * bm / denom)
    return (p, m, v), (bp.clamp_min(FLOOR), bm, bv)


def check_step(got, p0, g, m0, v0, t, lr, gscale=1.0, skip=None, what="", hyper=None):
    """got = (p, m, v) after one step from (p0, m0, v0); every element outside `skip` within its bound (computed on the
    device that holds p0).  -> the largest error / bound of p, m, v."""
    ref, bounds = adam_bounds(p0, g, m0, v0, t, lr, gscale=gscale, **(hyper or HYPER))
    keep = torch.ones(p0.numel(), dtype=torch.bool, device=p0.device)
    if skip is not None and len(skip):
        keep[skip] = False
    ratios = []
    for name, a, r, b in zip("pmv", got, ref, bounds):
        a = a.detach().to(p0.device).double()
        assert bool(torch.isfinite(a[keep]).all()), (what, name, t)
        err = (a - r).abs()[keep]
        ratio = err / b[keep]
        worst = int(ratio.argmax()) if ratio.numel() else 0
        ratios.append(float(ratio[worst]) if ratio.numel() else 0.0)
        assert ratios[-1] <= 1.0, (what, name, "t", t, "lr", lr, "element", int(keep.nonzero()[worst]), "error", float(err[worst]),
                                   "bound", float(b[keep][worst]), "ratio", ratios[-1])
    return ratios


def adam_step_f32(p, g, m, v, t, lr, b1, b2, eps, gscale=1.0, eps_inside=False, t_shift=0.0):
    """The formula of the module docstring with torch's CPU fp32 operators, every scalar an fp32 value.
    eps_inside / t_shift: two WRONG variants (eps on the wrong side of the bias correction; t - 1 in the corrections)."""
    s = lambda x: torch.tensor(x, dtype=torch.float32)
    g = g * s(gscale)
    m = torch.lerp(m, g, s(1.0) - s(b1))
    v = s(b2) * v + ((s(1.0) - s(b2)) * g) * g
    bc1 = s(1.0) - torch.pow(s(b1), s(t - t_shift))
    bc2 = s(1.0) - torch.pow(s(b2), s(t - t_shift))
    step, sq = s(lr) / bc1, bc2.sqrt()
    denom = (v.sqrt() + s(eps)) / sq if eps_inside else v.sqrt() / sq + s(eps)
    return p - (step * m) / denom, m, v


def same_class(a, b):
    """NaN / +inf / -inf / finite, element by element."""
    return bool(((a.isnan() == b.isnan()) & (a.isposinf() == b.isposinf()) & (a.isneginf() == b.isneginf())).all())


def test_reference_equals_torch_adam_in_float64():
    """Six steps, StepLR(optimizer, 2, 0.1), the reference's constructor arguments (lr only): p, exp_avg and exp_avg_sq."""
    gen = torch.Generator().manual_seed(0)
    n = 1000
    w = torch.randn(n, generator=gen, dtype=torch.float64).requires_grad_(True)
    opt = torch.optim.Adam([w], lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.1)
    group = opt.param_groups[0]
    p, m, v = w.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    lrs = []
    for t in range(1, 7):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** (16.0 * torch.rand(n, generator=gen) - 12.0).double()
        lrs.append(group["lr"])
        p, m, v = R.adam_step(p, g, m, v, t, group["lr"], *group["betas"], group["eps"])
        w.grad = g.clone()
        opt.step()
        sched.step()
        st = opt.state[w]
        assert int(st["step"]) == t
        assert rel_err(p, w.detach()) <= 1e-14 and rel_err(m, st["exp_avg"]) <= 1e-14 and rel_err(v, st["exp_avg_sq"]) <= 1e-14, t
        # element by element too (max-abs would hide the small entries): 1e-14 of each value
        for a, b in ((m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert bool(((a - b).abs() <= 1e-14 * b.abs()).all()), t
    assert [round(math.log10(x)) for x in lrs] == [-3, -3, -4, -4, -5, -5]


def _run_f32(n, seed, **wrong):
    """The PLAN with the fp32 evaluation in the kernel's place -> largest error / bound of p, m, v over the run."""
    p, m, v = initial_p(n, seed), torch.zeros(n), torch.zeros(n)
    worst = [0.0, 0.0, 0.0]
    for k, (t, lr) in enumerate(PLAN):
        g = gradient(n, seed, k)
        special = plant_specials(g, n)
        got = adam_step_f32(p, g, m, v, float(t), f32(lr), **HYPER, **wrong)
        if wrong:
            ref, bounds = adam_bounds(p, g, m, v, t, lr, **HYPER)
            keep = torch.ones(n, dtype=torch.bool)
            keep[special] = False
            ratio = ((got[0].double() - ref[0]).abs() / bounds[0])[keep]
            worst[0] = max(worst[0], float(ratio.nan_to_num(nan=math.inf).max()))
        else:
            worst = [max(a, b) for a, b in zip(worst, check_step(got, p, g, m, v, t, lr, skip=special, what=f"fp32 n={n}"))]
        p, m, v = got
    return worst


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, 65539])
def test_a_correct_fp32_evaluation_meets_the_bounds(n):
    """The bounds are attainable: the formula in fp32 on the step-by-step inputs of tests/test_adam_gpu.py (same sizes, same
    plan of t and lr, same gradients, same planted specials) stays inside them, with room."""
    worst = _run_f32(n, seed=n)
    print(f"n={n}: fp32 evaluation, largest error / bound  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    assert max(worst) <= 1.0


@pytest.mark.parametrize("wrong", [dict(eps_inside=True), dict(t_shift=1.0)], ids=["eps_inside", "t_minus_1"])
def test_the_bounds_reject_a_wrong_formula(wrong):
    """... and they are tight enough to tell: eps on the wrong side of the bias correction, or t - 1 in the corrections,
    leaves p outside its bound by orders of magnitude."""
    assert _run_f32(1027, seed=1027, **wrong)[0] > 100.0
