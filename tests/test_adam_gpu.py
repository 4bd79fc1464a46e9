"""`adam_flat_kernel` (csrc/adam.hip) at its edges, through both entry points (ppea_adam_flat_f32, ppea_adam_flat_scaled_f32),
against the float64 Adam of oracle/ref_ops.py::adam_step.

Protocol, inputs and bounds are those of tests/test_adam_cpu.py (derivation in its module docstring; a plain fp32 evaluation
of the formula meets them there):  ONE step at a time -- the fp32 P, M, V before the launch, the gradient and the HOST's t and
lr go into the float64 reference, P, M, V after the launch are compared with it element by element:

    |m - m_ref| <= 2 u (|m_prev| + |g gscale|)          u = 2^-24
    |v - v_ref| <= 6 u v_ref
    |p - p_ref| <= u max(|p_prev|, |p_ref|) + |update| (14.5 + 2 r1 + r2) u + step 2u (|m_prev| + |g gscale|) / denom
                   r_i = b_i^t / (1 - b_i^t): powf's assumed 1 ulp through the cancellation in 1 - b^t (r2 = 999 at t = 1)

each with the floor 2^-126 and the factor 1 + 2^-10.  Gradients are randn * 10^U, U in [-12, 4] (eps from dominant to
negligible), |p| from 1e-8 to 1, M and V carried from the previous launches.  Up to 8 special gradient values (0, +-1e-40,
+-3e38, +-inf, NaN), each alone in a float4 group, are compared by class with the fp32 CPU evaluation and left out of the
bounds; their neighbours are not.

Sizes: n in {1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027} and 8192 * 1024 + 1203 (the launch is capped at 8192 blocks of 256
threads x 4 elements: 300 threads take a second grid-stride trip, 3 elements go to the tail); per n every valid n_lo of
{0 with w16 NULL, 0 with w16 given, 1, 2, 3, 5, n - 1, n}.  P, M and V do not depend on n_lo, nor on the entry point once the
gradients are pre-scaled: every variant starts from the same state and must reproduce the first one bit for bit, so one float64
pass per step serves them all.  Every buffer has 64 sentinel elements on both sides of the (16-byte aligned) region the kernel is
handed, W16 holds sentinels beyond n_lo as well, and all of them must come back unchanged.  After every launch W16[:n_lo] is
torch's CPU rounding of the new P[:n_lo], bit for bit (a NaN only has to be a NaN: `_same_bf16`).

Largest error / bound measured on MI355X over all sizes: p 0.994, m 0.514, v 0.737 ("Optimizer phase").
"""
import math

import pytest
import torch

from test_adam_cpu import (FLOOR, HYPER, PLAN, adam_step_f32, check_step, f32, gradient, initial_p, plant_specials,
                           same_class)

pytestmark = pytest.mark.gpu

GUARD = 64
SENT32, SENT16 = 0x5EA7BEEF, 0x5A5A
GSCALE = f32(1.0 / 3.0)              # 1 / world of three ranks: the product g * gscale rounds
BIG = 8192 * 1024 + 1203


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bf16(w, expect):
    """Bit for bit, except that a NaN only has to be a NaN: it has no rounding, and torch's own conversions do not agree on
    its encoding (the CPU's vectorised one returns 0xFFFF, the scalar one 0x7FC0; the kernel keeps sign and quiet bit)."""
    nan = expect.isnan()
    return bool((w.isnan() == nan).all()) and torch.equal(_bits(w)[~nan], _bits(expect)[~nan])


class _Buffers:
    """P, G, M, V fp32 [n] and W16 bf16 [n], each a 16-byte aligned view with GUARD sentinel elements on both sides."""

    def __init__(self, device, n):
        self.n = n
        self.raw = {k: torch.full((GUARD + n + GUARD,), SENT32, dtype=torch.int32, device=device) for k in "PGMV"}
        self.raw16 = torch.full((GUARD + n + GUARD,), SENT16, dtype=torch.int16, device=device)
        self.P, self.G, self.M, self.V = (self.raw[k].view(torch.float32)[GUARD:GUARD + n] for k in "PGMV")
        self.W = self.raw16.view(torch.bfloat16)[GUARD:GUARD + n]
        for t in (self.P, self.G, self.M, self.V, self.W):
            assert t.data_ptr() % 16 == 0 and t.is_contiguous()

    def load(self, p, g, m, v):
        self.P.copy_(p), self.G.copy_(g), self.M.copy_(m), self.V.copy_(v)
        self.raw16.fill_(SENT16)

    def assert_guards(self, written16, what):
        for k, raw in self.raw.items():
            assert bool((raw[:GUARD] == SENT32).all()) and bool((raw[GUARD + self.n:] == SENT32).all()), (what, k)
        assert bool((self.raw16[:GUARD] == SENT16).all()) and bool((self.raw16[GUARD + written16:] == SENT16).all()), (what, "W16")


def _launch(buf, scaled, n_lo, has_w, state):
    from ppeadepth._abi import call, ptr, stream_ptr
    args = [ptr(buf.P), ptr(buf.G), ptr(buf.M), ptr(buf.V), ptr(buf.W) if has_w else None, buf.n, n_lo, ptr(state),
            HYPER["b1"], HYPER["b2"], HYPER["eps"]]
    if scaled:
        call("ppea_adam_flat_scaled_f32", *args, GSCALE, stream_ptr())
    else:
        call("ppea_adam_flat_f32", *args, stream_ptr())


def _variants(n):
    """(scaled entry?, n_lo, w16 given?) -- the first one is the variant the float64 reference is compared with."""
    cuts = [(n, True), (0, False), (0, True)] + [(k, True) for k in (1, 2, 3, 5, n - 1) if 0 < k < n]
    cuts = list(dict.fromkeys(cuts))
    return [(scaled, n_lo, has_w) for scaled in (True, False) for n_lo, has_w in cuts]


def _run_plan(device, n, plan, check_from=0):
    """Every launch of `plan` in every variant.  -> largest error / bound of p, m, v."""
    buf = _Buffers(device, n)
    p, m, v = initial_p(n, n).to(device), torch.zeros(n, device=device), torch.zeros(n, device=device)
    state = torch.tensor([0.0, plan[0][1]], device=device)
    worst = [0.0, 0.0, 0.0]
    for k, (t, lr) in enumerate(plan):
        g = gradient(n, n, k)
        special = plant_specials(g, n)
        gd = g.to(device)
        gpre = gd * GSCALE                              # what a separate scaling pass would have stored
        if k < 4:
            state[0] += 1                                # as TrainEngine._flat_adam_step counts
        else:
            state[0].fill_(float(t))
        state[1].fill_(lr)
        assert float(state[0]) == t
        first = exp16 = None
        for scaled, n_lo, has_w in _variants(n):
            what = f"n={n} t={t} lr={lr} {'scaled' if scaled else 'plain'} n_lo={n_lo} w16={'given' if has_w else 'NULL'}"
            src = gd if scaled else gpre
            buf.load(p, src, m, v)
            _launch(buf, scaled, n_lo, has_w, state)
            torch.cuda.synchronize()
            buf.assert_guards(n_lo, what)
            assert torch.equal(_bits(buf.G), _bits(src)), what
            if first is None:
                first = (buf.P.clone(), buf.M.clone(), buf.V.clone())
                host = [x.cpu() for x in first]
                exp16 = host[0].bfloat16().to(device)               # torch's CPU rounding of the new masters
                p0, m0, v0 = p.cpu(), m.cpu(), v.cpu()
                if k >= check_from:
                    r = check_step(host, p0, g, m0, v0, t, lr, gscale=GSCALE, skip=special, what=what)
                    worst = [max(a, b) for a, b in zip(worst, r)]
                    # the plain entry on pre-scaled gradients returns these very bits (asserted below): its own reference
                    if n <= 4096:                            # (one float64 pass is enough at the large size)
                        r = check_step(host, p0, gpre.cpu(), m0, v0, t, lr, skip=special, what=what + " (as plain)")
                        worst = [max(a, b) for a, b in zip(worst, r)]
                if len(special):
                    cls = adam_step_f32(p0[special], g[special], m0[special], v0[special], float(t), f32(lr), gscale=GSCALE, **HYPER)
                    for a, b in zip(host, cls):
                        assert same_class(a[special], b), (what, a[special], b)
            else:
                for name, a, b in zip("PMV", (buf.P, buf.M, buf.V), first):
                    assert torch.equal(_bits(a), _bits(b)), (what, name)
            if has_w and n_lo:
                assert _same_bf16(buf.W[:n_lo], exp16[:n_lo]), what
        p, m, v = first
    return worst


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027])
def test_adam_flat_edge_sizes_against_float64(device, n):
    """t = 1..4 carried, then t = 10, 1000, 100000 written into state[0]; lr 1e-3, 1e-4, 1e-6 changed in state[1] between
    launches; every n_lo cut and both entry points at every launch."""
    worst = _run_plan(device, n, PLAN)
    print(f"n={n}: kernel, largest error / bound  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")


def test_adam_flat_second_grid_stride_trip_and_tail(device):
    """n = 8192 * 1024 + 1203, the path every real flat buffer takes: the 8192-block cap makes 300 threads loop a second time
    and the last 3 elements go to the tail.  Step 1 builds non-zero moments (bit identity across the variants, guards and
    working copy only), step 2 is compared with float64."""
    worst = _run_plan(device, BIG, [(1, 1e-3), (2, 1e-4)], check_from=1)
    print(f"n={BIG}: kernel, largest error / bound  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", [1, 3, 6, 1027])
def test_zero_gradient_on_zero_moments_changes_nothing(device, n, scaled):
    buf = _Buffers(device, n)
    p = initial_p(n, 3 * n).to(device)
    zero = torch.zeros(n, device=device)
    state = torch.tensor([1.0, 1e-3], device=device)
    buf.load(p, zero, zero, zero)
    _launch(buf, scaled, n, True, state)
    torch.cuda.synchronize()
    buf.assert_guards(n, n)
    assert torch.equal(_bits(buf.P), _bits(p))
    assert torch.equal(_bits(buf.M), _bits(zero)) and torch.equal(_bits(buf.V), _bits(zero))
    assert torch.equal(_bits(buf.W.cpu()), _bits(p.cpu().bfloat16()))


def test_working_copy_rounds_as_torch_does(device):
    """g = 0 on zero moments leaves P alone, so W16 is the rounding of planted values: bf16 round-to-nearest-even ties in both
    directions and their neighbours, a finite value above bf16's largest, signed zeros, subnormals, infinities and NaN -- in
    float4 groups and in the scalar tail."""
    n = 1027
    t2 = 2.0 ** -8                                       # half a bf16 ulp at 1.0
    plant = [1 + t2, 1 + 3 * t2, -(1 + t2), -(1 + 3 * t2), 1 + t2 + 2.0 ** -23, 1 + t2 - 2.0 ** -23, 1 + 3 * t2 - 2.0 ** -23,
             3.4e38, -3.4e38, 0.0, -0.0, 1e-40, -1e-40, math.inf, -math.inf, math.nan]
    expect = [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x3F81, 0x7F80, 0xFF80, 0x0000, 0x8000]     # the first eleven
    where = [5 * i + 2 for i in range(len(plant) - 3)] + [1024, 1025, 1026]                           # the tail holds three
    p = initial_p(n, 77)
    p[where] = torch.tensor(plant)
    buf = _Buffers(device, n)
    zero = torch.zeros(n, device=device)
    state = torch.tensor([1.0, 1e-3], device=device)
    buf.load(p.to(device), zero, zero, zero)
    _launch(buf, False, n, True, state)
    torch.cuda.synchronize()
    buf.assert_guards(n, "planted P")
    after = buf.P.cpu()
    normal = ~((p != 0) & (p.abs() < FLOOR))             # (a flushed subnormal is not a finding)
    assert torch.equal(_bits(after)[normal], _bits(p)[normal])
    assert _same_bf16(buf.W.cpu(), after.bfloat16())
    assert bool(buf.W[where[-1]].isnan()) and bool(after[where[-1]].isnan())
    w = _bits(buf.W.cpu())
    got = [int(x) & 0xFFFF for x in w[where[:len(expect)]]]
    assert got == expect, [hex(x) for x in got]


def test_captured_launch_reads_the_device_scalars(device):
    """One launch captured on a side stream and replayed three times with `state` and the gradient buffer changed in place
    between the replays == the eager sequence, bit for bit: t and lr are read from the device at run time, not frozen into
    the graph."""
    n, n_lo = 1027, 5
    steps = [(1, 1e-3), (2, 1e-4), (100000, 1e-6)]
    p = initial_p(n, 9).to(device)
    zero = torch.zeros(n, device=device)
    grads = [gradient(n, 9, k).to(device) for k in range(len(steps))]
    res = []
    for captured in (False, True):
        buf = _Buffers(device, n)
        buf.load(p, zero, zero, zero)
        state = torch.tensor([0.0, 0.0], device=device)
        graph = None
        if captured:
            side = torch.cuda.Stream(device)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                _launch(buf, True, n_lo, True, state)
            torch.cuda.synchronize()
            assert torch.equal(_bits(buf.P), _bits(p))   # capturing runs nothing
        for (t, lr), g in zip(steps, grads):
            state[0].fill_(float(t))
            state[1].fill_(lr)
            buf.G.copy_(g)
            if captured:
                torch.cuda.synchronize()
                graph.replay()
            else:
                _launch(buf, True, n_lo, True, state)
            torch.cuda.synchronize()
        buf.assert_guards(n_lo, "graph" if captured else "eager")
        res.append([x.clone() for x in (buf.P, buf.M, buf.V, buf.W[:n_lo])])
    assert not torch.equal(_bits(res[0][0]), _bits(p))
    for name, a, b in zip(("P", "M", "V", "W16"), *res):
        assert torch.equal(_bits(a), _bits(b)), name
