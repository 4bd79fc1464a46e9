"""Every instantiation of the plane-sweep kernel cost_volume_fwd<F, DB, PK, RING> (csrc/cost_volume.hip) through its raw entry
point against the float64 reference of oracle/cv_inputs.py, element by element, each element held to the bound derived there
(tests/test_cv_arms_cpu.py proves the reference, the cap on undecided entries and that the bound catches index, mask and
count faults).  The cost is a NaN-filled view into a guarded buffer, the bf16 pair workspace and the rings are guarded too: an
entry never stored is outside its bound, a store past either end changes a guard.  One upload and one launch per row and
entry point.  Ring rows also equal, bit for bit, the multi entry on the gathered frames.  Then the ring's store and advance
kernels on state words that are out of range, and every refusal of the file as a return code."""
import functools

import pytest
import torch

from oracle import cv_inputs as V

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
UNSUPPORTED, BAD_ARG = -1, -2


def _ids(rows):
    return [r.name for r in rows]


@functools.lru_cache(maxsize=None)
def _numerics(name):
    r = V.BY_NAME[name]
    inp = V.make_inputs(r)
    return r, inp, V.reference(r, inp)


def _words(t, device):
    """int32 host tensor -> a guarded device buffer holding those dwords: (buffer, int32 view)."""
    buf, body = V.guarded(tuple(t.shape), F32, device)
    body.view(I32).copy_(t.to(device))
    return buf, body.view(I32)


def _multi(ops, r, d, look, skip, bufs, device):
    """The multi entry on uploaded operands `d` -> the guarded cost."""
    buf, cost = V.guarded((r.B, r.D, r.h, r.w), F32, device)
    bufs.append(buf)
    tail = (ops.ptr(d["P"]), ops.ptr(d["inv_K"]), ops.ptr(d["bins"]), ops.ptr(skip), ops.ptr(cost), r.B, r.F, r.C, r.h, r.w, r.D,
            float(r.eps), ops.stream_ptr())
    if r.dtype == "bf16":
        n = r.B * (r.C // 2) * r.h * r.w
        pbuf, pairs = V.guarded(((1 + r.F) * n,), F32, device)
        bufs.append(pbuf)
        ops.call("ppea_cost_volume_multi_fwd_bf16", ops.ptr(d["cur"]), ops.ptr(look), ops.ptr(pairs), *tail)
        want = torch.cat([V.pack_pairs(d["cur"].cpu()).reshape(-1), V.pack_pairs(look.cpu()).reshape(-1)])
        assert torch.equal(pairs.view(I32).cpu(), want), "the pair workspace is not the packed inputs"
    else:
        ops.call("ppea_cost_volume_multi_fwd_f32", ops.ptr(d["cur"]), ops.ptr(look), *tail)
    return cost


@pytest.mark.parametrize("r", V.ROWS, ids=_ids(V.ROWS))
def test_rows(device, r):
    """Measured on an MI355X: worst err / bound 0.054 .. 0.124 on the 16 generic rows (the position term (b) of the bound
    dominates: largest error 1.1e-05 .. 3.5e-05 at costs near 2.2), 0.177 at most elsewhere; exact rows 0.165 .. 0.395 with a
    largest error of 3.4e-07 .. 7.6e-07 (one to three fp32 roundings of a cost near 2.4); no entry undecided or left out; every
    entry of every row has the bits of the fp32 emulation (the table per instantiation: DESIGN.md, "Several lookup frames")."""
    from ppeadepth import ops
    _, inp, ref = _numerics(r.name)
    d = {k: inp[k].to(device).contiguous() for k in ("cur", "look", "P", "inv_K", "bins", "skip")}
    bufs = []
    if r.form == "multi":
        cost = _multi(ops, r, d, d["look"], d["skip"], bufs, device)
    else:
        state = inp["state"].to(device)
        skip_arg = None if inp["skip_arg"] is None else inp["skip_arg"].to(device)
        buf, cost = V.guarded((r.B, r.D, r.h, r.w), F32, device)
        bufs.append(buf)
        if r.dtype == "bf16":
            cur = V.pack_pairs(inp["cur"]).to(device)
            rbuf, ring = _words(V.pack_pairs(inp["ring"]), device)
            name = "ppea_cost_volume_ring_fwd_bf16"
        else:
            cur = d["cur"]
            rbuf, ring = V.guarded(tuple(inp["ring"].shape), F32, device)
            ring.copy_(inp["ring"].to(device))
            name = "ppea_cost_volume_ring_fwd_f32"
        bufs.append(rbuf)
        before = ring.clone()
        ops.call(name, ops.ptr(cur), ops.ptr(ring), ops.ptr(state), ops.ptr(d["P"]), ops.ptr(d["inv_K"]), ops.ptr(d["bins"]),
                 ops.ptr(skip_arg), ops.ptr(cost), r.B, r.F, r.C, r.h, r.w, r.D, float(r.eps), ops.stream_ptr())
        # the same bits as the multi entry on the frames gathered in order, with the skip flags the seen counts imply
        gathered = _multi(ops, r, d, d["look"], d["skip"], bufs, device)
        torch.cuda.synchronize()
        assert torch.equal(cost.view(I32), gathered.view(I32)), "ring entry and multi entry differ"
        assert torch.equal(ring.view(I32), before.view(I32)) and torch.equal(state.cpu(), inp["state"])
    torch.cuda.synchronize()
    s = V.hold(r, ref, cost)
    same = float((cost.cpu() == V.evaluate(r, inp)).float().mean())
    F, DB, PK, RING = V.instantiation(r)
    print(f"CVARM <{F},{DB},{int(PK)},{int(RING)}> | {r.name}: worst err / bound {s['ratio']:.3f}, largest error {s['max_err']:.2e}, "
          f"undecided {s['undecided']} left out {s['left_out']}, {same:.1%} of the entries equal the fp32 emulation's")
    assert s["outside"] == 0, f"{r.name}: {s['outside']} entries outside the bound, worst err / bound {s['ratio']:.3f}"
    for buf in bufs:
        assert V.guards_intact(buf, F32), f"{r.name}: a guard element was overwritten"


# ---------------------------------------------------------------------------------------------
# ring store and advance on state words that are out of range
# ---------------------------------------------------------------------------------------------
HEAD_WORDS = (-1, -2, 3, 5, V.INT32_MAX, -V.INT32_MAX - 1)


@pytest.mark.parametrize("head", HEAD_WORDS)
def test_ring_store_and_advance_on_out_of_range_words(device, head):
    """F = 3: the store lands in slot head mod 3 (brought into 0 .. 2) of a guarded ring whose other slots keep their
    pattern, for fp32 and for bf16 pairs; the advance gives the integer reference's words."""
    from ppeadepth import ops
    F, B, C, h, w = 3, 2, 6, 5, 7
    seen = [0, -3, 8, V.INT32_MAX, -V.INT32_MAX - 1, 2]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, h, w, generator=g)
    slot = head % F
    state = torch.tensor([head] + seen[:B], dtype=torch.int64).to(I32).to(device)
    for dtype in ("f32", "bf16"):
        src = x if dtype == "f32" else x.bfloat16()
        want = src if dtype == "f32" else V.pack_pairs(src)
        CE = C if dtype == "f32" else C // 2
        buf, ring = V.guarded((F, B, CE, h, w), F32, device)
        ring.view(I32).fill_(-7)
        sd = src.to(device)
        ops.call(f"ppea_cv_ring_store_{dtype}", ops.ptr(sd), ops.ptr(ring), ops.ptr(state), B, F, C, h, w, ops.stream_ptr())
        torch.cuda.synchronize()
        for s in range(F):
            got = ring[s].view(I32).cpu()
            assert torch.equal(got, want.view(I32) if s == slot else torch.full_like(got, -7)), (dtype, head, s)
        assert V.guards_intact(buf, F32)
    sbuf, st = _words(torch.tensor([head] + seen, dtype=torch.int64).to(I32), device)
    ops.call("ppea_cv_ring_advance", ops.ptr(st), len(seen), F, ops.stream_ptr())
    torch.cuda.synchronize()
    assert st.cpu().tolist() == V.ring_advance_ref([head] + seen, F)
    assert V.guards_intact(sbuf, F32)


# ---------------------------------------------------------------------------------------------
# refusals: return codes, nothing launched
# ---------------------------------------------------------------------------------------------
def _entry_args(device, entry, cost, B=1, F=1, C=2, h=5, w=5, D=1, null=()):
    """Arguments of `entry` ("multi_f32" | "multi_bf16" | "ring_f32" | "ring_bf16") on one-item dummy buffers."""
    z = lambda n, dt=F32: torch.zeros(n, dtype=dt, device=device)        # noqa: E731
    t = dict(cur=z(64), lookup=z(64), pairs=z(128), P=z(12), inv_K=z(16), bins=z(1), skip=z(1, I32), state=z(2, I32), cost=cost)
    p = {k: (None if k in null else _abi().ptr(v)) for k, v in t.items()}
    dims = (B, F, C, h, w, D, 1e-7, _abi().stream_ptr())
    if entry == "multi_f32":
        return (p["cur"], p["lookup"], p["P"], p["inv_K"], p["bins"], p["skip"], p["cost"]) + dims, t
    if entry == "multi_bf16":
        return (p["cur"], p["lookup"], p["pairs"], p["P"], p["inv_K"], p["bins"], p["skip"], p["cost"]) + dims, t
    return (p["cur"], p["lookup"], p["state"], p["P"], p["inv_K"], p["bins"], p["skip"], p["cost"]) + dims, t


def _abi():
    from ppeadepth import _abi
    return _abi


ENTRIES = {"multi_f32": "ppea_cost_volume_multi_fwd_f32", "multi_bf16": "ppea_cost_volume_multi_fwd_bf16",
           "ring_f32": "ppea_cost_volume_ring_fwd_f32", "ring_bf16": "ppea_cost_volume_ring_fwd_bf16"}
REFUSED = [(dict(F=0), UNSUPPORTED), (dict(F=5), UNSUPPORTED), (dict(h=4), UNSUPPORTED), (dict(w=4), UNSUPPORTED),
           (dict(D=0), UNSUPPORTED), (dict(D=65536), UNSUPPORTED), (dict(B=65536), UNSUPPORTED), (dict(B=-1), UNSUPPORTED),
           (dict(C=0), UNSUPPORTED), (dict(B=0), 0)]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals(device, entry):
    """F = 0, F = 5, h = 4, w = 4, D = 0, D = 65536, B = 65536, odd C on the bf16 entries, NULL operands (skip may be NULL on
    the ring entries only, state never): the status comes back and the guarded cost stays NaN; B = 0 returns 0 likewise."""
    lib = _abi().lib
    buf, cost = V.guarded((1, 1, 5, 5), F32, device)
    cases = list(REFUSED)
    if entry.endswith("bf16"):
        cases += [(dict(C=3), UNSUPPORTED), (dict(C=1), UNSUPPORTED)]
    ptrs = ["cur", "lookup", "P", "inv_K", "bins", "cost"] + (["pairs"] if entry == "multi_bf16" else [])
    ptrs += ["skip"] if entry.startswith("multi") else ["state"]
    cases += [(dict(null=(k,)), BAD_ARG) for k in ptrs]
    for kw, want in cases:
        args, keep = _entry_args(device, entry, cost, **kw)
        assert getattr(lib, ENTRIES[entry])(*args) == want, (entry, kw)
    args, keep = _entry_args(device, entry, cost)                         # the same call unrefused: it is served
    assert getattr(lib, ENTRIES[entry])(*args) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(cost).any()) and V.guards_intact(buf, F32)
    buf, cost = V.guarded((1, 1, 5, 5), F32, device)
    for kw, want in cases:
        args, keep = _entry_args(device, entry, cost, **kw)
        getattr(lib, ENTRIES[entry])(*args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(cost).all()) and V.guards_intact(buf, F32)


def test_reduce_refuses_a_batch_past_the_grid(device):
    lib, ptr = _abi().lib, _abi().ptr
    one = torch.zeros(1, device=device)
    idx = torch.zeros(1, device=device, dtype=torch.int64)
    buf, out = V.guarded((1,), F32, device)
    args = (ptr(one), ptr(one), ptr(out), ptr(out), ptr(idx), ptr(out))
    assert lib.ppea_cost_volume_reduce_f32(*args, 65536, 1, 1, 1, _abi().stream_ptr()) == UNSUPPORTED
    assert lib.ppea_cost_volume_reduce_f32(*args, 0, 1, 1, 1, _abi().stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and V.guards_intact(buf, F32)
