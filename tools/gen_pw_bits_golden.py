"""Writes tests/golden/pw_bits.json: the sha256 of the raw bytes of every tensor the entry points of the pointwise GEMM family
(csrc/pwconv.hip, csrc/pwgrad.hip, csrc/tapsum.hip) write, on every row of the family's pin.

    python tools/gen_pw_bits_golden.py [--out tests/golden/pw_bits.json]          (needs the GPU)

The fixture pins the ARITHMETIC of the family -- the order of the K sums in each tile, the epilogue's roundings, the order of
the statistics and split sums -- across changes that are meant to leave it alone: tests/test_pw_bits_gpu.py calls `compute()`
again and compares.  Record it at the commit BEFORE such a change; re-record only for a change that is meant to alter the
arithmetic.  Inputs are not stored: the rows are oracle/pw_inputs.py's, their inputs come from its seeded generators, and each
row runs under its own hook variables through the launchers of tests/pw_launch.py (the ones the pin uses).

Keys are "<table>/<row name>/<output>":
  tile, edge     P.TILE_CASES, P.EDGE_CASES: y, y2 (EPI 1, and the second output of ops.pwconv_table for EPI 5), sums (EPI 4)
  pwgrad         P.PWGRAD_CASES: C [M][N], rowsum (where the row asks for it)
  into           P.INTO_CASES: dw, db
  pair           P.PAIR_CASES: a/dw, a/db, b/dw, b/db -- from the pair kernel where it serves the row, else from the two
                 single launches of ops.pwgrad_into_pair
  tapsum         P.TAPSUM_CASES: pre, h, dT
Only the written view is hashed, never the guards around it.
"""
import argparse
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ppea-depth_amd"), os.path.join(ROOT, "tests")]

ROWS = 68 + 51 + 14 + 9 + 5 + 15


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _put(out, prefix, tensors):
    for k, t in tensors.items():
        out[f"{prefix}/{k}"] = _sha(t)


def compute(device):
    """-> {key: sha256 hex digest}, every output listed in the module docstring."""
    import pw_launch as L
    from oracle import pw_inputs as P
    from ppeadepth import ops
    out, mp = {}, pytest.MonkeyPatch()
    try:
        for table, rows in (("tile", P.TILE_CASES), ("edge", P.EDGE_CASES)):
            for c in rows:
                inp = L.to(P.make_pw_inputs(c), device)
                with L.hooks(mp, c.env):
                    if c.epi == 5:
                        y, y2 = L.launch_infer(ops, inp)
                        got = dict(y=y, y2=y2)
                    else:
                        served, got, _ = L.launch_pw(ops, c, inp, ops.pwconv_plan(c.B, c.M, c.K, c.HW, c.ta))
                        assert served, c.name
                    torch.cuda.synchronize()
                _put(out, f"{table}/{c.name}", got)
        for c in P.PWGRAD_CASES:
            inp = L.to(P.make_pwgrad_inputs(c), device)
            with L.hooks(mp, c.env):
                served, got, _ = L.launch_pwgrad(ops, c, inp, device, ops.pwgrad_plan(c.B, c.M, c.N, c.H * c.W))
                torch.cuda.synchronize()
            assert served, c.name
            got = dict(C=got["out"][:c.M * c.N], **(dict(rowsum=got["out"][c.M * c.N:]) if c.rowsum else {}))
            _put(out, f"pwgrad/{c.name}", got)
        for c in P.INTO_CASES:
            inp = L.to(P.make_into_inputs(c), device)
            with L.hooks(mp, c.env):
                served, got, _ = L.launch_into(ops, c, inp, device, ops.pwgrad_plan(c.B, c.taps * c.Ch, c.N, c.H * c.W))
                torch.cuda.synchronize()
            assert served, c.name
            _put(out, f"into/{c.name}", got)
        for name, a, b, env, claimed in P.PAIR_CASES:
            inps = [L.to(P.make_into_inputs(c), device) for c in (a, b)]
            with L.hooks(mp, env):
                plan = ops.pwgrad_pair_plan(a.B, (a.taps * a.Ch, b.taps * b.Ch), (a.N, b.N), a.H * a.W)
                served, outs, _ = L.launch_pair(ops, a, b, inps, device, plan)
                if not served:
                    outs = [dict(dw=dw, **({} if db is None else dict(db=db)))
                            for dw, db in ops.pwgrad_into_pair(L.op_args(a, inps[0]), L.op_args(b, inps[1]))]
                torch.cuda.synchronize()
            assert served == claimed, name
            for tag, o in zip("ab", outs):
                _put(out, f"pair/{name}/{tag}", o)
        for c in P.TAPSUM_CASES:
            inp = L.to(P.make_tapsum_inputs(c), device)
            served, got, _ = L.launch_tapsum(ops, c, inp, device)
            torch.cuda.synchronize()
            assert served, c.name
            _put(out, f"tapsum/{c.name}", got)
    finally:
        mp.undo()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pw_bits.json"))
    args = ap.parse_args()
    out = compute(torch.device("cuda:0"))
    assert len({k.rsplit("/", 2 if k.startswith("pair/") else 1)[0] for k in out}) == ROWS
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(out)} hashes, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
