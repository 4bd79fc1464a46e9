"""Every output of the csrc/geometry.hip kernels, bit for bit, against tests/golden/geometry_bits.npz: the bits those
kernels produced before their projection arithmetic, block reductions and 4x4 product were folded into shared device
functions (recorded by tools/gen_geometry_bits_golden.py at the last commit that spelled each kernel out).

The other geometry tests tie the split kernels to the fused ones and both to the reference at 1e-5: a shared helper that
changed an association would move them together and pass.  This one holds the arithmetic itself still -- fused and split
projection forward and backward, the reduced dP / d_inv_K at one and at two passes of the reduction's lane loop,
grid_sample in both padding modes, pose_matrix both ways, pose_chain and pose_chain_ring for F = 1..4.  The inputs are not
stored: the generator's `compute()` draws them again from its seeded host generators.
"""
import importlib.util
import os

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("gen_geometry_bits_golden",
                                                  os.path.join(ROOT, "tools", "gen_geometry_bits_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_geometry_kernels_reproduce_the_recorded_bits(device, golden):
    want = golden("geometry_bits")
    got = _generator().compute(device)
    assert sorted(got) == sorted(want) and len(want) == 76
    differing = []
    for name, w in want.items():
        g = got[name]
        if g.dtype != w.dtype or g.shape != w.shape or not torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)):
            differing.append(name)
    assert not differing, differing
    # the fixture is not trivially equal: the reduced gradients are non-zero, the chains hold masked and absent frames
    assert all(bool(want[f"{op}/1x72x232/T.grad"].any()) for op in ("bpp", "p3d", "p3dz"))
    assert bool(want["bp/1x72x232/d_inv_K"].any())
    for Fr in range(1, 5):
        keep_zeroed = want[f"chain/{Fr}/T"][1, (Fr - 1) // 2]
        assert not keep_zeroed.any() and bool(want[f"chain/{Fr}/T_all"][1, (Fr - 1) // 2].any())
        assert want[f"ring/{Fr}/present"].tolist() == [[j < seen for j in range(Fr)] for seen in (Fr, Fr - 1, Fr + 2)]
