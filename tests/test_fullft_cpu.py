"""Full fine-tuning (--fullft_reb), host side: the freeze rule against the reference's own flags and the C ABI of the
weight-gradient entry points.  No GPU."""
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.mark.parametrize("size", ["b", "l"])
def test_fullft_freeze_rule_matches_reference(size):
    """RepDepth(opt) under --adapter --fullft_reb: the same parameter names, each with the reference's requires_grad
    (repdepth.py:47, :121 skip the freeze rule) -- and the backbone convolutions really are among the trainable ones."""
    from ppeadepth import networks, options
    z = np.load(os.path.join(GOLDEN, "fullft_spec.npz"))
    names = [str(n) for n in z[f"{size}:names"]]
    want = dict(zip(names, (bool(t) for t in z[f"{size}:trainable"])))
    model = networks.RepDepth(options.default_options(rep_size=size, fullft_reb=True))
    got = {n: p.requires_grad for n, p in model.named_parameters()}
    assert set(got) == set(want)
    wrong = [n for n in names if got[n] != want[n]]
    assert not wrong, wrong[:8]
    for enc in ("encoder.replk.", "mono_encoder."):
        for k in ("stem.0.conv.weight", "stem.1.conv.weight", "transitions.0.0.conv.weight",
                  "stages.0.blocks.0.large_kernel.lkb_origin.conv.weight",
                  "stages.2.blocks.7.pw1.conv.weight", "stages.3.blocks.1.pw2.conv.weight"):
            assert got[enc + k], enc + k
    # the adapter rule is what it was
    frozen = networks.RepDepth(options.default_options(rep_size=size))
    assert not dict(frozen.named_parameters())["encoder.replk.stages.2.blocks.7.pw1.conv.weight"].requires_grad


def test_fullft_entry_points_are_declared_and_exported():
    from ppeadepth import _abi
    for name in ("ppea_dwconv3x3_bwd_filter_workspace_bytes", "ppea_dwconv3x3_bwd_filter_f32",
                 "ppea_dwconv3x3_bwd_filter_bf16", "ppea_dwconv_lk_bwd_filter_workspace_bytes",
                 "ppea_dwconv_lk_bwd_filter_bf16"):
        assert name in _abi.SIGNATURES, name
        assert hasattr(_abi.lib, name), name
    # the sizes are host arithmetic: positive for a served shape, and large enough for one fp32 tile per part
    assert _abi.lib.ppea_dwconv3x3_bwd_filter_workspace_bytes(2, 3, 5, 7, 2) >= 3 * 9 * 4
    assert _abi.lib.ppea_dwconv_lk_bwd_filter_workspace_bytes(2, 3, 6, 20, 13, 5) >= 3 * (13 * 13 + 25) * 4
    assert _abi.lib.ppea_dwconv_lk_bwd_filter_workspace_bytes(2, 3, 6, 20, 7, 0) < 0          # unserved K
