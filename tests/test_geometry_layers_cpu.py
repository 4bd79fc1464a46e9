"""Host side of `layers.BackprojectDepth` / `layers.Project3D`: the composite is what it was, the pixel buffers are built
only when it runs, the operators behind the device path refuse host tensors, the C ABI carries the four kernels and
`Trainer` has the reference's two module dictionaries."""
import pytest
import torch

from conftest import rel_err


def test_host_composite_matches_reference_golden(golden):
    from ppeadepth import layers
    g = golden("layers_geometry")
    B, _, H, W = g["depth"].shape
    bp = layers.BackprojectDepth(B, H, W)
    assert bp._host is None and not list(bp.buffers()) and not list(bp.parameters())      # nothing until the host path runs
    pts = bp(g["depth"], g["inv_K"])
    assert rel_err(pts, g["points"]) < 1e-6
    assert bp.pix_coords.shape == (B, 3, H * W) and bp.ones.shape == (B, 1, H * W)
    pix, z = layers.Project3D(B, H, W, dc=True)(pts, g["K"], g["T_inv"])
    assert (pix - g["grid"]).abs().max() < 1e-5
    assert z.shape == (B, 1, H, W)


def test_ops_refuse_host_tensors(golden):
    from ppeadepth import ops
    from ppeadepth._abi import PpeaKernelError
    g = golden("layers_geometry")
    B, _, H, W = g["depth"].shape
    with pytest.raises(PpeaKernelError):
        ops.backproject(g["depth"], g["inv_K"])
    with pytest.raises(PpeaKernelError):
        ops.project3d(g["points"], g["K"], g["T_inv"], H, W)


def test_abi_binds_the_geometry_layer_kernels():
    from ppeadepth import _abi
    for name in ("ppea_backproject_fwd_f32", "ppea_backproject_bwd_f32", "ppea_project3d_fwd_f32", "ppea_project3d_bwd_f32"):
        assert name in _abi.SIGNATURES and hasattr(_abi.lib, name)
    # 72 blocks of 256 pixels per image at 96x192: 9 / 12 partial sums per block
    assert _abi.lib.ppea_backproject_bwd_workspace_bytes(3, 96, 192) == 3 * 72 * 9 * 4
    assert _abi.lib.ppea_project3d_bwd_workspace_bytes(3, 96, 192) == 3 * 72 * 12 * 4
    # argument checks happen before anything is launched
    assert _abi.lib.ppea_project3d_fwd_f32(None, None, None, None, 1, 1, 8, 1e-7, None) == -1
    assert _abi.lib.ppea_backproject_fwd_f32(None, None, None, 1, 4, 4, None) == -2
    # B is the grid's y extent
    assert _abi.lib.ppea_backproject_fwd_f32(None, None, None, 65536, 4, 4, None) == -1
    assert _abi.lib.ppea_project3d_bwd_f32(None, None, None, None, None, None, None, 65536, 4, 4, 1e-7, None) == -1


def test_trainer_has_the_reference_module_dictionaries():
    from ppeadepth import layers, options
    from ppeadepth.trainer import Trainer
    opt = options.default_options(height=64, width=96, batch_size=2)
    tr = Trainer(opt, None, "cpu")
    assert list(tr.backproject_depth) == list(tr.project_3d) == list(range(opt.sclm + 1))
    bp, pr = tr.backproject_depth[0], tr.project_3d[0]
    assert isinstance(bp, layers.BackprojectDepth) and isinstance(pr, layers.Project3D)
    assert (bp.batch_size, bp.height, bp.width) == (pr.batch_size, pr.height, pr.width) == (2, 64, 96)
    assert pr.dc is False and pr.eps == 1e-7
