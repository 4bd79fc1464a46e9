"""Host-side logic of the device metric path (no GPU): the crop rectangle the workspace is sized by, the flat ground-truth
layout, the ABI of the new entry points and the refusal of tensors that are not on a HIP device."""
import numpy as np
import pytest
import torch


def _scored_pixels(split, H, W):
    """Size of the array `evaluate.evaluate_image` masks, by doing its slicing."""
    from ppeadepth import evaluate
    gt = np.ones((H, W), np.float32)
    if split == "cityscapes":
        return gt[:int(round(H * 0.75))][256:, 192:1856].size
    if split == "eigen":
        return int(evaluate.eigen_crop_mask(gt).sum())
    return gt.size


@pytest.mark.parametrize("split", ["eigen", "cityscapes", "benchmark"])
def test_region_size_is_the_rectangle_the_host_protocol_scores(split):
    from ppeadepth import evaluate
    sizes = [(375, 1242), (370, 1226), (374, 1238), (376, 1241), (1024, 2048), (1022, 2048), (1026, 1800), (300, 150),
             (96, 320), (341, 193), (342, 193), (7, 5)]
    for H, W in sizes:
        assert evaluate.region_size(split, H, W) == _scored_pixels(split, H, W), (split, H, W)


def test_device_ground_truth_is_one_flat_buffer_and_a_table():
    from ppeadepth import evaluate
    g = np.random.default_rng(0)
    maps = [g.random((5, 7)), g.random((4, 9)).astype(np.float32), g.random((6, 6))]
    gt = evaluate.DeviceGroundTruth(np.array(maps, dtype=object), "cpu")
    assert len(gt) == 3 and gt.flat.dtype == torch.float32 and gt.table.dtype == torch.int64
    assert gt.table.tolist() == [[0, 5, 7], [35, 4, 9], [71, 6, 6]]
    for (off, h, w), m in zip(gt.table.tolist(), maps):
        assert np.array_equal(gt.flat[off:off + h * w].reshape(h, w).numpy(), m.astype(np.float32))
    assert gt.max_region("benchmark") == 36 and gt.max_region("benchmark", 0, 2) == 36 and gt.max_region("benchmark", 0, 1) == 35
    with pytest.raises(ValueError):
        evaluate.DeviceGroundTruth([], "cpu")


def test_depth_errors_refuses_tensors_that_are_not_on_a_hip_device():
    from ppeadepth import _abi, evaluate, ops
    gt = evaluate.DeviceGroundTruth([np.ones((8, 8), np.float32)] * 2, "cpu")
    pred = torch.rand(2, 4, 4)
    with pytest.raises(_abi.PpeaKernelError):
        ops.depth_errors(pred, gt.flat, gt.table, gt.max_region("eigen"))
    with pytest.raises(_abi.PpeaKernelError):
        gt.score(pred, 0)
    with pytest.raises(_abi.PpeaKernelError):
        ops.depth_errors(pred, gt.flat, gt.table[:1], 64)                  # table / batch mismatch
    with pytest.raises(_abi.PpeaKernelError):
        ops.depth_errors_mean(torch.zeros(3, 7, dtype=torch.float64))


def test_depth_errors_abi():
    from ppeadepth import _abi
    assert _abi.ABI_VERSION >= 14
    for name, nargs in (("ppea_depth_errors_f32", 16), ("ppea_depth_errors_mean_f64", 4), ("ppea_depth_errors_workspace_bytes", 2)):
        assert len(_abi.SIGNATURES[name]) == nargs and hasattr(_abi.lib, name)
    ws = _abi.lib.ppea_depth_errors_workspace_bytes
    # two fp32 workspaces of B x max_region, 7 fp64 partial sums per 2048-pixel chunk, 4 passes x 4 selections x 256 bins
    B, R = 12, 219 * 1153
    assert ws(B, R) >= 2 * 4 * B * R + 8 * 7 * B * -(-R // 2048) + 4 * B * (4 * 4 * 256 + 1)
    assert ws(B, R) <= 2 * 4 * B * R + 8 * 7 * B * -(-R // 2048) + 4 * B * (4 * 4 * 256 + 1) + 4 * 256
    assert ws(1, 0) > 0 and ws(0, 10) < 0 and ws(2 * B, R) > ws(B, R)


def test_val_rejects_an_unknown_metrics_mode():
    from ppeadepth.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    with pytest.raises(ValueError):
        tr.val([], [], metrics="gpu")
