"""Host side of the HIP input pipeline (no GPU): the ABI of its entry points, the compact tap table the resize kernels read,
the packed ColorJitter parameter table, and the refusals."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = {"ppea_lanczos_h_u8": 13, "ppea_lanczos_v_u8": 9, "ppea_color_jitter_workspace_bytes": 3,
               "ppea_color_jitter_u8": 10, "ppea_repeat_rows_f32": 6}
# (insize, outsize): the workload's first level and its 2:1 levels, then the sizes of tests/test_input_pipeline_gpu.py
SIZES = [(1242, 640), (375, 192), (640, 320), (192, 96), (320, 160), (96, 48), (160, 80), (48, 24),
         (101, 64), (47, 32), (64, 32), (32, 16), (16, 8), (8, 4), (40, 64), (20, 32), (33, 64)]


def test_input_pipeline_abi():
    from ppeadepth import _abi
    assert _abi.lib.ppea_abi_version() == _abi.ABI_VERSION >= 20         # 20: the version these entry points arrived with
    header = open(os.path.join(ROOT, "include", "ppea_depth.h")).read()
    declared = set(re.findall(r"^(?:int|long)\s+(ppea_\w+)\s*\(", header, flags=re.M))
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared, name
        assert len(_abi.SIGNATURES[name]) == nargs and hasattr(_abi.lib, name), name
    ws = _abi.lib.ppea_color_jitter_workspace_bytes
    # one 32-bit partial sum per image and chunk of at most 4096 pixels, never fewer than the scalar path's 1024-pixel chunks
    assert ws(36, 192, 640) == 36 * 4 * (192 * 640 // 1024) and ws(1, 13, 17) == 4 and ws(0, 4, 4) < 0


@pytest.mark.parametrize("insize,outsize", SIZES)
def test_compact_tap_table_reproduces_the_dense_matrix(insize, outsize):
    from ppeadepth import input_pipeline as ip
    dense = ip.lanczos_matrix(insize, outsize)
    table = ip.compact_taps(dense)
    assert table.dtype == np.int32 and table.shape[0] == outsize
    assert np.array_equal(ip.dense_taps(table, insize), dense)
    lo, n = table[:, 0].astype(int), table[:, 1].astype(int)
    assert (lo >= 0).all() and (n >= 1).all() and (lo + n <= insize).all() and table.shape[1] == 2 + n.max()
    assert n.max() <= int(2 * 3.0 * max(insize / outsize, 1.0)) + 1           # support 3 x scale on each side
    for i in range(outsize):
        assert not table[i, 2 + n[i]:].any()                      # padding past a row's taps is zero


def _resize_int32(img, table_h, table_v):
    """The kernels' arithmetic in numpy: int32 accumulator from 1 << 21, arithmetic shift by 22, clip; rows, then columns."""
    def one_pass(x, table):                                       # along the last axis
        out = np.empty(x.shape[:-1] + (len(table),), np.uint8)
        for i, row in enumerate(table):
            lo, n = int(row[0]), int(row[1])
            acc = (x[..., lo:lo + n].astype(np.int64) * row[2:2 + n].astype(np.int64)).sum(-1) + (1 << 21)
            assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31
            out[..., i] = np.clip(acc >> 22, 0, 255)
        return out
    x = one_pass(img, table_h) if table_h is not None else img
    return one_pass(x.swapaxes(-1, -2), table_v).swapaxes(-1, -2) if table_v is not None else x


@pytest.mark.parametrize("in_hw,out_hw", [((47, 101), (32, 64)), ((8, 16), (4, 8)), ((20, 40), (32, 64)), ((47, 64), (32, 64))])
def test_integer_formulation_over_the_compact_table_equals_the_torch_path(in_hw, out_hw):
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (2, 3) + in_hw, generator=g, dtype=torch.uint8)
    img[1, :, ::2, ::2] = 255                                     # checkerboard: the negative lobes reach the clip
    img[1, :, 1::2, ::2] = 0
    img[1, :, ::2, 1::2] = 0
    img[1, :, 1::2, 1::2] = 255
    want = ip.LanczosResize(in_hw, out_hw, "cpu")(img)
    th = ip.compact_taps(ip.lanczos_matrix(in_hw[1], out_hw[1])) if in_hw[1] != out_hw[1] else None
    tv = ip.compact_taps(ip.lanczos_matrix(in_hw[0], out_hw[0])) if in_hw[0] != out_hw[0] else None
    assert np.array_equal(_resize_int32(img.numpy(), th, tv), want.numpy())
    # the flip-only first pass: one tap of weight 1.0 changes no byte
    assert np.array_equal(_resize_int32(img.numpy(), ip.identity_taps(in_hw[1]), None), img.numpy())


def test_packed_jitter_parameters():
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(2)
    a, b = ip.draw_jitter_params(3, g), ip.draw_jitter_params(3, g)
    b["hue"] = torch.tensor([-0.1, 0.0, 0.1])
    apply = torch.tensor([True, False, True, True, True, False])
    t = ip.pack_jitter_params([a, b], apply)
    assert t.dtype == torch.int32 and tuple(t.shape) == (6, 10) and t.is_contiguous()
    assert torch.equal(t[:, :4].long(), torch.cat([a["order"], b["order"]]))
    for j, k in enumerate(("brightness", "contrast", "saturation")):
        assert torch.equal(t[:, 4 + j].contiguous().view(torch.float32), torch.cat([a[k], b[k]]))
    assert t[3:, 7].tolist() == [int(-0.1 * 255) & 255, 0, int(0.1 * 255) & 255] == [231, 0, 25]
    assert t[:, 8].tolist() == [1, 0, 1, 1, 1, 0] and not t[:, 9].any()
    assert torch.equal(ip.pack_jitter_params(a, apply[:3]), t[:3])


def test_hip_backend_is_refused_on_the_cpu():
    from ppeadepth import _abi, ops
    from ppeadepth import input_pipeline as ip
    with pytest.raises(ValueError):
        ip.DeviceInputPipeline((47, 101), 32, 64, "cpu", backend="hip")
    with pytest.raises(ValueError):
        ip.DeviceInputPipeline((47, 101), 32, 64, "cpu", backend="triton")
    assert ip.DeviceInputPipeline((47, 101), 32, 64, "cpu").backend == "torch"
    img = torch.zeros(2, 3, 8, 16, dtype=torch.uint8)
    taps = torch.from_numpy(ip.compact_taps(ip.lanczos_matrix(16, 8)))
    with pytest.raises(_abi.PpeaKernelError):
        ops.lanczos_resize_u8(img, (8, 8), taps)                  # CPU tensors: no fallback
    with pytest.raises(_abi.PpeaKernelError):
        ops.lanczos_resize_u8(img, (8, 8))                        # a change of width without a table
    with pytest.raises(_abi.PpeaKernelError):
        ops.color_jitter_u8(img, torch.zeros(2, 10, dtype=torch.int32))
    with pytest.raises(_abi.PpeaKernelError):
        ops.color_jitter_u8(img, torch.zeros(3, 10, dtype=torch.int32))
