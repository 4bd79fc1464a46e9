"""Cityscapes on the GPU: backend "hip" (the view pass `ppea_lanczos_h_view_u8`, then the kernels every pipeline shares)
returns the bytes of backend "torch", which tests/test_cityscapes_pipeline_cpu.py compares with Pillow.  Equality only.

Every source the view pass reads is a slice of a larger buffer filled with 255: in front of and behind the frames (the odd
front pad also takes the windows off every alignment), and for the evaluation frames below the crop.  A read outside the
windows then changes output bytes."""
import copy
import ctypes
import random

import pytest
import torch

from test_cityscapes_pipeline_cpu import SCALES, cameras, eval_case, training_case

pytestmark = pytest.mark.gpu

FRONT, BACK = 37, 91            # guard bytes around a source


def _guarded(t, device):
    """The host tensor inside a device buffer of 255s; the returned view has t's shape and (dense) strides."""
    buf = torch.full((FRONT + t.numel() + BACK,), 255, dtype=torch.uint8, device=device)
    view = buf[FRONT:FRONT + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + FRONT and view.is_contiguous()
    return view


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, k
        assert torch.equal(a[k], b[k]), k


def _train_inputs(B, raw_hw, flips, seed):
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(seed)
    trip = torch.randint(0, 256, (B, raw_hw[0], 3 * raw_hw[1], 3), generator=g, dtype=torch.uint8)
    trip[0, :, 2 * raw_hw[1]: 2 * raw_hw[1] + raw_hw[1] // 2] //= 16
    jitter = {(f, s): ip.draw_jitter_params(B, g) for f in (0, -1, 1) for s in range(SCALES)}
    return dict(B=B, raw_hw=raw_hw, triplets=trip, cameras=cameras(B), do_flip=torch.tensor(flips),
                do_color_aug=torch.ones(B, dtype=torch.bool), jitter=jitter)


# (inputs, (height, width)): the CPU test's case; one row of the real width with a row count (3 x 33) that is no multiple of
# the two rows a workgroup takes at width 96; windows 53 pixels wide (53 % 4 == 1: byte offsets 159 and 318), all flipped
# and none flipped
TRAIN_CASES = {
    "cpu_case": lambda: (training_case(), (16, 24)),
    "real_width_odd_rows": lambda: (_train_inputs(1, (33, 1024), [True], 1), (16, 96)),
    "w53_all_flipped": lambda: (_train_inputs(2, (20, 53), [True, True], 2), (8, 24)),
    "w53_none_flipped": lambda: (_train_inputs(2, (20, 53), [False, False], 2), (8, 24)),
}


@pytest.mark.parametrize("case", sorted(TRAIN_CASES))
def test_training_pipeline_hip_equals_torch(device, case):
    from ppeadepth.input_pipeline import CityscapesInputPipeline
    c, (H, W) = TRAIN_CASES[case]()
    args = (c["cameras"], c["do_color_aug"], c["do_flip"], c["jitter"])
    hip = CityscapesInputPipeline(device, H, W, c["raw_hw"])
    assert hip.backend == "hip"
    got = hip(_guarded(c["triplets"], device), *args)
    want = CityscapesInputPipeline(device, H, W, c["raw_hw"], backend="torch")(c["triplets"].to(device), *args)
    assert len(got) == 2 * 3 * SCALES + 2 * SCALES
    _same(got, want)
    if case == "cpu_case":                                         # item 1's frame +1 is blank: never jittered
        for s in range(SCALES):
            assert torch.equal(got[("color_aug", 1, s)][1], got[("color", 1, s)][1]) and not got[("color", 1, s)][1].any()
            assert not torch.equal(got[("color_aug", 1, s)][0], got[("color", 1, s)][0])


def test_view_pass_marks_the_blank_third(device):
    from ppeadepth import input_pipeline as ip, ops
    c = training_case()
    B, (Hraw, w), (H, W) = c["B"], c["raw_hw"], c["hw"]
    trip = _guarded(c["triplets"], device)
    thirds = [trip[:, :, k * w:(k + 1) * w] for k in (1, 0, 2)]                # frames 0, -1, +1
    flip = c["do_flip"].to(torch.int32).repeat(3).to(device)
    nonzero = torch.full((3 * B,), 5, dtype=torch.int32, device=device)
    rs = ip.LanczosResize((Hraw, w), (H, W), device, "hip", first=True)
    got = ops.lanczos_resize_view_u8(thirds, (H, W), rs.taps_h, rs.taps_v, flip, nonzero)
    planar = torch.cat([t.permute(0, 3, 1, 2) for t in thirds])
    flipped = torch.where(flip.bool().reshape(-1, 1, 1, 1), planar.flip(-1), planar)
    assert torch.equal(got, ip.LanczosResize((Hraw, w), (H, W), device)(flipped))
    assert nonzero.tolist() == [1] * (2 * B) + [1, 0, 1]                        # image 2 * B + 1: item 1's frame +1
    assert not got[2 * B + 1].any()


# the CPU test's two cases, and one row of the real width: 3 x 2048 staged bytes, Pillow's ksize of 25 (24 non-zero taps)
@pytest.mark.parametrize("raw_hw,hw,B", [((42, 64), (16, 24), 3), ((40, 64), (16, 24), 3), ((8, 2048), (8, 512), 2)])
def test_eval_pipeline_hip_equals_torch(device, raw_hw, hw, B):
    from ppeadepth.input_pipeline import CityscapesEvalPipeline
    c = eval_case(raw_hw, B)
    hip = CityscapesEvalPipeline(device, hw[0], hw[1], raw_hw)
    assert hip.backend == "hip" and (raw_hw[1] != 2048 or hip.resize[0].taps_h.shape[1] - 2 == 24)
    got = hip({f: _guarded(v, device) for f, v in c["raw"].items()}, c["cameras"])
    want = CityscapesEvalPipeline(device, hw[0], hw[1], raw_hw, backend="torch")({f: v.to(device) for f, v in c["raw"].items()},
                                                                                c["cameras"])
    assert len(got) == 2 * 2 * SCALES + 2 * SCALES
    _same(got, want)
    for f in (0, -1):
        assert torch.equal(got[("color_aug", f, 0)], got[("color", f, 0)])


@pytest.mark.parametrize("flipped", [False, True])
def test_view_entry_on_a_planar_source_equals_the_dense_entry(device, flipped):
    from ppeadepth import input_pipeline as ip, ops
    g = torch.Generator().manual_seed(4)
    N, in_hw, out_hw = 3, (47, 101), (32, 64)
    img = torch.randint(0, 256, (N, 3) + in_hw, generator=g, dtype=torch.uint8)
    img[1] = 0
    img = _guarded(img, device)
    rs = ip.LanczosResize(in_hw, out_hw, device, "hip", first=True)
    flip = torch.tensor([1, 1, 0] if flipped else [0, 0, 0], dtype=torch.int32, device=device)
    nz_old, nz_new = (torch.full((N,), 5, dtype=torch.int32, device=device) for _ in range(2))
    want = ops.lanczos_resize_u8(img, out_hw, rs.taps_h, rs.taps_v, flip, nz_old)
    view = img.permute(0, 2, 3, 1)                                 # pixel stride 1, channel stride H * W
    assert view.stride() == (3 * 47 * 101, 101, 1, 47 * 101)
    got = ops.lanczos_resize_view_u8(view, out_hw, rs.taps_h, rs.taps_v, flip, nz_new)
    assert torch.equal(got, want) and torch.equal(nz_new, nz_old) and nz_new.tolist() == [1, 0, 1]
    # the horizontal pass alone, and without the optional arguments
    assert torch.equal(ops.lanczos_resize_view_u8(view, (47, 64), rs.taps_h), ops.lanczos_resize_u8(img, (47, 64), rs.taps_h))


def test_view_entry_refuses_before_it_launches(device):
    from ppeadepth import _abi, input_pipeline as ip, ops
    H, Win, Wout = 8, 16, 8
    src = torch.zeros(2, H, Win, 3, dtype=torch.uint8, device=device)
    taps = torch.from_numpy(ip.compact_taps(ip.lanczos_matrix(Win, Wout))).to(device)
    dst = torch.full((2, 3, H, Wout), 7, dtype=torch.uint8, device=device)
    nonzero = torch.full((2,), 7, dtype=torch.int32, device=device)
    good = dict(src=src.data_ptr(), C=3, pixel=3, row=Win * 3, channel=1, item=H * Win * 3, Win=Win)

    def status(**kw):
        a = dict(good, **kw)
        ptrs = (ctypes.c_void_p * 1)(a["src"])
        return _abi.lib.ppea_lanczos_h_view_u8(ptrs, 1, 2, a["C"], a["pixel"], a["row"], a["channel"], a["item"],
                                               _abi.ptr(taps), taps.shape[1] - 2, None, _abi.ptr(nonzero), _abi.ptr(dst),
                                               H, a["Win"], Wout, _abi.stream_ptr())
    ARG, UNSUPPORTED = -2, -1
    assert status(src=None) == ARG                                 # a null source
    for stride in ("pixel", "row", "channel", "item"):
        assert status(**{stride: 0}) == ARG and status(**{stride: -good[stride]}) == ARG
    assert status(row=Win * 3 - 1) == ARG                          # the window is wider than the row stride allows
    assert status(pixel=2) == ARG                                  # three channels do not fit a 2-byte pixel
    assert status(Win=20480, row=20480 * 3, item=H * 20480 * 3) == UNSUPPORTED      # 61 440 bytes: no row can be staged
    with pytest.raises(_abi.PpeaKernelError, match="unsupported"):
        _abi.check(UNSUPPORTED, "ppea_lanczos_h_view_u8")
    torch.cuda.synchronize()
    assert (dst == 7).all() and (nonzero == 7).all()               # nothing ran, not even the memset of the marks
    assert status() == 0                                           # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert not (dst == 7).all() and not nonzero.any()
    # the same refusals through ops, from the strides of the view it is given
    with pytest.raises(_abi.PpeaKernelError, match="inconsistent"):
        ops.lanczos_resize_view_u8(src[:, :, :1].expand(2, H, Win, 3), (H, Wout), taps)            # pixel stride 0
    with pytest.raises(_abi.PpeaKernelError, match="inconsistent"):
        ops.lanczos_resize_view_u8(torch.as_strided(src, (2, H, Win, 3), (H * Win * 3, 40, 3, 1)), (H, Wout), taps)
    wide = torch.zeros(1, 1, 20480, 3, dtype=torch.uint8, device=device)
    with pytest.raises(_abi.PpeaKernelError, match="unsupported"):
        ops.lanczos_resize_view_u8(wide, (1, 8), torch.from_numpy(ip.identity_taps(8)).to(device))
    with pytest.raises(_abi.PpeaKernelError):
        ops.lanczos_resize_view_u8([src, src[:, :, :8]], (H, Wout), taps)                          # two shapes


def test_hip_dictionary_drives_process_batch(device):
    """The small-model size of tests/test_e2e_gpu.py (64x96, B = 2): the step is a pure function of state, inputs and seeds
    and the two dictionaries are byte-equal, so the two losses are the same bits."""
    from oracle import synth
    from ppeadepth import input_pipeline as ip, networks, options, rng
    from ppeadepth.trainer import Trainer
    B, H, W, raw_hw = 2, 64, 96, (80, 128)
    c = _train_inputs(B, raw_hw, [True, False], 6)
    cams = cameras(B) * (raw_hw[1] / 1024.0)
    cams[:, 2, 2] = 1
    assert (cams[0] != cams[1]).any()
    args = (cams, c["do_color_aug"], c["do_flip"], c["jitter"])
    got = ip.CityscapesInputPipeline(device, H, W, raw_hw)(_guarded(c["triplets"], device), *args)
    want = ip.CityscapesInputPipeline(device, H, W, raw_hw, backend="torch")(c["triplets"].to(device), *args)
    _same(got, want)
    opt = options.default_options(height=H, width=W, batch_size=B)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model)
    model.to(device).train()
    rng.set_mode("reference")
    try:
        tr = Trainer(opt, model, device)
        tracker = copy.deepcopy(tr.depth_bin_tracker)
        losses = []
        for inputs in (got, want):
            tr.depth_bin_tracker = copy.deepcopy(tracker)
            torch.manual_seed(3)
            random.seed(3)
            outputs, loss = tr.process_batch(dict(inputs), True)
            assert outputs[("disp", 0)].shape == (B, 1, H, W)
            losses.append(loss["loss"].detach().clone())
    finally:
        rng.set_mode("device")
    assert torch.isfinite(losses[0]).item() and torch.equal(losses[0], losses[1])
