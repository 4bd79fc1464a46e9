"""The HIP input pipeline (csrc/input_pipeline.hip) against the torch formulation run on the CPU, Pillow and the Pillow-based
ColorJitter restatement (oracle/ref_jitter.py).  Every comparison is exact: the arithmetic is integer, or IEEE operations
in a fixed order."""
import itertools
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ORDERS = list(itertools.permutations(range(4)))
LIBRARY = re.compile(r"Cijk_|igemm|ck::|ck_tile|miopen|MIOpen|gemm_|Gemm|rocblas|hipblaslt|rocprim|hipcub|cub::|sort|Sort|"
                     r"at::native|elementwise|reduce_kernel")


def _unit(u8):
    """ToTensor of a uint8 image on the CPU: one correctly rounded fp32 division."""
    return u8.cpu().to(torch.float32) / 255.0


def _params(B, g, order=None, **fixed):
    from ppeadepth import input_pipeline as ip
    prm = ip.draw_jitter_params(B, g)
    if order is not None:
        prm["order"] = torch.tensor(order)
    for k, v in fixed.items():
        prm[k] = torch.tensor(v, dtype=torch.float32)
    return prm


def _jitter_hip(img, prm, apply, device, nonzero=None):
    from ppeadepth import input_pipeline as ip, ops
    table = ip.pack_jitter_params(prm, apply).to(device)
    color, aug = ops.color_jitter_u8(img.to(device), table, nonzero)
    assert color.dtype == aug.dtype == torch.float32 and color.is_contiguous() and aug.is_contiguous()
    assert torch.equal(color.cpu(), _unit(img))
    return aug.cpu()


# ---- 1. resize ------------------------------------------------------------------------------------------------------
def _resize_images(in_hw, g):
    img = torch.randint(0, 256, (5 + 3, 3) + in_hw, generator=g, dtype=torch.uint8)
    img[5], img[6] = 0, 255
    yy, xx = torch.meshgrid(torch.arange(in_hw[0]), torch.arange(in_hw[1]), indexing="ij")
    img[7] = (((yy + xx) % 2) * 255).to(torch.uint8)              # 0 / 255 checkerboard: both sides of the clip
    return img


@pytest.mark.parametrize("in_hw,out_hw", [((47, 101), (32, 64)), ((32, 64), (16, 32)), ((8, 16), (4, 8)), ((20, 40), (32, 64)),
                                          ((47, 64), (32, 64)), ((47, 101), (32, 63))])
def test_lanczos_resize_equals_the_cpu_path(device, in_hw, out_hw):
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(in_hw[0])
    img = _resize_images(in_hw, g)
    N = img.shape[0]
    ref = ip.LanczosResize(in_hw, out_hw, "cpu")
    want = ref(img)
    got = ip.LanczosResize(in_hw, out_hw, device, "hip")(img.to(device))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, 3) + out_hw and torch.equal(got.cpu(), want)
    # the first level: flip folded into the horizontal read (which then runs even between equal widths), the images given
    # as two tensors, and the mark of the images that hold a non-zero byte
    flip = torch.arange(N) % 3 == 1
    flip[7] = True
    flipped = torch.where(flip.reshape(-1, 1, 1, 1), img.flip(-1), img)
    first = ip.LanczosResize(in_hw, out_hw, device, "hip", first=True)
    assert (first.taps_h is not None) and (in_hw[1] != out_hw[1] or first.taps_h.shape[1] == 3)
    nonzero = torch.full((N,), 7, device=device, dtype=torch.int32)
    d = img.to(device)
    got = first([d[:4].contiguous(), d[4:].contiguous()], flip.to(device, torch.int32), nonzero)
    assert torch.equal(got.cpu(), ref(flipped))
    assert nonzero.tolist() == [1, 1, 1, 1, 1, 0, 1, 1]


def test_lanczos_resize_equals_pillow(device):
    from PIL import Image
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(9)
    in_hw, out_hw = (47, 101), (32, 64)
    img = _resize_images(in_hw, g)
    got = ip.LanczosResize(in_hw, out_hw, device, "hip")(img.to(device)).cpu()
    for n in range(img.shape[0]):
        im = Image.fromarray(img[n].permute(1, 2, 0).numpy()).resize((out_hw[1], out_hw[0]), Image.LANCZOS)
        assert np.array_equal(got[n].permute(1, 2, 0).numpy(), np.asarray(im)), n


# ---- 1b. planar frames through the generic-stride horizontal kernel -------------------------------------------------
def _carved(parts, device):
    """The host tensors as contiguous views of ONE device buffer of 255s, at the byte offsets 1, 7 (mod 16), 1, 7, ..."""
    starts, end = [], 0
    for k, t in enumerate(parts):
        start = -(-end // 16) * 16 + (1, 7)[k % 2]
        starts.append(start)
        end = start + t.numel()
    buf = torch.full((end + 16,), 255, dtype=torch.uint8, device=device)
    views = [buf[s:s + t.numel()].view(t.shape) for s, t in zip(starts, parts)]
    for v, t in zip(views, parts):
        v.copy_(t)
    assert [(v.data_ptr() - buf.data_ptr()) % 16 for v in views[:2]] == [1, 7][:len(views)] and buf.data_ptr() % 16 == 0
    return views


# shape -> (H, Wout), the flips, the images set to zero, the number of sources:
#   141 rows at 4 per workgroup: the last workgroup is partial; 101 is no multiple of the 16-byte pitch
#   C = 1 (rows per image = H), 10 rows per workgroup across image borders, flips and one blank image
#   an output wider than a workgroup: one row per workgroup
#   two sources off every alignment
PLANAR_CASES = {
    "partial_last_workgroup": ((1, 3, 47, 101), (47, 64), [0], [], 1),
    "one_channel_flips_blank": ((5, 1, 9, 40), (9, 24), [1, 0, 1, 1, 0], [3], 1),
    "one_row_per_workgroup": ((2, 3, 3, 333), (3, 300), [0, 1], [], 1),
    "two_unaligned_sources": ((4, 3, 5, 37), (5, 24), [0, 1, 1, 0], [2], 2),
}


@pytest.mark.parametrize("case", sorted(PLANAR_CASES))
def test_planar_frames_through_the_strided_horizontal_kernel(device, case):
    from PIL import Image
    from ppeadepth import input_pipeline as ip
    shape, out_hw, flips, blank, nsrc = PLANAR_CASES[case]
    N, C, in_hw = shape[0], shape[1], shape[2:]
    img = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(N * in_hw[1]), dtype=torch.uint8)
    img[:, :, 0, 0] = 255                                         # no image is blank by chance
    for n in blank:
        img[n] = 0
    flip = torch.tensor(flips, dtype=torch.bool)
    flipped = torch.where(flip.reshape(-1, 1, 1, 1), img.flip(-1), img)
    want = ip.LanczosResize(in_hw, out_hw, "cpu")(flipped)
    srcs = _carved(list(img.chunk(nsrc)), device)
    nonzero = torch.full((N,), 7, device=device, dtype=torch.int32)
    first = ip.LanczosResize(in_hw, out_hw, device, "hip", first=True)
    assert first.taps_v is None                                   # the horizontal pass alone
    got = first(srcs if nsrc > 1 else srcs[0], flip.to(device, torch.int32), nonzero)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, C) + out_hw and torch.equal(got.cpu(), want)
    assert nonzero.tolist() == [int(n not in blank) for n in range(N)]
    if not any(flips):                                            # and without the optional arguments
        assert torch.equal(first(srcs if nsrc > 1 else srcs[0]).cpu(), want)
    if C == 3:
        for n in range(N):
            im = Image.fromarray(flipped[n].permute(1, 2, 0).numpy()).resize((out_hw[1], out_hw[0]), Image.LANCZOS)
            assert np.array_equal(got[n].cpu().permute(1, 2, 0).numpy(), np.asarray(im)), n


# ---- 2. jitter, all orders ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ends", [False, True])
def test_color_jitter_every_operation_order(device, ends):
    from oracle import ref_jitter
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(21 + ends)
    B = len(ORDERS)
    img = torch.randint(0, 256, (B, 3, 8, 20), generator=g, dtype=torch.uint8)
    img[:, :, 0] = img[:, :1, 0]                                  # a gray row, a black and a white pixel in every item
    img[:, :, 1, 0], img[:, :, 1, 1] = 0, 255
    fixed = {}
    if ends:                                                      # the ends of the ranges; hue also at 0
        pick = lambda vals, step: [vals[(b // step) % len(vals)] for b in range(B)]      # noqa: E731
        fixed = dict(brightness=pick([0.8, 1.2], 1), contrast=pick([0.8, 1.2], 2), saturation=pick([0.8, 1.2], 4),
                     hue=pick([-0.1, 0.0, 0.1], 1))
    prm = _params(B, g, ORDERS, **fixed)
    apply = torch.arange(B) % 5 != 3
    got = _jitter_hip(img, prm, apply, device)
    want = ip.color_jitter(img, prm, apply)
    assert torch.equal(got, _unit(want))
    assert torch.equal(got[~apply], _unit(img[~apply])) and not torch.equal(got[apply], _unit(img[apply]))
    for b in range(B):
        pil = img[b].permute(1, 2, 0).numpy()
        if bool(apply[b]):
            pil = ref_jitter.color_jitter(pil, prm["order"][b].tolist(), float(prm["brightness"][b]), float(prm["contrast"][b]),
                                          float(prm["saturation"][b]), float(prm["hue"][b]))
        assert np.array_equal(want[b].permute(1, 2, 0).numpy(), pil), b


# ---- 3. jitter, colour cube -----------------------------------------------------------------------------------------
def test_color_jitter_colour_cube(device):
    from ppeadepth import input_pipeline as ip
    v = torch.arange(0, 256, 5)
    assert v[-1] == 255 and len(v) == 52
    cube = torch.stack(torch.meshgrid(v, v, v, indexing="ij")).reshape(1, 3, 52 * 52, 52).to(torch.uint8)
    orders = [[(k + j) % 4 for j in range(4)] for k in range(4)]
    img = cube.repeat(4, 1, 1, 1)
    prm = _params(4, torch.Generator().manual_seed(31), orders)
    apply = torch.ones(4, dtype=torch.bool)
    assert torch.equal(_jitter_hip(img, prm, apply, device), _unit(ip.color_jitter(img, prm, apply)))


# ---- 4. contrast mean on a .5 boundary ------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(13, 17), (192, 640)])
def test_contrast_mean_on_a_half_boundary(device, hw):
    """Gray images (L = the pixel value) of 100s and 101s whose sum puts mean(L) on the first value >= 100.5 (exactly 100.5
    for an even pixel count) and on the last one below it: int(mean + 0.5) is 101 and 100.  Once contrast runs first on
    that image; once on its double after brightness 0.5, which halves every (even) value exactly."""
    from ppeadepth import input_pipeline as ip
    HW = hw[0] * hw[1]
    g = torch.Generator().manual_seed(41)
    ones = -(-HW // 2)                                             # ceil(HW / 2) pixels of 101: mean >= 100.5
    imgs = []
    for count in (ones, ones - 1):
        gray = torch.full((HW,), 100, dtype=torch.uint8)
        gray[torch.randperm(HW, generator=g)[:count]] = 101
        assert (int(gray.sum()) / HW + 0.5 >= 101) == (count == ones)
        gray = gray.reshape(1, *hw).repeat(3, 1, 1)
        imgs += [gray, gray * 2]
    img = torch.stack(imgs)
    prm = _params(4, g, [[1, 0, 2, 3], [0, 1, 3, 2]] * 2, brightness=[1.1, 0.5] * 2, contrast=[1.2, 0.8] * 2)
    apply = torch.ones(4, dtype=torch.bool)
    want = ip.color_jitter(img, prm, apply)
    assert not torch.equal(want[0], want[2])                      # the two sides of the boundary do differ
    assert torch.equal(_jitter_hip(img, prm, apply, device), _unit(want))


# ---- 5. whole pipeline ----------------------------------------------------------------------------------------------
def _device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [(e.time_range.start, e.name) for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name]
    return [n for _, n in sorted(ev)]


def _pipeline_case(raw_hw, H, W, B, seed):
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(seed)
    raw = {f: torch.randint(0, 256, (B, 3) + raw_hw, generator=g, dtype=torch.uint8) for f in (0, -1, 1)}
    raw[1][B - 1] = 0                                             # a missing neighbour frame
    flip = torch.arange(B) % 2 == 1
    aug = torch.arange(B) != 1
    jit = {(f, s): ip.draw_jitter_params(B, g) for f in (0, -1, 1) for s in range(4)}
    return raw, aug, flip, jit


def _assert_same(got, want):
    assert list(got) == list(want) and len(got) == 32
    for k, v in want.items():
        assert got[k].dtype == torch.float32 and got[k].is_contiguous() and got[k].shape == v.shape, k
        assert torch.equal(got[k].cpu(), v), k


def test_pipeline_equals_the_cpu_path(device):
    from ppeadepth import input_pipeline as ip
    raw_hw, H, W, B = (47, 101), 32, 64, 3
    raw, aug, flip, jit = _pipeline_case(raw_hw, H, W, B, 51)
    want = ip.DeviceInputPipeline(raw_hw, H, W, "cpu")(raw, aug, flip, jit)
    pipe = ip.DeviceInputPipeline(raw_hw, H, W, device)
    assert pipe.backend == "hip"
    raw_d = {f: v.to(device) for f, v in raw.items()}
    got = pipe(raw_d, aug, flip, jit)
    _assert_same(got, want)
    assert torch.equal(got[("color_aug", 1, 0)][B - 1], got[("color", 1, 0)][B - 1])      # the blank frame is not jittered
    assert not got[("color", 1, 0)][B - 1].any()
    assert torch.equal(got[("color_aug", 0, 2)][1], got[("color", 0, 2)][1])              # nor the item without do_color_aug
    assert not torch.equal(got[("color_aug", 0, 2)][0], got[("color", 0, 2)][0])
    _assert_same(ip.DeviceInputPipeline(raw_hw, H, W, device, backend="torch")(raw_d, aug, flip, jit), want)
    with pytest.raises(ValueError):                               # flags on the device would need a copy back to the host
        pipe(raw_d, aug.to(device), flip, jit)
    again = pipe(raw_d, aug, flip, jit)                           # two calls: bitwise equal
    assert all(again[k].cpu().numpy().tobytes() == got[k].cpu().numpy().tobytes() for k in got)
    # parameters drawn inside the call come from the generator in the torch path's order
    seeded = [p(raw_d if p is pipe else raw, generator=torch.Generator().manual_seed(5))
              for p in (pipe, ip.DeviceInputPipeline(raw_hw, H, W, "cpu"))]
    _assert_same(*seeded)
    # launches: the same at B = 3 and B = 1, and none of them a library or ATen kernel
    one = {f: v[:1].contiguous() for f, v in raw_d.items()}
    jit1 = {k: {n: t[:1] for n, t in p.items()} for k, p in jit.items()}
    n3 = _device_events(lambda: pipe(raw_d, aug, flip, jit))
    n1 = _device_events(lambda: pipe(one, aug[:1], flip[:1], jit1))
    kernels = [n for n in n3 if re.search(r"lanczos_[hv]|jitter_(sum|out)|repeat_rows", n)]
    print(f"one pipeline call: {len(n3)} device events at B=3, {len(n1)} at B=1; kernels {len(kernels)}: {sorted(set(n3))}")
    assert len(kernels) == 17, "4 levels x (2 resize passes + 2 jitter launches) + the K / inv_K repeat"
    assert len(n1) == len(n3) <= 17 + 2                           # + the blank-mark memset and the parameter upload
    assert not [n for n in n3 if LIBRARY.search(n)]


def test_pipeline_at_the_workload_ratio(device):
    from ppeadepth import input_pipeline as ip
    raw_hw, H, W, B = (375, 1242), 192, 640, 2
    raw, aug, flip, jit = _pipeline_case(raw_hw, H, W, B, 61)
    want = ip.DeviceInputPipeline(raw_hw, H, W, "cpu")(raw, aug, flip, jit)
    _assert_same(ip.DeviceInputPipeline(raw_hw, H, W, device)(raw, aug, flip, jit), want)


# ---- 6. launches of the other three pipelines -----------------------------------------------------------------------
CONV_OR_GEMM = re.compile(r"Cijk_|igemm|ck::|ck_tile|miopen|MIOpen|gemm|Gemm|GEMM|rocblas|hipblaslt|conv|Conv")


def _cameras(B):
    cam = torch.zeros(B, 3, 3, dtype=torch.float64)
    cam[:, 0, 0], cam[:, 1, 1], cam[:, 2, 2] = 1131.0 + torch.arange(B), 1130.0 - torch.arange(B), 1
    cam[:, 0, 2], cam[:, 1, 2] = 523.0, 191.0 + torch.arange(B)
    return cam


def _ddad_call(device, B):
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(71)
    raw = {f: torch.randint(0, 256, (B, 3, 50, 77), generator=g, dtype=torch.uint8).to(device) for f in (0, -1)}
    pipe, cams = ip.DDADInputPipeline(device, 16, 24, (50, 77)), _cameras(B)
    return lambda: pipe(raw, cams)


def _cityscapes_training_call(device, B):
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(72)
    trip = torch.randint(0, 256, (B, 40, 3 * 52, 3), generator=g, dtype=torch.uint8)
    trip[B - 1, :, 2 * 52:] = 0                                   # a missing neighbour frame
    trip = trip.to(device)
    jit = {(f, s): ip.draw_jitter_params(B, g) for f in (0, -1, 1) for s in range(4)}
    pipe, cams = ip.CityscapesInputPipeline(device, 16, 24, (40, 52)), _cameras(B)
    aug, flip = torch.ones(B, dtype=torch.bool), torch.arange(B) % 2 == 0
    return lambda: pipe(trip, cams, aug, flip, jit)


def _cityscapes_eval_call(device, B):
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(73)
    raw = {f: torch.randint(0, 256, (B, 42, 64, 3), generator=g, dtype=torch.uint8).to(device) for f in (0, -1)}
    pipe, cams = ip.CityscapesEvalPipeline(device, 16, 24, (42, 64)), _cameras(B)
    return lambda: pipe(raw, cams)


# (the pipeline's kernels, memsets, fills, copies) of one call, as measured on the commit before the four pipelines got
# one core, which this one may not exceed: 4 levels x (2 resize passes + 2 jitter launches), + `repeat_rows` for DDAD; the
# memset of the blank-frame marks, or where nothing is jittered the fill of the all-zero parameter table (torch.zeros: an
# ATen fill kernel); the one host-to-device copy
PIPELINE_LAUNCHES = {
    "ddad": (_ddad_call, (17, 0, 1, 1)),
    "cityscapes_training": (_cityscapes_training_call, (16, 1, 0, 1)),
    "cityscapes_eval": (_cityscapes_eval_call, (16, 0, 1, 1)),
}


def _launch_counts(names):
    """(pipeline kernels, memsets, fills, copies, anything else)"""
    found = [len([n for n in names if re.search(p, n)])
             for p in (r"lanczos_[hv]|jitter_(sum|out)|repeat_rows", "Memset", "FillFunctor", "Memcpy")]
    return tuple(found) + (len(names) - sum(found),)


@pytest.mark.parametrize("which", sorted(PIPELINE_LAUNCHES))
def test_launches_do_not_depend_on_the_batch_size(device, which):
    make, expected = PIPELINE_LAUNCHES[which]
    n2, n1 = _device_events(make(device, 2)), _device_events(make(device, 1))
    print(f"{which}: {len(n2)} device events at B=2, {len(n1)} at B=1: {_launch_counts(n2)} {sorted(set(n2))}")
    assert _launch_counts(n2) == _launch_counts(n1) == expected + (0,) and len(n1) == len(n2)
    assert not [n for n in n2 if CONV_OR_GEMM.search(n)]
