"""Mixed-size KITTI batches on the GPU: the ragged level-0 launch pair (csrc/input_pipeline.hip, lanczos_h_ragged3 /
lanczos_v_ragged) against Pillow and the torch backend on the CPU, and `DeviceInputPipeline(None, ...)` "hip" against
"torch".  Every comparison is exact: the arithmetic is integer, or IEEE operations in a fixed order."""
import re

import numpy as np
import pytest
import torch

from test_kitti_ragged_cpu import AUG, FLIP, FRAMES, H, SCALES, SIZES, W, ragged_batch

pytestmark = pytest.mark.gpu

LIBRARY = re.compile(r"Cijk_|igemm|ck::|ck_tile|miopen|MIOpen|gemm_|Gemm|rocblas|hipblaslt|rocprim|hipcub|cub::|sort|Sort|"
                     r"at::native|elementwise|reduce_kernel")
KITTI_SIZES = [(375, 1242), (370, 1224), (374, 1238), (370, 1226), (376, 1241)]


def _checkerboard(hw):
    yy, xx = np.meshgrid(np.arange(hw[0]), np.arange(hw[1]), indexing="ij")
    return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, 2)      # both sides of the clip


def _random(hw, g):
    return g.integers(0, 256, tuple(hw) + (3,), dtype=np.uint8)


def _ragged_hip(items, out_hw, flips, device, fill=0xFF):
    """The launch pair on a list of HWC items (None: absent) -> (uint8 [N,3,Hout,Wout] on the host, nonzero list, frames)."""
    from ppeadepth import input_pipeline as ip, ops
    frames = ip.pack_frames({0: items}, (0,))
    level0 = ip.RaggedLevel0(out_hw, device, "hip")
    desc = level0.describe(frames)
    taps_h, taps_v = level0.tables()
    N, hcap = len(items), max(int(desc[:, 1].max()), 1)
    scratch = torch.full((N * 3 * hcap * out_hw[1],), fill, dtype=torch.uint8, device=device)      # an unwritten row shows
    nonzero = torch.full((N,), 7, dtype=torch.int32, device=device)
    got = ops.lanczos_resize_ragged_u8(frames.buf.to(device), desc, out_hw, taps_h, taps_v,
                                       torch.tensor(flips, dtype=torch.int32, device=device), nonzero, scratch)
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (N, 3) + tuple(out_hw)
    return got.cpu(), nonzero.tolist(), (frames, desc, taps_h, taps_v)


def _ragged_cpu(items, out_hw, flips):
    """The torch backend on the CPU, per item the `LanczosResize` of its size."""
    from ppeadepth import input_pipeline as ip
    out = []
    for it, fl in zip(items, flips):
        if it is None:
            out.append(torch.zeros((3,) + tuple(out_hw), dtype=torch.uint8))
            continue
        img = torch.from_numpy(it).permute(2, 0, 1)
        out.append(ip.LanczosResize(it.shape[:2], out_hw, "cpu")._torch(img.flip(-1) if fl else img))
    return torch.stack(out)


# ---- 5. the launch pair against Pillow, per image ---------------------------------------------------------------------
def test_ragged_resize_equals_pillow(device):
    from PIL import Image
    g = np.random.default_rng(11)
    up, same_w, same_h = (20, 40), (47, 64), (32, 70)             # upscaling; identity horizontal; identity vertical table
    out_hw = (32, 64)
    items = [_random(SIZES[0], g), _random(SIZES[1], g), np.zeros(SIZES[2] + (3,), np.uint8),
             np.full(SIZES[3] + (3,), 255, np.uint8), _checkerboard(up), None, _random(same_w, g), _random(same_h, g),
             _random(SIZES[0], g), _random(up, g)]
    flips = [0, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    got, nonzero, (frames, desc, taps_h, taps_v) = _ragged_hip(items, out_hw, flips, device)
    assert sum(int(o) % 16 != 0 for o in desc[:, 0]) >= 2         # packed back to back: off every alignment
    assert len(frames.sizes) == 7 and tuple(taps_h.shape[:2]) == (7, 64) and tuple(taps_v.shape[:2]) == (7, 32)
    kh = [int(taps_h[k, :, 1].max()) for k in range(7)]           # the classes' own kmax: the table's rows are padded
    assert max(kh) == taps_h.shape[2] - 2 and min(kh) == 1 and sorted(set(kh))[1] < max(kh) - 2
    assert int(taps_v[frames.sizes.index(same_h), :, 1].max()) == 1
    for n, (it, fl) in enumerate(zip(items, flips)):
        if it is None:
            assert not got[n].any()
            continue
        im = Image.fromarray(it)
        im = im.transpose(Image.FLIP_LEFT_RIGHT) if fl else im
        im = im.resize((out_hw[1], out_hw[0]), Image.LANCZOS)
        assert np.array_equal(got[n].permute(1, 2, 0).numpy(), np.asarray(im)), n
    assert nonzero == [1, 1, 0, 1, 1, 0, 1, 1, 1, 1]
    assert not got[2].any() and bool((got[3] == 255).all())


# ---- 6. workgroup geometry ------------------------------------------------------------------------------------------
def _geometry_cases():
    g = np.random.default_rng(12)
    mixed = [_random(hw, g) for hw in SIZES + [(20, 40), (47, 64), (32, 70)]]
    mixed.insert(3, None)
    wide = [_random((12, 700), g), _random((11, 690), g), _random((12, 700), g)]
    return {
        # 16 rows per workgroup, 285 rows: workgroups straddle images of different H and W; the last one is partial
        "rows_cross_image_borders": (mixed, (8, 16), [0, 1, 0, 0, 1, 0, 1, 0]),
        # an output wider than the workgroup's 256 threads: one row per workgroup
        "one_row_per_workgroup": (wide, (8, 300), [0, 1, 1]),
        # Wout % 4 != 0: the scalar vertical path
        "scalar_vertical_path": (mixed, (32, 63), [1, 0, 0, 1, 0, 0, 0, 1]),
        "one_image": ([_random((45, 97), g)], (32, 64), [1]),
        "all_absent": ([None, None], (8, 16), [0, 1]),
    }


GEOMETRY = _geometry_cases()


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_ragged_resize_workgroup_geometry(device, case):
    items, out_hw, flips = GEOMETRY[case]
    rows = sum(it.shape[0] for it in items if it is not None)
    if case == "rows_cross_image_borders":
        rpb = 256 // out_hw[1]
        starts = np.cumsum([0] + [0 if it is None else it.shape[0] for it in items])
        assert rpb == 16 and rows % rpb != 0 and any(s % rpb != 0 for s in starts[1:-1])
    got, nonzero, _ = _ragged_hip(items, out_hw, flips, device)
    assert torch.equal(got, _ragged_cpu(items, out_hw, flips))
    assert nonzero == [int(it is not None) for it in items]


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def _device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [(e.time_range.start, e.name) for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name]
    return [n for _, n in sorted(ev)]


def test_ragged_resize_refusals_launch_nothing(device):
    from ppeadepth import _abi, input_pipeline as ip, ops
    g = np.random.default_rng(13)
    items = [_random((9, 20), g), _random((7, 22), g)]
    frames = ip.pack_frames({0: items}, (0,))
    level0 = ip.RaggedLevel0((8, 16), device, "hip")
    desc = level0.describe(frames)
    taps_h, taps_v = level0.tables()
    buf = frames.buf.to(device)
    words = torch.cat([desc.reshape(-1), ops.ragged_row_prefix(desc)]).to(device)
    past, klass = desc.clone(), desc.clone()
    past[1, 1] += 1                                               # one row more than the buffer holds
    klass[0, 3] = 2                                               # K = 2
    out = torch.empty(2 * 3 * 10 * 16, dtype=torch.uint8, device=device)
    args = lambda d: (buf.data_ptr(), buf.numel(), d.data_ptr(), words.data_ptr(), words.data_ptr() + 32, 2,      # noqa: E731
                      taps_h.data_ptr(), 2, taps_h.shape[2] - 2, None, None, out.data_ptr(), 10, 16, None)
    torch.cuda.synchronize()

    def refused():
        for bad in (past, klass):
            with pytest.raises(_abi.PpeaKernelError):
                ops.lanczos_resize_ragged_u8(buf, bad, (8, 16), taps_h, taps_v)
            with pytest.raises(_abi.PpeaKernelError):             # ... also by the pair form, whose device copy is not read
                ops.lanczos_resize_ragged_u8(buf, (bad, words), (8, 16), taps_h, taps_v)
            assert _abi.lib.ppea_lanczos_h_ragged_u8(*args(bad)) == -2           # and by the entry point itself
        with pytest.raises(_abi.PpeaKernelError):
            ops.lanczos_resize_ragged_u8(frames.buf, desc, (8, 16), taps_h, taps_v)                  # a CPU tensor
        with pytest.raises(_abi.PpeaKernelError):
            ops.lanczos_resize_ragged_u8(buf.view(torch.int8), desc, (8, 16), taps_h, taps_v)        # not uint8
        with pytest.raises(_abi.PpeaKernelError):
            ops.lanczos_resize_ragged_u8(buf, desc.to(device), (8, 16), taps_h, taps_v)              # desc on the device
        with pytest.raises(_abi.PpeaKernelError):
            ops.lanczos_resize_ragged_u8(buf, desc, (8, 16), taps_h, taps_v, flip=torch.zeros(3, dtype=torch.int32, device=device))
        # a row too wide to be staged: 20 480 pixels are 61 440 bytes
        wide = torch.tensor([[0, 1, 20480, 0]], dtype=torch.int32)
        big = torch.zeros(61440, dtype=torch.uint8, device=device)
        a = list(args(wide))
        a[0], a[1], a[5] = big.data_ptr(), big.numel(), 1
        assert _abi.lib.ppea_lanczos_h_ragged_u8(*a) == -1

    names = _device_events(refused)
    assert not [n for n in names if re.search(r"lanczos|Memset", n)], names
    assert _abi.lib.ppea_lanczos_h_ragged_u8(*args(desc)) == 0    # the same arguments with the true descriptor are served
    torch.cuda.synchronize()


# ---- 8. the pipeline, "hip" against "torch" -----------------------------------------------------------------------------
def _jitter(B, seed):
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(seed)
    return {(f, s): ip.draw_jitter_params(B, g) for f in FRAMES for s in range(SCALES)}


def _assert_same(got, want):
    assert list(got) == list(want) and len(got) == 32
    for k, v in want.items():
        assert got[k].dtype == torch.float32 and got[k].is_contiguous() and got[k].shape == v.shape, k
        assert torch.equal(got[k].cpu(), v.cpu()), k


def test_ragged_pipeline_equals_the_cpu_path(device):
    from ppeadepth import input_pipeline as ip
    raw, jit = ragged_batch(), _jitter(4, 21)
    want = ip.DeviceInputPipeline(None, H, W, "cpu")(raw, AUG, FLIP, jit)
    pipe = ip.DeviceInputPipeline(None, H, W, device)
    assert pipe.backend == "hip"
    got = pipe(raw, AUG, FLIP, jit)
    _assert_same(got, want)
    for s in range(SCALES):                                       # the missing frame: zeros, never jittered
        assert not got[("color", -1, s)][2].any() and not got[("color_aug", -1, s)][2].any()
    assert not torch.equal(got[("color_aug", 0, 0)][0], got[("color", 0, 0)][0])
    _assert_same(pipe(ip.pack_frames(raw, FRAMES), AUG, FLIP, jit), want)       # pre-packed: the same call
    _assert_same(ip.DeviceInputPipeline(None, H, W, device, backend="torch")(raw, AUG, FLIP, jit), want)
    seeded = [p(raw, generator=torch.Generator().manual_seed(5)) for p in (pipe, ip.DeviceInputPipeline(None, H, W, "cpu"))]
    _assert_same(*seeded)                                         # parameters drawn inside the call: the torch path's order


def test_one_size_equals_the_fixed_size_pipeline(device):
    from ppeadepth import input_pipeline as ip
    g = torch.Generator().manual_seed(31)
    B, hw = 3, (47, 101)
    planar = {f: torch.randint(0, 256, (B, 3) + hw, generator=g, dtype=torch.uint8) for f in FRAMES}
    planar[1][B - 1] = 0                                          # a blank frame there, an absent one here
    items = {f: [v[b].permute(1, 2, 0).contiguous().numpy() for b in range(B)] for f, v in planar.items()}
    items[1][B - 1] = None
    aug, flip, jit = torch.tensor([True, False, True]), torch.tensor([False, True, True]), _jitter(B, 32)
    fixed = ip.DeviceInputPipeline(hw, H, W, device)({f: v.to(device) for f, v in planar.items()}, aug, flip, jit)
    ragged = ip.DeviceInputPipeline(None, H, W, device)(items, aug, flip, jit)
    assert list(fixed) == list(ragged)
    for k in fixed:
        assert fixed[k].cpu().numpy().tobytes() == ragged[k].cpu().numpy().tobytes(), k


# ---- 9. the five KITTI sizes, once --------------------------------------------------------------------------------------
def test_the_five_kitti_sizes(device):
    from ppeadepth import input_pipeline as ip
    g = np.random.default_rng(41)
    B = len(KITTI_SIZES)
    raw = {f: [_random(hw, g) for hw in KITTI_SIZES] for f in FRAMES}
    aug, flip, jit = torch.arange(B) % 3 == 1, torch.arange(B) % 2 == 0, _jitter(B, 42)
    pipe = ip.DeviceInputPipeline(None, 192, 640, device)
    got = pipe(raw, aug, flip, jit)
    assert (pipe.ragged.table_builds, pipe.ragged.table_uploads) == (5, 1) and sorted(pipe.ragged.classes) == sorted(KITTI_SIZES)
    _assert_same(got, ip.DeviceInputPipeline(None, 192, 640, device, backend="torch")(raw, aug, flip, jit))
    tables = (pipe.ragged.taps_h, pipe.ragged.taps_v)
    again = pipe({f: v[::-1] for f, v in raw.items()}, aug, flip, jit)          # the same sizes, in another order
    assert (pipe.ragged.table_builds, pipe.ragged.table_uploads) == (5, 1)      # no table built, none uploaded
    assert tables[0] is pipe.ragged.taps_h and tables[1] is pipe.ragged.taps_v
    assert torch.equal(again[("color", 0, 0)][0], got[("color", 0, 0)][B - 1])
    pipe({f: v + [_random((100, 300), g)] for f, v in raw.items()}, torch.zeros(B + 1, dtype=torch.bool),
         torch.zeros(B + 1, dtype=torch.bool), _jitter(B + 1, 43))
    assert (pipe.ragged.table_builds, pipe.ragged.table_uploads) == (6, 2)      # a new class: one build, one upload


# ---- 10. launch census ----------------------------------------------------------------------------------------------
KERNELS = r"lanczos_[hv]|jitter_(sum|out)|repeat_rows"


def test_ragged_launch_census(device):
    from ppeadepth import input_pipeline as ip
    raw, jit = ragged_batch(), _jitter(4, 51)
    pipe = ip.DeviceInputPipeline(None, H, W, device)
    frames = ip.pack_frames(raw, FRAMES)
    names = _device_events(lambda: pipe(frames, AUG, FLIP, jit))
    one_size = {f: [raw[0][0]] * 4 for f in FRAMES}
    same = _device_events(lambda: pipe(one_size, AUG, FLIP, jit))
    hw = SIZES[0]
    fixed_pipe = ip.DeviceInputPipeline(hw, H, W, device)
    planar = {f: torch.from_numpy(np.stack(v)).permute(0, 3, 1, 2).contiguous().to(device) for f, v in one_size.items()}
    fixed = _device_events(lambda: fixed_pipe(planar, AUG, FLIP, jit))
    kernels = [n for n in names if re.search(KERNELS, n)]
    print(f"ragged call: {len(names)} device events, kernels {len(kernels)}: {sorted(set(names))}; fixed-size call: {len(fixed)}")
    assert not [n for n in names if LIBRARY.search(n)]
    level0 = [n for n in kernels if re.search(r"ragged", n)]
    assert len(level0) == 2 and re.search("lanczos_h_ragged3", level0[0]) and re.search("lanczos_v_ragged", level0[1])
    assert len([n for n in same if re.search(r"ragged", n)]) == 2                # four size classes or one
    count = lambda ns: len([n for n in ns if re.search(KERNELS, n)])            # noqa: E731
    assert count(names) == count(same) == count(fixed) == 17
    # beside the kernels: the memset of the blank marks, the parameter copy, and here the one copy of the frame bytes
    assert len([n for n in names if "Memset" in n]) == len([n for n in fixed if "Memset" in n]) == 1
    assert len([n for n in names if "Memcpy" in n]) == 2 and len(names) == 17 + 3
