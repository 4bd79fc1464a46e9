"""Mixed-size KITTI batches on the CPU: the torch backend of `DeviceInputPipeline(None, ...)` against Pillow itself, the
packing of ragged frames, the on-disk reader and the two new entry points.  Every comparison is exact."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(47, 101), (45, 97), (48, 100), (46, 103)]
FRAMES = (0, -1, 1)
H, W, SCALES = 32, 64, 4


def ragged_batch(seed=5):
    """B = 4 items x frames (0, -1, 1), one size per item; item 2 has no frame -1.  -> {frame id: list of HWC arrays}"""
    g = np.random.default_rng(seed)
    raw = {f: [g.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in SIZES] for f in FRAMES}
    raw[-1][2] = None
    return raw


FLIP = torch.tensor([True, False, False, True])
AUG = torch.tensor([True, True, False, True])


def pillow_pyramid(item, flip):
    """One frame through Pillow as the reference's loader runs it: flip, then the chained LANCZOS resizes."""
    from PIL import Image
    img = Image.fromarray(item)
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    out = []
    for s in range(SCALES):
        img = img.resize((W >> s, H >> s), Image.LANCZOS)
        out.append(torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).to(torch.float32) / 255.0)
    return out


def pillow_colors(raw):
    """{("color", f, s): fp32 [B,3,h,w]} by Pillow, per item; a missing frame is zeros."""
    want = {}
    for f in FRAMES:
        per_item = [pillow_pyramid(it, bool(FLIP[b])) if it is not None else
                    [torch.zeros(3, H >> s, W >> s) for s in range(SCALES)] for b, it in enumerate(raw[f])]
        for s in range(SCALES):
            want[("color", f, s)] = torch.stack([p[s] for p in per_item])
    return want


@pytest.fixture(scope="module")
def batch():
    raw = ragged_batch()
    return raw, pillow_colors(raw)


def _assert_colors(got, want):
    for k, v in want.items():
        assert got[k].dtype == torch.float32 and got[k].shape == v.shape and torch.equal(got[k].cpu(), v), k


# ---- 1. the torch backend against Pillow --------------------------------------------------------------------------
def test_torch_backend_equals_pillow(batch):
    from ppeadepth import input_pipeline as ip
    raw, want = batch
    pipe = ip.DeviceInputPipeline(None, H, W, "cpu")
    assert pipe.backend == "torch"
    got = pipe(raw, AUG, FLIP, generator=torch.Generator().manual_seed(3))
    assert len(got) == 2 * len(FRAMES) * SCALES + 2 * SCALES
    _assert_colors(got, want)
    for s in range(SCALES):                                       # the missing frame: zeros, and never jittered
        assert not got[("color", -1, s)][2].any() and not got[("color_aug", -1, s)][2].any()
        assert got[("K", s)].shape == (4, 4, 4)
    assert not torch.equal(got[("color_aug", 0, 0)][0], got[("color", 0, 0)][0])      # the others are
    assert torch.equal(got[("color_aug", 0, 0)][2], got[("color", 0, 0)][2])          # but not the item without do_color_aug
    assert sorted(pipe.ragged.classes) == sorted(SIZES) and pipe.ragged.table_builds == 4
    # a pre-packed batch is the same call
    again = pipe(ip.pack_frames(raw, FRAMES, pin=False), AUG, FLIP, generator=torch.Generator().manual_seed(3))
    assert list(again) == list(got) and all(torch.equal(again[k], got[k]) for k in got)
    assert pipe.ragged.table_builds == 4


def test_a_size_tuple_still_selects_the_fixed_size_pipeline():
    from ppeadepth import input_pipeline as ip
    pipe = ip.DeviceInputPipeline((47, 101), H, W, "cpu")
    assert pipe.ragged is None and pipe.resize[0] is not None
    g = torch.Generator().manual_seed(1)
    raw = {f: torch.randint(0, 256, (2, 3, 47, 101), generator=g, dtype=torch.uint8) for f in FRAMES}
    flip, aug = torch.tensor([True, False]), torch.tensor([False, False])
    fixed = pipe(raw, aug, flip)
    items = {f: [v[b].permute(1, 2, 0).contiguous() for b in range(2)] for f, v in raw.items()}      # tensors as items
    ragged = ip.DeviceInputPipeline(None, H, W, "cpu")(items, aug, flip)
    assert list(fixed) == list(ragged) and all(torch.equal(fixed[k], ragged[k]) for k in fixed)


# ---- 2. pack_frames -------------------------------------------------------------------------------------------------
def test_pack_frames_layout(batch):
    from ppeadepth import input_pipeline as ip, ops
    raw, _ = batch
    fr = ip.pack_frames(raw, FRAMES, pin=False)
    B, N = 4, 12
    assert fr.batch == B and len(fr) == N and fr.desc.dtype == torch.int32 and tuple(fr.desc.shape) == (N, 4)
    assert fr.buf.dtype == torch.uint8 and fr.buf.dim() == 1 and fr.sizes == SIZES
    off = 0
    for n in range(N):                                            # frame-major: image n = fi * B + b
        item = raw[FRAMES[n // B]][n % B]
        if item is None:
            assert fr.desc[n].tolist() == [off, 0, 0, 0] and fr.image(n) is None
            continue
        h, w = item.shape[:2]
        assert fr.desc[n].tolist() == [off, h, w, SIZES.index((h, w))]
        assert np.array_equal(fr.image(n).numpy(), item)
        off += h * w * 3
    assert fr.buf.numel() == off
    prefix = ops.ragged_row_prefix(fr.desc)
    assert prefix.dtype == torch.int32 and prefix.tolist() == [0] + np.cumsum(fr.desc[:, 1].numpy()).tolist()
    assert prefix[N] == sum(it.shape[0] for f in FRAMES for it in raw[f] if it is not None)
    with pytest.raises(ValueError):
        ip.pack_frames({0: raw[0], -1: raw[-1][:3], 1: raw[1]}, FRAMES, pin=False)
    with pytest.raises(ValueError):
        ip.pack_frames({0: [raw[0][0].astype(np.float32)]}, (0,), pin=False)


def test_two_gib_of_frames_are_refused_before_anything_is_allocated():
    from ppeadepth import input_pipeline as ip
    big = (16384, 16384)                                          # 805 306 368 bytes each
    desc, sizes, total = ip.ragged_layout([big, None, big])
    assert total == 2 * 16384 * 16384 * 3 < 1 << 31 and desc[2].tolist() == [16384 * 16384 * 3, 16384, 16384, 0]
    with pytest.raises(ValueError, match="2\\^31"):
        ip.ragged_layout([big, big, big])
    # the boundary: 2^31 - 2 bytes pass, 2^31 + 1 do not (no multiple of 3 lies between)
    assert ip.ragged_layout([big, big, (1, 178956970)])[2] == (1 << 31) - 2
    with pytest.raises(ValueError, match="2\\^31"):
        ip.ragged_layout([big, big, (1, 178956971)])
    fake = torch.empty((16384, 16384, 3), dtype=torch.uint8, device="meta")      # a size without its bytes
    with pytest.raises(ValueError, match="2\\^31"):
        ip.pack_frames({0: [fake, fake, fake]}, (0,), pin=False)


# ---- 3. the on-disk reader ----------------------------------------------------------------------------------------
def _write_tree(root, raw):
    """Item b of `raw` as folder day_b/drive, frames 5 + f, camera 2 for even b and 3 for odd b; lossless PNG."""
    from PIL import Image
    lines = []
    for b in range(len(raw[0])):
        side = "lr"[b % 2]
        folder = f"day_{b}/drive_{b}_sync"
        for f in FRAMES:
            if raw[f][b] is None:
                continue
            d = os.path.join(root, folder, "image_0%d" % (2 + b % 2), "data")
            os.makedirs(d, exist_ok=True)
            Image.fromarray(raw[f][b]).save(os.path.join(d, "%010d.png" % (5 + f)))
        lines.append(f"{folder} 5 {side}")
    return lines


def test_kitti_raw_dataset_reads_what_was_written(batch, tmp_path):
    from ppeadepth import datasets, input_pipeline as ip
    raw, want = batch
    lines = _write_tree(str(tmp_path), raw)
    split = tmp_path / "train_files.txt"
    split.write_text("\n".join(lines) + "\n")
    assert datasets.readlines(str(split)) == lines
    data = datasets.KITTIRAWDataset(str(tmp_path), lines, FRAMES, img_ext=".png")
    assert len(data) == 4
    assert data.index_to_folder_and_frame_idx(1) == ("day_1/drive_1_sync", 5, "r")
    assert data.get_image_path("a/b", 7, "l") == os.path.join(str(tmp_path), "a/b", "image_02/data", "0000000007.png")
    assert data.get_image_path("a/b", 7, "r") == os.path.join(str(tmp_path), "a/b", "image_03/data", "0000000007.png")
    assert datasets.KITTIRAWDataset("/d", [], (0,)).get_image_path("a", 12, "l") == "/d/a/image_02/data/0000000012.jpg"
    items = [data[i] for i in range(4)]
    for b, item in enumerate(items):
        assert list(item) == list(FRAMES)
        for f in FRAMES:
            if raw[f][b] is None:
                assert item[f] is None                            # a neighbour that does not exist
            else:
                assert item[f].dtype == np.uint8 and np.array_equal(item[f], raw[f][b])
    # a missing frame 0 is an error, with the hint
    gone = datasets.KITTIRAWDataset(str(tmp_path), ["day_0/drive_0_sync 900 l"], FRAMES, img_ext=".png")
    with pytest.raises(FileNotFoundError, match="--data_path"):
        gone[0]
    with pytest.raises(FileNotFoundError, match="--png"):
        datasets.KITTIRAWDataset(str(tmp_path), lines, FRAMES)[0]             # the default extension is .jpg
    with pytest.raises(ValueError):
        datasets.KITTIRAWDataset(str(tmp_path), lines, (0, "s"))
    # collate -> the pipeline: the same dictionary as Pillow's
    frames = datasets.collate_raw(items)
    assert isinstance(frames, ip.RaggedFrames) and frames.batch == 4 and len(frames) == 12
    got = ip.DeviceInputPipeline(None, H, W, "cpu")(frames, AUG, FLIP, generator=torch.Generator().manual_seed(3))
    _assert_colors(got, want)
    direct = ip.DeviceInputPipeline(None, H, W, "cpu")(raw, AUG, FLIP, generator=torch.Generator().manual_seed(3))
    assert list(got) == list(direct) and all(torch.equal(got[k], direct[k]) for k in got)
    # and as a DataLoader's collate_fn
    loader = torch.utils.data.DataLoader(data, batch_size=4, collate_fn=datasets.collate_raw)
    (only,) = list(loader)
    assert torch.equal(only.buf, frames.buf) and torch.equal(only.desc, frames.desc)


# ---- 4. ABI ---------------------------------------------------------------------------------------------------------
def test_ragged_entry_points_in_header_abi_and_library():
    from ppeadepth import _abi
    with open(os.path.join(ROOT, "include", "ppea_depth.h")) as f:
        header = f.read()
    assert _abi.lib.ppea_abi_version() == _abi.ABI_VERSION >= 28         # 28: the version these entry points arrived with
    for name in ("ppea_lanczos_h_ragged_u8", "ppea_lanczos_v_ragged_u8"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_abi.SIGNATURES[name]), name
        assert hasattr(_abi.lib, name)
