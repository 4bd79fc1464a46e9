"""The Cityscapes run on the host (no GPU): the two folder readers (paths against a hand-written table taken from the
reference's datasets/cityscapes_preprocessed_dataset.py:40, :96 and datasets/cityscapes_evaldataset.py:43-44, :75-80, :97-102;
contents against Pillow), reader + collate + pipeline against Pillow used the way the loaders use it, `train.main`'s preflight
and refusals, the `--dc` build order and the stage hand-over, the single-file ground truth (trainer.py:780) and the
device-resident validation store.

The reference's dataset classes import torchvision, which is not installed where this was written: there is no recorded
fixture of their output, the table below is the pin."""
import os

import numpy as np
import pytest
import torch

import cityscapes_folder

SCALES = 4
TRIPLET_HW, EVAL_HW, HW = (48, 64), (64, 128), (16, 24)

TRAIN_LINES = ["aachen aachen_000000_000019", "ulm ulm_000000_000020", "aachen aachen_000001_000021", "ulm ulm_000001_000022"]
TEST_LINES = ["aachen aachen_000000_000100", "ulm ulm_000001_000012", "aachen aachen_000002_000019"]
# per line: (image, camera) below --data_path
TRAIN_PATHS = [("aachen/aachen_000000_000019.jpg", "aachen/aachen_000000_000019_cam.txt"),
               ("ulm/ulm_000000_000020.jpg", "ulm/ulm_000000_000020_cam.txt"),
               ("aachen/aachen_000001_000021.jpg", "aachen/aachen_000001_000021_cam.txt"),
               ("ulm/ulm_000001_000022.jpg", "ulm/ulm_000001_000022_cam.txt")]
# per line: (frame 0, frame -1 = two frames earlier in the sequence folder, six digits, camera) below --cs_eval_path
TEST_PATHS = [("leftImg8bit/test/aachen/aachen_000000_000100_leftImg8bit.png",
               "leftImg8bit_sequence/test/aachen/aachen_000000_000098_leftImg8bit.png",
               "camera_trainvaltest/camera/test/aachen/aachen_000000_000100_camera.json"),
              ("leftImg8bit/test/ulm/ulm_000001_000012_leftImg8bit.png",
               "leftImg8bit_sequence/test/ulm/ulm_000001_000010_leftImg8bit.png",
               "camera_trainvaltest/camera/test/ulm/ulm_000001_000012_camera.json"),
              ("leftImg8bit/test/aachen/aachen_000002_000019_leftImg8bit.png",
               "leftImg8bit_sequence/test/aachen/aachen_000002_000017_leftImg8bit.png",
               "camera_trainvaltest/camera/test/aachen/aachen_000002_000019_camera.json")]


@pytest.fixture(scope="module")
def cs(tmp_path_factory):
    return cityscapes_folder.make(tmp_path_factory.mktemp("cs"), TRIPLET_HW, EVAL_HW, 4, 3)


def _files_below(root):
    return sorted(os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/") for d, _, fs in os.walk(root) for f in fs)


def _pil(path):
    from PIL import Image
    with Image.open(path) as img:
        return np.array(img.convert("RGB"))


# ---- the readers ---------------------------------------------------------------------------------------------------------
def test_reader_paths_equal_the_reference_table(cs):
    from ppeadepth import datasets
    assert cs["train"] == TRAIN_LINES and cs["test"] == TEST_LINES
    # the folders hold the table's files and no other: a reader that opens anything else fails below
    assert _files_below(cs["data"]) == sorted(p for row in TRAIN_PATHS for p in row)
    assert _files_below(cs["eval"]) == sorted(p for row in TEST_PATHS for p in row)
    tr = datasets.CityscapesPreprocessedDataset(cs["data"], cs["train"])
    ev = datasets.CityscapesEvalDataset(cs["eval"], cs["test"])
    assert len(tr) == 4 and len(ev) == 3
    for i, (img, cam) in enumerate(TRAIN_PATHS):
        city, name, side = tr.index_to_folder_and_frame_idx(i)
        assert side is None
        assert tr.get_image_path(city, name) == os.path.join(cs["data"], *img.split("/"))
        assert tr.get_camera_path(city, name) == os.path.join(cs["data"], *cam.split("/"))
        tr[i]
    for i, (f0, fm1, cam) in enumerate(TEST_PATHS):
        city, name, side = ev.index_to_folder_and_frame_idx(i)
        assert side is None
        assert ev.get_image_path(city, name) == os.path.join(cs["eval"], *f0.split("/"))
        assert ev.get_image_path(city, ev.get_offset_framename(name, -2), is_sequence=True) == os.path.join(cs["eval"], *fm1.split("/"))
        assert ev.get_camera_path(city, name) == os.path.join(cs["eval"], *cam.split("/"))
        ev[i]
    assert ev.get_offset_framename("ulm_000064_000012") == "ulm_000064_000010"       # -2 by default, six digits
    assert ev.get_offset_framename("ulm_000064_001000", -2) == "ulm_000064_000998"


def test_reader_items_are_pillows_decode(cs):
    from ppeadepth import datasets
    from ppeadepth import input_pipeline as ip
    tr = datasets.CityscapesPreprocessedDataset(cs["data"], cs["train"])
    assert tr.frame_hw == (48, 192) and tr.raw_hw == TRIPLET_HW
    for i, (img, cam) in enumerate(TRAIN_PATHS):
        item = tr[i]
        assert set(item) == {"triplet", "camera"}
        want = _pil(os.path.join(cs["data"], img))
        assert item["triplet"].dtype == np.uint8 and item["triplet"].shape == (48, 3 * 64, 3) and (item["triplet"] == want).all()
        assert item["camera"].dtype == np.float64 and (item["camera"] == ip.read_cityscapes_cam_txt(os.path.join(cs["data"], cam))).all()
        assert item["camera"][0, 0] == 1131.25 + i and item["camera"][1, 2] == 191.25 + i
    ev = datasets.CityscapesEvalDataset(cs["eval"], cs["test"])
    assert ev.raw_hw == EVAL_HW
    for i, (f0, fm1, cam) in enumerate(TEST_PATHS):
        item = ev[i]
        assert list(item) == [0, -1, "camera"]
        assert item[0].shape == (64, 128, 3) and (item[0] == _pil(os.path.join(cs["eval"], f0))).all()
        assert (item[-1] == _pil(os.path.join(cs["eval"], fm1))).all() and not (item[-1] == item[0]).all()
        assert (item["camera"] == ip.read_cityscapes_camera_json(os.path.join(cs["eval"], cam))).all()
    only0 = datasets.CityscapesEvalDataset(cs["eval"], cs["test"], frame_idxs=(0,))[1]
    assert list(only0) == [0, "camera"]
    with pytest.raises(ValueError):
        datasets.CityscapesEvalDataset(cs["eval"], cs["test"], frame_idxs=(0, -1, 1))


def test_the_thirds_are_frames_minus_one_zero_plus_one(tmp_path):
    """Three flat thirds of values 10, 20, 30: the pipeline's frame -1 is the left one, 0 the middle, +1 the right."""
    from PIL import Image
    from ppeadepth import datasets
    from ppeadepth.input_pipeline import CityscapesInputPipeline
    os.makedirs(tmp_path / "ulm")
    wide = np.concatenate([np.full((48, 64, 3), v, np.uint8) for v in (10, 20, 30)], 1)
    Image.fromarray(wide).save(str(tmp_path / "ulm" / "ulm_000000_000001.jpg"), quality=100)
    (tmp_path / "ulm" / "ulm_000000_000001_cam.txt").write_text("1131.0,0.0,523.0,0.0,1130.0,191.0,0.0,0.0,1.0\n")
    data = datasets.CityscapesPreprocessedDataset(str(tmp_path), ["ulm ulm_000000_000001"])
    trip, cams = datasets.collate_cityscapes([data[0]])
    out = CityscapesInputPipeline("cpu", *HW, data.raw_hw, is_train=False, backend="torch")(trip, cams)
    for f, v in ((-1, 10), (0, 20), (1, 30)):
        assert torch.equal(out[("color", f, 0)], torch.full((1, 3) + HW, float(v)) / 255), f


def test_another_size_and_a_missing_file_name_the_file(cs, tmp_path):
    import shutil
    from PIL import Image
    from ppeadepth import datasets
    root = tmp_path / "copy"
    shutil.copytree(cs["root"], root)
    data, raw = str(root / "cs_triplets"), str(root / "cityscapes")
    odd = os.path.join(data, *TRAIN_PATHS[2][0].split("/"))
    Image.fromarray(np.zeros((48, 195, 3), np.uint8)).save(odd)
    tr = datasets.CityscapesPreprocessedDataset(data, TRAIN_LINES)
    tr[1]
    with pytest.raises(ValueError) as e:
        tr[2]
    assert odd in str(e.value)
    odd = os.path.join(raw, *TEST_PATHS[1][1].split("/"))
    Image.fromarray(np.zeros((60, 128, 3), np.uint8)).save(odd)
    ev = datasets.CityscapesEvalDataset(raw, TEST_LINES)
    with pytest.raises(ValueError) as e:
        ev[1]
    assert odd in str(e.value)
    gone = os.path.join(raw, *TEST_PATHS[2][1].split("/"))          # the sequence frame: an error, never a blank frame
    os.remove(gone)
    with pytest.raises(FileNotFoundError) as e:
        ev[2]
    assert gone in str(e.value)


# ---- reader + collate + pipeline against Pillow --------------------------------------------------------------------------
def _pyramid(im, H, W):
    from PIL import Image
    out = []
    for s in range(SCALES):                                       # mono_dataset.py:96-100, chained
        im = im.resize((W // 2 ** s, H // 2 ** s), Image.LANCZOS)
        out.append(np.asarray(im))
    return out


def _unit(img_hwc):
    return torch.from_numpy(np.array(img_hwc)).permute(2, 0, 1).float() / 255           # ToTensor


def _loader_K(fx, fy, u0, v0, raw_width, raw_height, width, height, scale):
    K = np.array([[fx, 0, u0, 0], [0, fy, v0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]).astype(np.float32)
    K[0, :] /= raw_width
    K[1, :] /= raw_height
    K[0, :] *= width // (2 ** scale)
    K[1, :] *= height // (2 ** scale)
    return K, np.linalg.pinv(K)


def test_training_chain_from_the_files_is_pillow_byte_for_byte(cs):
    from PIL import Image
    from ppeadepth import datasets
    from ppeadepth.input_pipeline import CityscapesInputPipeline
    H, W = HW
    data = datasets.CityscapesPreprocessedDataset(cs["data"], cs["train"])
    idx = [1, 2, 3]
    trip, cams = datasets.collate_cityscapes([data[i] for i in idx])
    assert trip.dtype == torch.uint8 and tuple(trip.shape) == (3, 48, 192, 3) and tuple(cams.shape) == (3, 3, 3)
    assert not trip.is_pinned()
    flip = torch.tensor([True, False, True])
    out = CityscapesInputPipeline("cpu", H, W, data.raw_hw, backend="torch")(trip, cams, torch.zeros(3, dtype=torch.bool), flip)
    for b, i in enumerate(idx):
        with Image.open(os.path.join(cs["data"], TRAIN_PATHS[i][0])) as img:
            color = np.array(img.convert("RGB"))
        w = color.shape[1] // 3                                    # cityscapes_preprocessed_dataset.py:62-66
        thirds = {-1: Image.fromarray(color[:, :w]), 0: Image.fromarray(color[:, w:2 * w]), 1: Image.fromarray(color[:, 2 * w:])}
        for f, im in thirds.items():
            if bool(flip[b]):
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            for s, want in enumerate(_pyramid(im, H, W)):
                assert torch.equal(out[("color", f, s)][b], _unit(want)), (f, s, b)
                assert torch.equal(out[("color_aug", f, s)][b], _unit(want)), (f, s, b)
        for s in range(SCALES):
            K, inv_K = _loader_K(1131.25 + i, 1130.0 + 2 * i, 523.5 - i, 191.25 + i, 64, 48, W, H, s)
            assert (out[("K", s)][b].numpy() == K).all() and (out[("inv_K", s)][b].numpy() == inv_K).all()


def test_eval_chain_from_the_files_is_pillow_byte_for_byte(cs):
    from PIL import Image
    from ppeadepth import datasets
    from ppeadepth.input_pipeline import CityscapesEvalPipeline
    H, W = HW
    data = datasets.CityscapesEvalDataset(cs["eval"], cs["test"])
    raw, cams = datasets.collate_cityscapes_eval([data[i] for i in range(3)])
    assert list(raw) == [0, -1] and all(tuple(v.shape) == (3, 64, 128, 3) and v.dtype == torch.uint8 for v in raw.values())
    out = CityscapesEvalPipeline("cpu", H, W, data.raw_hw, backend="torch")(raw, cams)
    for i in range(3):
        for f, rel in ((0, TEST_PATHS[i][0]), (-1, TEST_PATHS[i][1])):
            with Image.open(os.path.join(cs["eval"], rel)) as img:
                color = img.convert("RGB")
            w, h = color.size                                      # cityscapes_evaldataset.py:66-68
            color = color.crop((0, 0, w, h * 3 // 4))
            for s, want in enumerate(_pyramid(color, H, W)):
                assert torch.equal(out[("color", f, s)][i], _unit(want)), (f, s, i)
        for s in range(SCALES):
            K, inv_K = _loader_K(2262.52 + i, 2265.3017905988554 - i, 1096.98 + i, 513.137 - i, 128, 64 * 0.75, W, H, s)
            assert (out[("K", s)][i].numpy() == K).all() and (out[("inv_K", s)][i].numpy() == inv_K).all()


# ---- train.main: preflight, refusals, build order ------------------------------------------------------------------------
class _Marker(Exception):
    pass


def _main_flags(cs, *more):
    return ["--data_path", cs["data"], "--cs_eval_path", cs["eval"], "--splits_dir", cs["splits"], "--num_workers", "0",
            "--device", "cpu", "--train_cs", "--adapter", "--use_checkpoint", "--weights_init", "scratch",
            "--batch_size", "2"] + list(more)


@pytest.fixture(scope="module")
def stage2_build(cs):
    """`train.main --train_cs --dc` up to the engine's construction, which is replaced by a marker: -> the trainer `main`
    built, as the engine would have received it."""
    from ppeadepth import dist, train
    seen = {}

    def engine(trainer, **kw):
        seen["trainer"], seen["kw"] = trainer, kw
        raise _Marker()
    real, dist.TrainEngine = dist.TrainEngine, engine
    try:
        with pytest.raises(_Marker):
            train.main(_main_flags(cs, "--dc", "--pytorch_random_seed", "5"))
    finally:
        dist.TrainEngine = real
    return seen["trainer"]


def test_main_gets_past_check_served_and_sizes_the_run_for_cityscapes(stage2_build):
    opt = stage2_build.opt
    assert (opt.dataset, opt.split, opt.eval_split, opt.height, opt.width) == \
        ("cityscapes_preprocessed", "cityscapes_preprocessed", "cityscapes", 192, 512)


def test_main_refuses_by_name(cs, tmp_path):
    from ppeadepth import train
    with pytest.raises(SystemExit) as e:
        train.main(["--data_path", str(tmp_path), "--splits_dir", str(tmp_path / "splits"), "--train_cs"])
    assert "--train_cs" in str(e.value) and os.path.join(str(tmp_path / "splits"), "cityscapes_preprocessed", "train_files.txt") in str(e.value)
    assert "not found" in str(e.value)
    with pytest.raises(SystemExit) as e:                            # the split is there, the first image is not
        train.main(["--data_path", str(tmp_path), "--splits_dir", cs["splits"], "--train_cs"])
    assert str(e.value).startswith("--train_cs: " + os.path.join(str(tmp_path), "aachen", "aachen_000000_000019.jpg") + " not found")
    for more in (["--use_future_frame"], ["--num_matching_frames", "2"]):
        with pytest.raises(SystemExit) as e:
            train.main(_main_flags(cs, *more))
        assert "--train_cs" in str(e.value) and "--use_future_frame" in str(e.value)
    a = train._run_parser().parse_args(["--data_path", "x"])
    assert a.cs_eval_path == "../cityscapes"


def _is_adapter(name):
    return "adpt" in name or "adapter" in name


def test_dc_build_order_and_the_stage_hand_over(stage2_build):
    from ppeadepth import networks, options
    model = stage2_build._module()
    assert model.dc and next(model.parameters()).device.type == "cpu"
    for dec in (model.depth, model.mono_depth):
        named = dict(dec.named_parameters())
        adapters = [n for n in named if _is_adapter(n)]
        assert adapters and all(named[n].requires_grad for n in adapters)
        assert all(not p.requires_grad for n, p in named.items() if not _is_adapter(n))
    keys = {n for n, _ in model.named_parameters() if n.startswith(("depth.", "mono_depth.")) and _is_adapter(n)}
    before = {k: v.clone() for k, v in model.state_dict().items()}
    # a Stage-1 document: no adapter key, so the adapters keep their fresh draws and everything else is the checkpoint's
    torch.manual_seed(21)
    stage1 = networks.RepDepth(options.default_options(height=192, width=512, batch_size=2)).state_dict()
    assert not keys & set(stage1)
    res = model.load_state_dict(stage1, strict=False)
    assert not res.unexpected_keys and keys <= set(res.missing_keys)
    after = model.state_dict()
    assert all(torch.equal(after[k], before[k]) for k in keys)
    assert all(torch.equal(after[k], v) for k, v in stage1.items())
    assert any(not torch.equal(before[k], v) for k, v in stage1.items() if v.dtype.is_floating_point)
    # a Stage-2 document restores the adapters
    torch.manual_seed(22)
    other = networks.RepDepth(options.default_options(height=192, width=512, batch_size=2, dc=True))
    other.dc_ft_init()
    stage2 = other.state_dict()
    assert keys <= set(stage2) and any(not torch.equal(stage2[k], before[k]) for k in keys)
    res = model.load_state_dict(stage2, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(model.state_dict()[k], stage2[k]) for k in keys)


# ---- the ground truth from single files ----------------------------------------------------------------------------------
def test_ground_truth_from_the_folder_equals_the_list_constructor(tmp_path):
    from ppeadepth.evaluate import DeviceGroundTruth
    g = np.random.default_rng(2)
    folder = tmp_path / "splits" / "cityscapes" / "gt_depths"
    os.makedirs(folder)
    count = 1001                                                    # index 1000: zfill(3) pads, it does not truncate
    maps = [g.uniform(0.0, 80.0, (2 + i % 3, 3 + i % 2)).astype(np.float32 if i % 5 else np.float64) for i in range(count)]
    for i, m in enumerate(maps):
        name = {0: "000_depth.npy", 7: "007_depth.npy", 42: "042_depth.npy", 999: "999_depth.npy", 1000: "1000_depth.npy"}.get(
            i, str(i).zfill(3) + "_depth.npy")
        np.save(str(folder / name), m)
    got, want = DeviceGroundTruth.from_folder(str(folder), count, "cpu"), DeviceGroundTruth(maps, "cpu")
    assert len(got) == count and got.shapes == want.shapes and got.device == want.device
    assert got.flat.dtype == torch.float32 and torch.equal(got.flat, want.flat)
    assert got.table.dtype == torch.int64 and torch.equal(got.table, want.table)
    os.remove(str(folder / "1000_depth.npy"))
    with pytest.raises(FileNotFoundError) as e:
        DeviceGroundTruth.from_folder(str(folder), count, "cpu")
    assert str(folder / "1000_depth.npy") in str(e.value) and "cityscapes/gt_depths" in str(e.value)
    assert "gt_depths_cityscapes.zip" in str(e.value)
    with pytest.raises(FileNotFoundError) as e:
        DeviceGroundTruth.from_folder(str(tmp_path / "nowhere"), 3, "cpu")
    assert str(tmp_path / "nowhere") in str(e.value)


# ---- the store -----------------------------------------------------------------------------------------------------------
def _loader_batches(N, B, frame_ids, plane, all_levels=False, seed=4):
    """What the evaluation pipeline hands on, level 0 only: colours k / 255 by ToTensor's true division, random K / inv_K,
    and entries the store must not keep."""
    g = torch.Generator().manual_seed(seed)
    unit = torch.full((), 255.0)
    out = []
    for b0 in range(0, N, B):
        n = min(B, N - b0)
        data = {}
        for f in frame_ids:
            k = torch.randint(0, 256, (n,) + plane, generator=g, dtype=torch.uint8)
            if all_levels:
                k.view(n, -1)[:, :256] = torch.arange(256, dtype=torch.uint8)
            data[("color", f, 0)] = k.to(torch.float32) / unit
            data[("color_aug", f, 0)] = data[("color", f, 0)].clone()
            data[("color", f, 1)] = torch.rand((n, 3, 2, 2), generator=g)
        for s in range(SCALES):
            data[("K", s)], data[("inv_K", s)] = torch.rand((n, 4, 4), generator=g), torch.rand((n, 4, 4), generator=g)
        out.append(data)
    return out


@pytest.mark.parametrize("N,B,frame_ids,plane,all_levels", [
    (5, 2, (0, -1), (3, 5, 7), False),                             # a partial last batch; no size a multiple of 16
    (5, 2, (0,), (3, 5, 7), False),                                # F = 1
    (3, 3, (0, -1), (3, 16, 16), True),                            # every byte value, in every item of both frames
    (4, 1, (0, -1, -2), (3, 1, 1), False)], ids=["partial", "one-frame", "all-levels", "three-frames"])
def test_store_batches_equal_loader_batches(N, B, frame_ids, plane, all_levels):
    from ppeadepth.valstore import ValidationStore
    loader = _loader_batches(N, B, frame_ids, plane, all_levels)
    if all_levels:
        assert all(len(torch.unique(d[("color", f, 0)][i])) == 256 for d in loader for f in frame_ids for i in range(B))
    store = ValidationStore(frame_ids, N, "cpu", torch.full((), 255.0), "torch")
    with pytest.raises(ValueError):
        list(store.batches(B))                                     # nothing to read before a complete pass
    for d in loader:
        store.add(d)
    store.finish()
    assert store.complete and store.colors.dtype == torch.uint8 and tuple(store.colors.shape) == (N, len(frame_ids)) + plane
    assert store.nbytes() == N * len(frame_ids) * int(np.prod(plane)) + 2 * N * 16 * 4
    for _ in range(2):                                             # every later validation reads the same batches
        got = list(store.batches(B))
        assert len(got) == len(loader)
        for a, b in zip(got, loader):
            assert set(a) == {("color", f, 0) for f in frame_ids} | {("K", 2), ("inv_K", 2)}
            for k in a:
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_store_raises_on_a_value_that_is_no_byte_over_255():
    from ppeadepth.valstore import ValidationStore, ValidationStoreError
    # a level at which the product with the reciprocal is not the quotient: what a pipeline that multiplied would hand on
    k = next(k for k in range(256) if np.float32(k) * np.float32(1.0 / 255) != np.float32(k) / np.float32(255))
    for bad in (0.5 / 255, np.float32(k) * np.float32(1.0 / 255), float("nan"), 256.0 / 255):
        loader = _loader_batches(3, 2, (0, -1), (3, 5, 7))
        loader[1][("color", -1, 0)][0, 2, 4, 6] = float(bad)
        store = ValidationStore((0, -1), 3, "cpu", torch.full((), 255.0), "torch")
        for d in loader:
            store.add(d)
        with pytest.raises(ValidationStoreError):
            store.finish()
        assert not store.complete
    store = ValidationStore((0, -1), 3, "cpu", torch.full((), 255.0), "torch")
    store.add(_loader_batches(3, 2, (0, -1), (3, 5, 7))[0])
    with pytest.raises(ValueError):
        store.finish()                                             # 2 of 3 items
