"""Cityscapes on the host (no GPU): `CityscapesInputPipeline` / `CityscapesEvalPipeline` with backend "torch" byte for byte
against Pillow itself, used the way the two loaders use it (datasets/cityscapes_preprocessed_dataset.py:55-72,
datasets/cityscapes_evaldataset.py:59-73, then MonoDataset.preprocess); the per-sample, per-level intrinsics against the
loaders' formula in numpy float32; the two camera-file readers; `--train_cs`; the ABI of the view pass."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

SCALES = 4


# ---- shared inputs (tests/test_cityscapes_pipeline_gpu.py builds the same ones) -----------------------------------------
def cameras(B, seed=5):
    """B distinct float64 [3,3] cameras around the preprocessed triplets' (fx, fy, u0, v0)."""
    g = np.random.default_rng(seed)
    cam = np.zeros((B, 3, 3))
    cam[:, 0, 0], cam[:, 1, 1] = 1131.0 * g.uniform(0.9, 1.1, B), 1130.0 * g.uniform(0.9, 1.1, B)
    cam[:, 0, 2], cam[:, 1, 2] = 523.0 * g.uniform(0.9, 1.1, B), 191.0 * g.uniform(0.9, 1.1, B)
    cam[:, 2, 2] = 1
    return cam


def training_case():
    """B = 3, 40 x 156 wide images (windows at byte offsets 0, 156, 312), flips [1,0,1], item 2 without jitter, item 1's
    frame +1 all zeros."""
    B, raw_hw, hw = 3, (40, 52), (16, 24)
    g = torch.Generator().manual_seed(7)
    trip = torch.randint(0, 256, (B, raw_hw[0], 3 * raw_hw[1], 3), generator=g, dtype=torch.uint8)
    trip[0, :, : raw_hw[1] // 2] //= 16                         # a dark half and a saturated corner
    trip[2, : raw_hw[0] // 3, -(raw_hw[1] // 3):] = 255
    trip[1, :, 2 * raw_hw[1]:] = 0
    from ppeadepth import input_pipeline as ip
    jitter = {(f, s): ip.draw_jitter_params(B, g) for f in (0, -1, 1) for s in range(SCALES)}
    return dict(B=B, raw_hw=raw_hw, hw=hw, triplets=trip, cameras=cameras(B), do_flip=torch.tensor([True, False, True]),
                do_color_aug=torch.tensor([True, True, False]), jitter=jitter)


def eval_case(raw_hw, B=3):
    """Raw frames whose rows below the crop are 255: a crop that is off by one row changes bytes."""
    g = torch.Generator().manual_seed(raw_hw[0])
    raw = {f: torch.randint(0, 256, (B,) + raw_hw + (3,), generator=g, dtype=torch.uint8) for f in (0, -1)}
    for f in raw:
        raw[f][:, raw_hw[0] * 3 // 4:] = 255
    return dict(B=B, raw_hw=raw_hw, hw=(16, 24), raw=raw, cameras=cameras(B, seed=9) * 2.0)


# ---- Pillow, as the loaders use it ----------------------------------------------------------------------------------
def _pyramid(im, H, W):
    from PIL import Image
    out = []
    for s in range(SCALES):                                       # mono_dataset.py:96-100, chained
        im = im.resize((W // 2 ** s, H // 2 ** s), Image.LANCZOS)
        out.append(np.asarray(im))
    return out


def _unit(img_hwc):
    return torch.from_numpy(np.array(img_hwc)).permute(2, 0, 1).float() / 255           # ToTensor


def test_training_pipeline_is_pillow_byte_for_byte():
    from PIL import Image
    from oracle import ref_jitter
    from ppeadepth.input_pipeline import CityscapesInputPipeline
    c = training_case()
    (H, W), (Hraw, Wraw), B = c["hw"], c["raw_hw"], c["B"]
    pipe = CityscapesInputPipeline("cpu", H, W, c["raw_hw"], backend="torch")
    out = pipe(c["triplets"], c["cameras"], c["do_color_aug"], c["do_flip"], c["jitter"])
    assert len(out) == 2 * 3 * SCALES + 2 * SCALES
    for b in range(B):
        color = c["triplets"][b].numpy()
        w = color.shape[1] // 3                                    # cityscapes_preprocessed_dataset.py:62-66
        assert w == Wraw
        thirds = {-1: Image.fromarray(color[:, :w]), 0: Image.fromarray(color[:, w:2 * w]), 1: Image.fromarray(color[:, 2 * w:])}
        for f, im in thirds.items():
            if bool(c["do_flip"][b]):
                im = im.transpose(Image.FLIP_LEFT_RIGHT)           # each third on its own
            blank = not np.asarray(im).any()
            assert blank == (b == 1 and f == 1)
            for s, want in enumerate(_pyramid(im, H, W)):
                got = out[("color", f, s)][b]
                assert got.dtype == torch.float32 and tuple(got.shape) == (3, H // 2 ** s, W // 2 ** s)
                assert torch.equal(got, _unit(want)), ("color", f, s, b)
                p = c["jitter"][(f, s)]
                if bool(c["do_color_aug"][b]) and not blank:       # mono_dataset.py:107-112
                    want = ref_jitter.color_jitter(want, p["order"][b].tolist(), float(p["brightness"][b]),
                                                   float(p["contrast"][b]), float(p["saturation"][b]), float(p["hue"][b]))
                    assert not torch.equal(_unit(want), got)
                assert torch.equal(out[("color_aug", f, s)][b], _unit(want)), ("color_aug", f, s, b)
    with pytest.raises(ValueError):
        pipe(torch.zeros(B, Hraw, 3 * Wraw + 1, 3, dtype=torch.uint8), c["cameras"])        # 157 wide
    with pytest.raises(ValueError):
        pipe(c["triplets"], c["cameras"][:2])


def test_training_pipeline_draws_nothing_when_not_training():
    from ppeadepth.input_pipeline import CityscapesInputPipeline
    c = training_case()
    out = CityscapesInputPipeline("cpu", *c["hw"], c["raw_hw"], is_train=False)(c["triplets"], c["cameras"])
    off = torch.zeros(c["B"], dtype=torch.bool)
    want = CityscapesInputPipeline("cpu", *c["hw"], c["raw_hw"])(c["triplets"], c["cameras"], off, off)
    assert out.keys() == want.keys() and all(torch.equal(out[k], want[k]) for k in out)
    assert all(torch.equal(out[("color_aug", f, s)], out[("color", f, s)]) for f in (0, -1, 1) for s in range(SCALES))


@pytest.mark.parametrize("raw_hw", [(42, 64), (40, 64)])
def test_eval_pipeline_is_pillow_byte_for_byte(raw_hw):
    from PIL import Image
    from ppeadepth.input_pipeline import CityscapesEvalPipeline
    c = eval_case(raw_hw)
    H, W = c["hw"]
    pipe = CityscapesEvalPipeline("cpu", H, W, raw_hw, backend="torch")
    out = pipe(c["raw"], c["cameras"])
    assert len(out) == 2 * 2 * SCALES + 2 * SCALES and pipe.crop_h == {42: 31, 40: 30}[raw_hw[0]]
    for f in (0, -1):
        for b in range(c["B"]):
            color = Image.fromarray(c["raw"][f][b].numpy())
            w, h = color.size                                      # cityscapes_evaldataset.py:66-68
            crop_h = h * 3 // 4
            color = color.crop((0, 0, w, crop_h))
            for s, want in enumerate(_pyramid(color, H, W)):
                assert torch.equal(out[("color", f, s)][b], _unit(want)), (f, s, b)
                assert torch.equal(out[("color_aug", f, s)][b], out[("color", f, s)][b])
    with pytest.raises(ValueError):
        pipe({f: v.permute(0, 3, 1, 2) for f, v in c["raw"].items()}, c["cameras"])         # planar frames


def _loader_K(cam, raw_width, raw_height, width, height, scale):
    """load_intrinsics of the two loaders, then mono_dataset.py:173-182, in numpy float32."""
    fx, fy, u0, v0 = cam[0, 0], cam[1, 1], cam[0, 2], cam[1, 2]
    K = np.array([[fx, 0, u0, 0],
                  [0, fy, v0, 0],
                  [0, 0, 1, 0],
                  [0, 0, 0, 1]]).astype(np.float32)
    K[0, :] /= raw_width
    K[1, :] /= raw_height
    K[0, :] *= width // (2 ** scale)
    K[1, :] *= height // (2 ** scale)
    return K, np.linalg.pinv(K)


def test_intrinsics_are_per_sample_and_per_level():
    from ppeadepth.input_pipeline import CityscapesEvalPipeline, CityscapesInputPipeline
    H, W = 16, 20                                                  # level 3: 20 // 8 = 2, not 2.5
    c = training_case()
    out = CityscapesInputPipeline("cpu", H, W, c["raw_hw"], is_train=False)(c["triplets"], c["cameras"])
    e = eval_case((42, 64))
    out_e = CityscapesEvalPipeline("cpu", H, W, (42, 64))(e["raw"], torch.from_numpy(e["cameras"]))
    seen = set()
    for got, cams, raw_w, raw_h in ((out, c["cameras"], 52, 40), (out_e, e["cameras"], 64, 42 * 0.75)):
        for s in range(SCALES):
            assert got[("K", s)].dtype == torch.float32 and tuple(got[("K", s)].shape) == (3, 4, 4)
            for b in range(3):
                K, inv_K = _loader_K(cams[b], raw_w, raw_h, W, H, s)
                assert (got[("K", s)][b].numpy() == K).all() and (got[("inv_K", s)][b].numpy() == inv_K).all()
                seen.add(K.tobytes())
    assert len(seen) == 2 * SCALES * 3                             # three distinct cameras, four distinct levels, twice
    fy = np.float32(np.float32(e["cameras"][0, 1, 1]) / np.float32(31.5)) * np.float32(16)
    assert out_e[("K", 0)][0, 1, 1].item() == float(fy) != float(np.float32(e["cameras"][0, 1, 1]) / np.float32(31) * np.float32(16))
    assert 42 * 3 // 4 == 31                                       # the crop height is not the divisor


def test_camera_file_readers(tmp_path):
    from ppeadepth import input_pipeline as ip
    txt, js = tmp_path / "ulm_000064_000012_cam.txt", tmp_path / "aachen_000000_000019_camera.json"
    txt.write_text("1131.3125,0.0,523.4375,0.0,1130.03125,191.265625,0.0,0.0,1.0\n")
    js.write_text(json.dumps({"extrinsic": {"baseline": 0.209313, "pitch": 0.038, "roll": 0.0, "x": 1.7, "y": 0.1, "yaw": -0.0195,
                                            "z": 1.22},
                              "intrinsic": {"fx": 2262.52, "fy": 2265.3017905988554, "u0": 1096.98, "v0": 513.137}}))
    a, b = ip.read_cityscapes_cam_txt(str(txt)), ip.read_cityscapes_camera_json(str(js))
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape == (3, 3)
    assert (a == np.array([[1131.3125, 0, 523.4375], [0, 1130.03125, 191.265625], [0, 0, 1]])).all()
    assert (b == np.array([[2262.52, 0, 1096.98], [0, 2265.3017905988554, 513.137], [0, 0, 1]])).all()
    # what the readers return is what the pipelines take
    kk = ip.cityscapes_intrinsics(np.stack([a]), 1024, 384, 512, 192, SCALES)
    assert (kk[2, 0, 0] == _loader_K(a, 1024, 384, 512, 192, 2)[0]).all()


CS = ("cityscapes_preprocessed", "cityscapes_preprocessed", "cityscapes", 192, 512)
ARGS = ["--adapter", "--weights_init", "scratch", "--batch_size", "1"]


def _five(opt):
    return opt.dataset, opt.split, opt.eval_split, opt.height, opt.width


def test_train_cs_flag_is_honoured():
    from ppeadepth import options
    from ppeadepth.trainer import Trainer
    opt = options.MonodepthOptions().parse(ARGS + ["--train_cs"])
    assert opt.train_cs and (opt.height, opt.width) == (192, 640)
    early = options.apply_train_cs(options.MonodepthOptions().parse(ARGS + ["--train_cs"]))
    assert _five(early) == CS
    once = dict(vars(early))
    assert options.apply_train_cs(early) is early and vars(early) == once          # idempotent
    plain = options.MonodepthOptions().parse(ARGS)
    before = dict(vars(plain))
    assert vars(options.apply_train_cs(plain)) == before and not hasattr(plain, "dataset")
    tr = Trainer(opt, torch.nn.Identity(), "cpu")
    assert _five(tr.opt) == CS and vars(tr.opt) == once
    for module in (tr.backproject_depth[0], tr.project_3d[0]):
        assert (module.height, module.width) == (192, 512)
    # the reference's order (trainer.py:90-103): with both flags DDAD wins
    both = Trainer(options.MonodepthOptions().parse(ARGS + ["--train_cs", "--ddad", "--frame_ids", "0", "-1"]),
                   torch.nn.Identity(), "cpu")
    assert _five(both.opt) == ("ddad", "ddad", "ddad", 384, 640)
    assert (both.backproject_depth[0].height, both.backproject_depth[0].width) == (384, 640)


def test_view_pass_abi():
    from ppeadepth import _abi
    assert _abi.lib.ppea_abi_version() == _abi.ABI_VERSION >= 24         # 24: the version this entry point arrived with
    header = open(os.path.join(ROOT, "include", "ppea_depth.h")).read()
    decl = re.search(r"^int\s+ppea_lanczos_h_view_u8\s*\(([^)]*)\)", header, flags=re.M | re.S)
    assert decl, "ppea_lanczos_h_view_u8 is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    sig = _abi.SIGNATURES["ppea_lanczos_h_view_u8"]
    assert len(params) == len(sig) == 17 and hasattr(_abi.lib, "ppea_lanczos_h_view_u8")
    import ctypes
    for p, t in zip(params, sig):                                 # pointers, ints and longs in the header's order
        want = ctypes.c_void_p if "*" in p else (ctypes.c_long if p.startswith("long ") else ctypes.c_int)
        assert t is want, p


def test_view_pass_refuses_the_cpu():
    from ppeadepth import _abi, ops
    from ppeadepth import input_pipeline as ip
    with pytest.raises(ValueError):
        ip.CityscapesInputPipeline("cpu", backend="hip")
    with pytest.raises(ValueError):
        ip.CityscapesEvalPipeline("cpu", backend="hip")
    assert ip.CityscapesInputPipeline("cpu", 16, 24, (40, 52)).backend == "torch"
    img = torch.zeros(2, 8, 16, 3, dtype=torch.uint8)
    taps = torch.from_numpy(ip.compact_taps(ip.lanczos_matrix(16, 8)))
    with pytest.raises(_abi.PpeaKernelError):
        ops.lanczos_resize_view_u8(img, (8, 8), taps)             # CPU tensors: no fallback
    with pytest.raises(_abi.PpeaKernelError):
        ops.lanczos_resize_view_u8(img, (8, 8), None)             # a view is read by the horizontal pass
