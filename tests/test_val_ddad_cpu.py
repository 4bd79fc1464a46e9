"""DDAD validation on the host: `evaluate.evaluate_disps_ddad` against the golden written from the reference's unmodified
`Trainer.val_ddad` (tools/gen_ddad_golden.py), `--ddad` honoured by `Trainer.__init__`, and `DDADInputPipeline(backend=
"torch")` byte for byte against Pillow itself."""
import numpy as np
import pytest
import torch

RTOL = 1e-5              # the bound between two statements of a protocol (tests/test_oracle_golden.py:320)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(d == 0, 0.0, d / np.abs(b))))


@pytest.mark.parametrize("options", ["default", "opts"])
def test_host_protocol_reproduces_the_reference_val_ddad(golden, options):
    from ppeadepth import evaluate
    g = golden("val_ddad")
    gt = g["gt_depth"].numpy()
    ms, sf = bool(g["median_scaling_" + options]), float(g["scale_factor_" + options])
    assert (ms, sf) == {"default": (True, 1.0), "opts": (False, 1.3)}[options]
    student = evaluate.evaluate_disps_ddad(g["pred_disp"].numpy(), gt, ms, sf)
    teacher = evaluate.evaluate_disps_ddad(g["pred_disp_mono"].numpy(), gt, True)      # never takes the two options
    for name, got, want in (("student", student, g["errors_" + options].numpy()),
                            ("teacher", teacher, g["errors_mono_" + options].numpy())):
        print(f"[{options}] {name}: {got}\n    reference {want}  rel {_rel(got, want):.3e}")
        assert got.shape == (7,) and _rel(got, want) <= RTOL
    # not the 80 m range test that the name "ddad" selects in evaluate_image
    range80 = evaluate.evaluate_disps(g["pred_disp"].numpy(), list(gt), "ddad", ms, sf)
    assert (np.abs(student - range80) / np.abs(range80) > 1e-3).all()
    assert (g["errors_mono_default"].numpy() == g["errors_mono_opts"].numpy()).all()


def test_evaluate_image_ddad_returns_the_ratio_and_scores_the_whole_map(golden):
    from ppeadepth import evaluate
    g = golden("val_ddad")
    disp, gt = g["pred_disp"].numpy()[0], g["gt_depth"].numpy()[0]
    errors, ratio = evaluate.evaluate_image_ddad(disp, gt)
    depth = torch.nn.functional.interpolate(1 / torch.from_numpy(disp)[None, None], gt.shape, mode="bilinear")[0, 0].numpy()
    mask = (gt > 1e-3) & (gt < 200)
    assert np.float32(ratio).tobytes() == np.float32(np.median(gt[mask]) / np.median(depth[mask])).tobytes()
    assert len(errors) == 7 and evaluate.evaluate_image_ddad(disp, gt, median_scaling=False)[1] is None
    assert evaluate.region_size("val_ddad", 1216, 1936) == 1216 * 1936
    from ppeadepth import ops
    assert ops.EVAL_MODES["val_ddad"] == 3 and ops.EVAL_MODES.get("ddad", 0) == 0


def test_ddad_flag_is_honoured_by_the_trainer():
    from ppeadepth import options
    from ppeadepth.trainer import Trainer
    opt = options.MonodepthOptions().parse(["--adapter", "--weights_init", "scratch", "--ddad", "--batch_size", "1",
                                            "--frame_ids", "0", "-1"])
    assert opt.ddad and (opt.height, opt.width) == (192, 640)
    tr = Trainer(opt, torch.nn.Identity(), "cpu")
    assert (tr.opt.dataset, tr.opt.split, tr.opt.eval_split, tr.opt.height, tr.opt.width) == ("ddad", "ddad", "ddad", 384, 640)
    for module in (tr.backproject_depth[0], tr.project_3d[0]):
        assert (module.height, module.width) == (384, 640)
    assert hasattr(tr, "val_ddad")
    # the helper a caller applies before building the model gives the same options, and applying it twice changes nothing
    early = options.apply_ddad(options.MonodepthOptions().parse(["--adapter", "--weights_init", "scratch", "--ddad"]))
    assert (early.dataset, early.split, early.eval_split, early.height, early.width) == ("ddad", "ddad", "ddad", 384, 640)
    assert vars(options.apply_ddad(early)) == vars(tr.opt) | {"batch_size": early.batch_size, "frame_ids": early.frame_ids}
    # the host metric refuses a DeviceGroundTruth by name, before it touches the model
    from ppeadepth import evaluate
    with pytest.raises(ValueError, match="metrics='host'"):
        tr.val_ddad([], evaluate.DeviceGroundTruth([np.ones((2, 3), np.float32)], "cpu"))
    plain = options.MonodepthOptions().parse(["--adapter", "--weights_init", "scratch", "--batch_size", "1"])
    assert not hasattr(Trainer(plain, torch.nn.Identity(), "cpu").opt, "dataset") and plain.height == 192


# ---- the loader's image path ---------------------------------------------------------------------------------------
def _pillow(img, H, W, scales):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0))).resize((W, H), Image.BILINEAR)      # ddad_dataset.py:121
    out = []
    for s in range(scales):                                    # :77, chained; scale 0 resizes to its own size (a copy)
        im = im.resize((W // 2 ** s, H // 2 ** s), Image.LANCZOS)
        out.append(np.asarray(im).transpose(2, 0, 1))
    return out


def _numpy_K(intr, width, height, raw_hw):
    K = np.zeros((4, 4), np.float32)
    K[:3, :3] = intr.copy()
    K[3][3] = 1
    K[0, :] *= width / raw_hw[1]
    K[1, :] *= height / raw_hw[0]
    return K, np.linalg.pinv(K)


@pytest.mark.parametrize("raw_hw,hw,B", [((50, 77), (16, 24), 3), ((1216, 1936), (384, 640), 1)])
def test_ddad_pipeline_is_pillow_byte_for_byte(raw_hw, hw, B):
    from ppeadepth.input_pipeline import DDADInputPipeline
    g = np.random.default_rng(3)
    raw = {f: g.integers(0, 256, (B, 3) + raw_hw, dtype=np.uint8) for f in (0, -1)}
    raw[0][0, :, :, : raw_hw[1] // 2] //= 16                   # a dark half and a saturated corner
    raw[-1][0, :, : raw_hw[0] // 3, : raw_hw[1] // 3] = 255
    intr = (np.array([[2181.0, 0, 928.0], [0, 2181.0, 616.0], [0, 0, 1]]) * g.uniform(0.9, 1.1, (B, 1, 1))).astype(np.float32)
    intr[:, 2, 2] = 1
    pipe = DDADInputPipeline("cpu", hw[0], hw[1], raw_hw, backend="torch")
    out = pipe({f: torch.from_numpy(v) for f, v in raw.items()}, intr)
    assert len(out) == 2 * 2 * 4 + 2 * 4
    for f in (0, -1):
        for b in range(B):
            want = _pillow(raw[f][b], hw[0], hw[1], 4)
            for s in range(4):
                color = out[("color", f, s)][b]
                assert color.dtype == torch.float32 and tuple(color.shape) == (3, hw[0] // 2 ** s, hw[1] // 2 ** s)
                assert torch.equal(color, torch.from_numpy(want[s].copy()).float() / 255)           # ToTensor
                assert torch.equal(out[("color_aug", f, s)][b], color)                             # no jitter, no flip
    for b in range(B):
        K, inv_K = _numpy_K(intr[b], hw[1], hw[0], raw_hw)
        for s in range(4):                                     # the same matrix at every scale
            assert out[("K", s)][b].numpy().tobytes() == K.tobytes()
            assert out[("inv_K", s)][b].numpy().tobytes() == inv_K.tobytes()


def test_resample_matrix_keeps_lanczos_and_adds_the_triangle():
    from ppeadepth import input_pipeline as ip
    assert (ip.resample_matrix(77, 24, "lanczos") == ip.lanczos_matrix(77, 24)).all()
    m = ip.resample_matrix(1936, 640, "bilinear")
    assert m.shape == (640, 1936) and (m.sum(1) > 0).all() and (m >= 0).all()
    assert int((m != 0).sum(1).max()) <= 2 * int(np.ceil(1936 / 640)) + 1          # support 1 x scale on either side
    assert abs(m.sum(1) / (1 << ip.PRECISION_BITS) - 1).max() < 1e-5
    with pytest.raises(ValueError):
        ip.resample_matrix(10, 5, "bicubic")
    with pytest.raises(ValueError):
        ip.DDADInputPipeline("cpu", backend="hip")
