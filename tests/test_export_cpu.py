"""Host side of the prediction export (no GPU): the ABI of its entry points, `vis.colorize` against matplotlib byte for byte,
the numpy statement of `disp_export` (what a device="cpu" predictor runs) against the float64 restatement, and the writers."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import export_oracle as eo

NEW_SYMBOLS = {"ppea_disp_export_f32": 13, "ppea_disp_export_u16": 13, "ppea_plane_range_f32": 6, "ppea_colorize_u8": 11}
CMAPS = ("plasma", "magma", "viridis", "inferno")


def test_export_abi():
    from ppeadepth import _abi
    assert _abi.lib.ppea_abi_version() == _abi.ABI_VERSION >= 29         # 29: the version these entry points arrived with
    header = open(os.path.join(ROOT, "include", "ppea_depth.h")).read()
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^(?:int|long)\s+(ppea_\w+)\s*\(([^;]*)\)\s*;", header, flags=re.M)}
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared, name
        assert len(declared[name].split(",")) == nargs, name
        assert len(_abi.SIGNATURES[name]) == nargs and hasattr(_abi.lib, name), name
    src = open(os.path.join(ROOT, "ppea-depth_amd", "csrc", "Makefile")).read()
    assert "depth_export.hip" in src


def test_ops_refuse_host_tensors():
    from ppeadepth import _abi, ops, vis
    x = torch.rand(1, 4, 6)
    with pytest.raises(_abi.PpeaKernelError):
        ops.disp_export(x, (8, 12))
    with pytest.raises(_abi.PpeaKernelError):
        ops.plane_range(x)
    with pytest.raises(_abi.PpeaKernelError):
        ops.colorize(x, (8, 12), torch.zeros(1, 2), torch.from_numpy(vis.lut("plasma").copy()))


def _planes():
    """Values below vmin, above vmax, exactly vmin and vmax, nextafter(1, 0), NaN, both infinities, for the range (0, 1)."""
    rng = np.random.default_rng(7)
    x = rng.normal(0.5, 0.5, (31, 45)).astype(np.float32)
    assert (x < 0).any() and (x > 1).any()
    x[0, :8] = [0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.nan, np.inf, -np.inf, -0.0,
                np.nextafter(np.float32(0), np.float32(-1))]
    return x


def _by_the_rule(value, vmin, vmax, name):
    """The reference's rule through matplotlib itself."""
    import matplotlib
    vmin = value.min() if vmin is None else vmin
    vmax = value.max() if vmax is None else vmax
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = (value - vmin) / (vmax - vmin) if vmin != vmax else value * 0.
    return matplotlib.colormaps[name](x, bytes=True)[..., :3]


@pytest.mark.parametrize("name", CMAPS)
def test_colorize_is_matplotlib_byte_for_byte(name):
    matplotlib = pytest.importorskip("matplotlib")
    from ppeadepth import vis
    table = vis.lut(name)
    assert table.dtype == np.uint8 and table.shape == (256, 3)
    assert np.array_equal(table, (np.asarray(matplotlib.colormaps[name].colors) * 255).astype(np.uint8))
    # every row is reachable and is matplotlib's
    centres = ((np.arange(256) + 0.5) / 256).astype(np.float32)[None]
    assert np.array_equal(vis.colorize(centres, 0, 1, name)[0], table)
    x = _planes()
    for value, vmin, vmax in ((x, 0, 1), (x, 0.2, 0.9), (x * 700 + 10, 10, 1000), (x.astype(np.float64), 0, 1),
                              (x, np.float32(0.25), np.float32(0.75))):
        got = vis.colorize(value, vmin, vmax, name)
        assert got.dtype == np.uint8 and got.shape == value.shape + (3,)
        assert np.array_equal(got, _by_the_rule(value, vmin, vmax, name)), (vmin, vmax)
    # exactly vmin and exactly vmax of another range
    edge = np.array([[0.2, 0.9, 0.19999999, 0.90000004]], dtype=np.float32)
    assert np.array_equal(vis.colorize(edge, np.float32(0.2), np.float32(0.9), name),
                          _by_the_rule(edge, np.float32(0.2), np.float32(0.9), name))
    assert (vis.colorize(np.array([[np.nan]], np.float32), 0, 1, name) == 0).all()
    # vmin / vmax None: the value's own minimum and maximum
    clean = np.where(np.isfinite(x), x, np.float32(0.5))
    for vmin, vmax in ((None, None), (None, 2.0), (-1.0, None)):
        assert np.array_equal(vis.colorize(clean, vmin, vmax, name), _by_the_rule(clean, vmin, vmax, name))
    assert np.array_equal(vis.colorize(clean, None, None, name)[clean == clean.max()][0], table[255])
    # a constant plane: value * 0 -> row 0; with a NaN in it the NaN rules the minimum, and everything is bad
    const = np.full((5, 7), 3.25, np.float32)
    assert (vis.colorize(const, None, None, name) == table[0]).all()
    assert np.array_equal(vis.colorize(const, None, None, name), _by_the_rule(const, None, None, name))
    assert (vis.colorize(const, 3.25, 3.25, name) == table[0]).all()
    const[2, 3] = np.nan
    assert np.array_equal(vis.colorize(const, None, None, name), _by_the_rule(const, None, None, name))
    got = vis.colorize(const, 3.25, 3.25, name)
    assert (got[2, 3] == 0).all() and (np.delete(got.reshape(-1, 3), 2 * 7 + 3, 0) == table[0]).all()


def test_shipped_tables_are_what_the_generator_writes():
    pytest.importorskip("matplotlib")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_colormaps", os.path.join(ROOT, "tools", "gen_colormaps.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from ppeadepth import vis
    made = gen.tables()
    assert tuple(made) == CMAPS == vis.CMAPS
    for name in CMAPS:
        assert np.array_equal(made[name], vis.lut(name))
    with pytest.raises(ValueError):
        vis.lut("jet")


@pytest.mark.parametrize("mode", ["disp", "depth"])
@pytest.mark.parametrize("size", eo.RAGGED + [(1, 1)])
def test_host_export_against_float64(size, mode):
    from ppeadepth import evaluate
    disp = eo.scene(3, *eo.SRC)
    for scale, lo, hi in ((0.5, 1e-3, 80.0), (5.4, 0.0, 80.0), (0.05, 1.0, 80.0)):
        want = eo.depth_f64(disp, size, scale, lo, hi, mode)
        got = evaluate.export_depth(disp, size, scale, lo, hi, mode)
        assert got.dtype == np.float32 and got.shape == tuple(size)
        assert eo.rel(got, want) <= eo.RTOL, (scale, eo.rel(got, want))
        if size != (1, 1):          # the three ranges put part of the image on neither clamp, on hi, on lo
            on_hi, on_lo = float((want == hi).mean()), float((want == np.float64(np.float32(lo))).mean())
            assert (on_hi > 0.02) == (scale == 5.4) and (on_lo > 0.02) == (scale == 0.05), (scale, on_hi, on_lo)
        q = evaluate.export_depth(disp, size, scale, lo, hi, mode, dtype=np.uint16)
        assert q.dtype == np.uint16 and np.array_equal(q, (got * np.float32(256)).astype(np.int64))
    with pytest.raises(ValueError):
        evaluate.export_depth(disp, size, 1.0, 0.0, 256.0, mode, dtype=np.uint16)


def test_cpu_colorize_device_takes_the_numpy_path():
    """Statistics on the source plane, resize as evaluate.resize_linear, then vis.colorize; dense and ragged returns."""
    from ppeadepth import evaluate, vis
    planes = np.stack([eo.scene(s, *eo.SRC) for s in (1, 2, 3)])
    flat, table = vis.colorize_device(torch.from_numpy(planes), eo.RAGGED, percentile=95.0)
    assert flat.dtype == torch.uint8 and tuple(flat.shape) == (sum(h * w for h, w in eo.RAGGED), 3)
    assert table.tolist() == [[0, 47, 157], [47 * 157, 24, 80], [47 * 157 + 24 * 80, 12, 41]]
    for b, (o, h, w) in enumerate(table.tolist()):
        p = planes[b]
        hi = np.percentile(p.astype(np.float64), 95.0).astype(np.float32)
        src = p if (h, w) == p.shape else evaluate.resize_linear(p, w, h)
        assert np.array_equal(flat[o:o + h * w].numpy().reshape(h, w, 3), vis.colorize(src, p.min(), hi))
    dense = vis.colorize_device(torch.from_numpy(planes), None, vmin=0.01, vmax=0.1, cmap="magma")
    assert tuple(dense.shape) == (3, 24, 80, 3)
    assert np.array_equal(dense[1].numpy(), vis.colorize(planes[1], np.float32(0.01), np.float32(0.1), "magma"))


def test_writers_round_trip(tmp_path):
    from PIL import Image
    from ppeadepth import evaluate, predict, vis
    disp = eo.scene(5, *eo.SRC)
    depth16 = evaluate.export_depth(disp, (47, 157), 5.4, 0.0, 80.0, dtype=np.uint16)
    assert depth16.max() > 255                              # more than 8 bits are in use
    path = str(tmp_path / "d.png")
    predict.save_png(path, depth16)
    with Image.open(path) as im:
        assert im.mode == "I;16" and im.size == (157, 47)
        back = np.array(im)
    assert back.dtype == np.uint16 and np.array_equal(back, depth16)
    rgb = vis.colorize(disp, None, None)
    path = str(tmp_path / "c.png")
    predict.save_png(path, rgb)
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (80, 24)
        assert np.array_equal(np.array(im), rgb)
