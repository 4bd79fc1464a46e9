"""The run monitor's host path (ops.run_monitor on CPU tensors, runlog.RunLog(device="cpu")) against float64 numpy, the
ring's wrap / `dropped` bookkeeping, the refusals, and `train.NonFiniteRun` out of `Run.check_log` -- on plain tensors: no
model is driven with non-finite values.

Bounds (the same as on the device, tests/test_run_monitor_gpu.py): grad_l2 within 2^-21 relative of the float64 value (one
rounding to fp32 plus one square root is < 1 ulp; 4 ulp is the margin), grad_max_abs, the non-finite count and the scalars'
bits exact."""
import os

import numpy as np
import pytest
import torch

L2_RTOL = 2.0 ** -21


def _values(n, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 10.0 ** g.uniform(-20, 18, n)).astype(np.float32)
    x[5::7] = (g.integers(1, 1000, len(x[5::7])) * 1e-42).astype(np.float32)        # denormals
    return x


def _reference(x, grad_scale=1.0):
    x = x.astype(np.float64)
    ok = np.isfinite(x)
    l2 = float(np.float32(grad_scale)) * float(np.sqrt(np.sum(x[ok] ** 2)))
    mx = np.float32(np.float32(grad_scale) * np.float32(np.abs(x[ok]).max() if ok.any() else 0.0))
    return l2, mx, int((~ok).sum())


@pytest.mark.parametrize("n", [0, 1, 3, 64, 65, 1023])
def test_host_rows_match_float64_numpy(n):
    from ppeadepth.runlog import RunLog
    x = _values(n, seed=n)
    bad = x.copy()
    for j, v in zip([0, n - 1, n // 2], [np.nan, np.inf, -np.inf]):
        if 0 <= j < n:
            bad[j] = v
    log = RunLog("cpu", capacity=4, names=("loss", "lr"))
    nan = torch.tensor([0x7fc01234], dtype=torch.int32).view(torch.float32)
    log.append(10, {"loss": torch.tensor(1.5)}, torch.from_numpy(x))
    log.append(11, {"loss": nan, "lr": torch.tensor([1e-4])}, torch.from_numpy(bad), grad_scale=0.5)
    rows = log.read()
    assert [r["step"] for r in rows] == [10, 11] and rows.dropped == 0
    for r, (v, gs) in zip(rows, [(x, 1.0), (bad, 0.5)]):
        l2, mx, cnt = _reference(v, gs)
        assert np.isfinite(l2)
        assert abs(float(r["grad_l2"]) - l2) <= L2_RTOL * l2
        assert r["grad_max_abs"].tobytes() == mx.tobytes() and r["grad_nonfinite"] == cnt
    assert rows[0]["loss"].tobytes() == np.float32(1.5).tobytes() and rows[0]["lr"] is None
    assert rows[1]["loss"].view(np.uint32) == 0x7fc01234 and rows[1]["lr"].tobytes() == np.float32(1e-4).tobytes()
    assert rows.first_bad_step == 11


def test_ring_wraps_and_counts_dropped_rows():
    from ppeadepth.runlog import RunLog
    log = RunLog("cpu", capacity=4, names=("loss", "lr"))
    for s in range(3):
        log.append(s, {"loss": torch.tensor(float(s))})
    first = log.read()
    assert [r["step"] for r in first] == [0, 1, 2] and first.dropped == 0 and first.first_bad_step == -1
    assert all(r["lr"] is None and r["loss"] == np.float32(r["step"]) for r in first)           # absent, not 0
    assert all(r["grad_l2"] == 0 and r["grad_max_abs"] == 0 and r["grad_nonfinite"] == 0 for r in first)
    for s in range(3, 9):
        log.append(s, {"loss": torch.tensor(float("inf") if s == 4 else 0.0)})
    second = log.read()
    assert [r["step"] for r in second] == [5, 6, 7, 8] and second.dropped == 2
    assert second.first_bad_step == 4                                  # sticky: the bad row itself was overwritten
    assert len(log.read()) == 0
    log.append(9, {"loss": torch.tensor(float("nan"))})
    third = log.read()
    assert [r["step"] for r in third] == [9] and third.dropped == 0 and third.first_bad_step == 4


def test_refusals_on_host_tensors():
    from ppeadepth._abi import PpeaKernelError
    from ppeadepth.runlog import RunLog
    with pytest.raises(PpeaKernelError):
        RunLog("cpu", names=tuple("abcdefghi"))
    log = RunLog("cpu", capacity=2, names=tuple("abcdefgh"))
    g = torch.zeros(16)
    with pytest.raises(PpeaKernelError):
        log.append(0, {}, g.to(torch.bfloat16))
    with pytest.raises(PpeaKernelError):
        log.append(0, {}, g[::2])
    with pytest.raises(PpeaKernelError):
        log.append(0, {"a": torch.zeros((), dtype=torch.float64)})
    with pytest.raises(PpeaKernelError):
        log.append(0, {"a": torch.zeros(2)})
    with pytest.raises(PpeaKernelError):
        log.append(0, {k: torch.zeros(()) for k in "abcdefghi"})
    assert len(log.read()) == 0                                        # a refused call appends nothing


def test_symbol_is_declared_and_bound():
    from ppeadepth import _abi
    assert _abi.lib.ppea_abi_version() == _abi.ABI_VERSION >= 30         # 30: the version this entry point arrived with
    assert "ppea_run_monitor_f32" in _abi.SIGNATURES and _abi.lib.ppea_run_monitor_row_words() == 16
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int ppea_run_monitor_f32(" in open(os.path.join(root, "include", "ppea_depth.h")).read()
    assert "run_monitor.hip" in open(os.path.join(root, "ppea-depth_amd", "csrc", "Makefile")).read()


def test_a_planted_nan_loss_stops_the_run_with_its_step_and_column():
    from ppeadepth import train
    from ppeadepth.runlog import RunLog
    run = train.Run.__new__(train.Run)
    run.log, run.rows, run.out = RunLog("cpu", capacity=8, names=train.LOG_NAMES), [], lambda *a: None
    good = {k: torch.tensor(1.0) for k in train.LOG_NAMES}
    run.log.append(0, good, torch.ones(5))
    assert len(run.check_log()) == 1
    run.log.append(1, dict(good, **{"loss/0": torch.tensor(float("nan"))}), torch.ones(5))
    run.log.append(2, good, torch.ones(5))
    with pytest.raises(train.NonFiniteRun) as e:
        run.check_log()
    assert e.value.step == 1 and e.value.columns == ("loss/0",) and "step 1" in str(e.value)
    run.log.append(3, good, torch.tensor([1.0, float("inf")]))
    with pytest.raises(train.NonFiniteRun) as e:                        # and it stays stopped
        run.check_log()
    assert e.value.step == 1
