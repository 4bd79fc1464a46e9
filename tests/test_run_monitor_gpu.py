"""The run monitor kernels (csrc/run_monitor.hip) through ops.run_monitor / runlog.RunLog against float64 numpy.

Sizes: 0, one element, below / at / above a wave, several blocks with a ragged tail; each with the buffer at element offset 0
and at offset 1 of a larger allocation (4-byte aligned only: the scalar head).  Values: normal(0,1) times magnitudes spread
over 1e-20 .. 1e18 with denormals mixed in (at the large sizes the sum of squares overflows fp32, never fp64), and the same
with NaN, +Inf and -Inf planted at element 0, at the last element and on both sides of a 16-byte and of a block boundary.

Bounds: grad_l2 within 2^-21 relative of the float64 value -- the fp64 accumulation error is negligible at these n, one
rounding to fp32 plus one square root is < 1 ulp, 4 ulp of fp32 is the margin; grad_max_abs, the non-finite count and the
scalars' bits exact; two calls on the same input give the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L2_RTOL = 2.0 ** -21
SIZES = [0, 1, 3, 63, 64, 65, 1023, 4097, 2 ** 20 + 5]
BLOCK = 256 * 4                                  # elements one block reads per grid-stride turn


def _values(n, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 10.0 ** g.uniform(-20, 18, n)).astype(np.float32)
    x[5::7] = (g.integers(1, 1000, len(x[5::7])) * 1e-42).astype(np.float32)        # denormals
    return x


def _planted(x, offset):
    """NaN / +Inf / -Inf at element 0, at the last one, on both sides of the first 16-byte boundaries and of the first block
    boundary of the aligned body (which starts `head` elements in)."""
    n, head = len(x), (4 - offset) % 4
    at = [0, n - 1, head - 1, head, head + 3, head + 4, head + BLOCK - 1, head + BLOCK, 3, 4]
    bad = x.copy()
    for k, j in enumerate(sorted({j for j in at if 0 <= j < n})):
        bad[j] = (np.nan, np.inf, -np.inf)[k % 3]
    return bad


def _reference(x):
    x = x.astype(np.float64)
    ok = np.isfinite(x)
    l2 = float(np.sqrt(np.sum(x[ok] ** 2)))
    assert np.isfinite(l2)                                   # the float64 reference itself is finite for these seeds
    return l2, np.float32(np.abs(x[ok]).max() if ok.any() else 0.0), int((~ok).sum())


def _on_device(x, offset, device):
    big = torch.zeros(len(x) + 8, device=device)
    assert big.data_ptr() % 16 == 0
    buf = big[offset:offset + len(x)]
    buf.copy_(torch.from_numpy(x))
    assert buf.is_contiguous() and (len(x) == 0 or buf.data_ptr() % 16 == 4 * offset)
    return buf


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_gradient_columns_match_float64(device, n, offset):
    from ppeadepth.runlog import RunLog
    x = _values(n, seed=100 + n)
    cases = [x, _planted(x, offset)]
    log = RunLog(device, capacity=8, names=("loss",))
    for k, v in enumerate(cases):
        buf = _on_device(v, offset, device)
        log.append(k, {}, buf)
        log.append(k, {}, buf)                                # the same input again: the same bits
    rows = log.read()
    assert len(rows) == 4 and rows.dropped == 0
    for k, v in enumerate(cases):
        l2, mx, cnt = _reference(v)
        a, b = rows[2 * k], rows[2 * k + 1]
        print(f"n={n} offset={offset} case={k}: l2 {a['grad_l2']!r} vs {l2!r} rel {abs(float(a['grad_l2']) - l2) / max(l2, 1e-300):.3e}; "
              f"max {a['grad_max_abs']!r} vs {mx!r}; nonfinite {a['grad_nonfinite']} vs {cnt}")
        assert abs(float(a["grad_l2"]) - l2) <= L2_RTOL * l2
        assert a["grad_max_abs"].tobytes() == mx.tobytes()
        assert a["grad_nonfinite"] == cnt
        assert a["step"] == b["step"] == k and a["loss"] is None
        assert all(a[c].tobytes() == b[c].tobytes() for c in ("grad_l2", "grad_max_abs")) and a["grad_nonfinite"] == b["grad_nonfinite"]
    assert rows.first_bad_step == (1 if n > 0 else -1)


def test_n_limits_the_scan_and_grad_scale_multiplies(device):
    from ppeadepth.runlog import RunLog
    x = _values(5000, seed=7)
    buf = _on_device(x, 1, device)
    log = RunLog(device, capacity=4, names=())
    log.append(0, {}, buf, n=4097, grad_scale=0.125)
    log.append(1, {}, None)
    log.append(2, {}, buf, n=0)
    rows = log.read()
    l2, mx, _ = _reference(x[:4097])
    assert abs(float(rows[0]["grad_l2"]) - 0.125 * l2) <= L2_RTOL * 0.125 * l2
    assert rows[0]["grad_max_abs"].tobytes() == np.float32(0.125 * mx).tobytes()
    assert all(r["grad_l2"] == 0 and r["grad_max_abs"] == 0 and r["grad_nonfinite"] == 0 for r in rows[1:])


def test_scalars_are_copied_bit_for_bit_and_absent_ones_are_absent(device):
    from ppeadepth.runlog import RunLog
    names = tuple("abcdefgh")
    bits = [0x7fc01234, 0xff800000, 0x00000001, 0x80000000, 0x3f800000, 0x7f7fffff, 0xffc00000, 0x12345678]
    src = torch.tensor(np.array(bits, dtype=np.uint32).view(np.int32), device=device).view(torch.float32)
    log = RunLog(device, capacity=4, names=names)
    log.append(5, {k: src[i] for i, k in enumerate(names)})                    # 0-dim views at 4-byte offsets
    log.append(6, {"c": src[2:3], "h": src[7].clone()})                        # one-element and 0-dim; the rest absent
    rows = log.read()
    assert [int(rows[0][k].view(np.uint32)) for k in names] == bits
    assert int(rows[1]["c"].view(np.uint32)) == bits[2] and int(rows[1]["h"].view(np.uint32)) == bits[7]
    assert all(rows[1][k] is None for k in "abdefg")                            # absent, not 0
    assert rows.first_bad_step == 5 and [r["step"] for r in rows] == [5, 6]


def test_ring_wraps_on_the_device_and_first_bad_step_is_sticky(device):
    from ppeadepth.runlog import RunLog
    log = RunLog(device, capacity=4, names=("loss", "lr"))
    one, inf = torch.ones((), device=device), torch.full((), float("inf"), device=device)
    g = torch.ones(100, device=device)
    for s in range(3):
        log.append(s, {"loss": one}, g)
    first = log.read()
    assert [r["step"] for r in first] == [0, 1, 2] and first.dropped == 0 and first.first_bad_step == -1
    assert all(r["lr"] is None and r["grad_l2"] == np.float32(10.0) for r in first)
    for s in range(3, 9):
        log.append(s, {"loss": inf if s == 4 else one, "lr": one}, g)
    second = log.read()
    assert [r["step"] for r in second] == [5, 6, 7, 8] and second.dropped == 2
    assert second.first_bad_step == 4                                           # later good rows do not clear it
    log.append(9, {"loss": inf})
    third = log.read()
    assert [r["step"] for r in third] == [9] and third.first_bad_step == 4 and third.dropped == 0   # ... nor later reads
    assert len(log.read()) == 0


def test_refusals(device):
    from ppeadepth._abi import PpeaKernelError
    from ppeadepth.runlog import RunLog
    log = RunLog(device, capacity=2, names=tuple("abcdefgh"))
    g = torch.zeros(64, device=device)
    with pytest.raises(PpeaKernelError):
        log.append(0, {}, g.to(torch.bfloat16))
    with pytest.raises(PpeaKernelError):
        log.append(0, {}, g[::2])
    with pytest.raises(PpeaKernelError):
        log.append(0, {"a": torch.zeros(())}, g)                               # a host scalar with a device buffer
    with pytest.raises(PpeaKernelError):
        log.append(0, {"a": torch.zeros((), device=device)}, g.cpu())
    with pytest.raises(PpeaKernelError):
        log.append(0, {k: torch.zeros((), device=device) for k in "abcdefghi"}, g)
    with pytest.raises(PpeaKernelError):
        RunLog(device, names=tuple("abcdefghi"))
    assert len(log.read()) == 0
