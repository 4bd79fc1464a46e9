"""Checkpoints on the GPU: the one-launch pack / unpack of scattered state (csrc/state_pack.hip through ops.pack_segments /
unpack_segments) against `torch.cat` of byte views, and the property the feature exists for -- a run that is stopped and
resumed from `TrainEngine.checkpoint_state()` equals the uninterrupted run BIT FOR BIT (the step is a bitwise pure function
of state, inputs and seeds), eager and under hipGraph replay, with the restore done in place after `capture()`.

Shapes: the whole-step tests run the 31B model at B = 2, 64 x 96 (the e2e_small shape) for four steps, like the existing
step tests; everything is compared with torch.equal -- there is no tolerance in this file."""
import random

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu


# ---- pack / unpack ----------------------------------------------------------------------------------------------------
GUARD = 64


def _segment(device, nbytes, dtype, shift, seed):
    """A tensor of `nbytes` bytes of `dtype` whose first byte sits `shift` bytes past a 16-byte boundary, as a view (with a
    storage offset) into a larger uint8 backing filled with random bytes; -> (tensor, backing, start)."""
    g = torch.Generator().manual_seed(seed)
    backing = torch.randint(0, 256, (GUARD + shift + nbytes + GUARD,), dtype=torch.uint8, generator=g).to(device)
    assert backing.data_ptr() % 16 == 0
    start = GUARD + shift
    t = backing[start:start + nbytes].view(dtype)
    assert (nbytes == 0 or t.data_ptr() % 16 == shift % 16) and t.numel() * t.element_size() == nbytes
    return t, backing, start


def _cases(unit):
    u8, bf, f32, i64 = torch.uint8, torch.bfloat16, torch.float32, torch.int64
    return {
        # every small size, then the same kinds of size behind every source alignment and dtype, all in ONE call
        "mixed": [(n, u8, 0) for n in (0, 1, 2, 8, 12, 15, 16, 17, 4 * 128 + 4)] +
                 [(8, i64, 8), (12, bf, 2), (4 * 128 + 4, f32, 4), (16, f32, 12), (17, u8, 1), (15, u8, 3), (32, i64, 8),
                  (4 * 128 + 4, bf, 2), (2, bf, 14), (0, f32, 4), (12, f32, 8), (4 * 128 + 4, u8, 12), (17, u8, 15)],
        # exactly one work unit of the byte split, one byte more, three units minus one; aligned and not
        "units": [(unit, u8, 0), (unit + 1, u8, 0), (3 * unit - 1, u8, 0), (unit, f32, 4), (unit + 1, u8, 2),
                  (3 * unit - 1, u8, 8), (3 * unit - 2, bf, 2), (2 * unit, i64, 8)],
        "one": [(17, u8, 0)],
        "one_unaligned_scalar": [(8, i64, 8)],
        "many": [(8, i64, 8 * (i % 2)) for i in range(2000)],
    }


@pytest.mark.parametrize("case", ["mixed", "units", "one", "one_unaligned_scalar", "many"])
def test_pack_unpack_segments_are_byte_exact_and_stay_in_bounds(device, case):
    from ppeadepth import _abi, ops
    unit = int(_abi.lib.ppea_pack_unit_bytes())
    assert unit % 16 == 0
    made = [_segment(device, n, dt, shift, seed=i) for i, (n, dt, shift) in enumerate(_cases(unit)[case])]
    srcs = [m[0] for m in made]
    src_backings = [m[1].clone() for m in made]
    layout = ops.SegmentLayout(srcs)
    assert all(o % 16 == 0 for o in layout.offsets) and layout.units == sum(-(-n // unit) for n in layout.nbytes)
    # pack into a buffer that is larger than needed, pre-filled: padding and guard bytes must come back unchanged
    out = torch.full((GUARD + max(layout.total, 16) + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    want = out.clone()
    for t, o, n in zip(srcs, layout.offsets, layout.nbytes):
        want[GUARD + o:GUARD + o + n] = t.reshape(-1).view(torch.uint8)
    packed = out[GUARD:]
    got, layout2 = ops.pack_segments(srcs, out=packed, layout=layout)
    torch.cuda.synchronize()
    assert layout2 is layout and got.data_ptr() == packed.data_ptr()
    assert torch.equal(out, want)
    assert all(torch.equal(m[1], b) for m, b in zip(made, src_backings))          # sources untouched
    # the same bytes as torch.cat of the byte views, each padded to 16
    cat = torch.cat([torch.cat([t.reshape(-1).view(torch.uint8),
                                torch.full(((-n) % 16,), 0xA5, dtype=torch.uint8, device=device)])
                     for t, n in zip(srcs, layout.nbytes)])
    assert torch.equal(packed[:layout.total], cat)
    # without `out`: a fresh zero-filled buffer
    fresh, _ = ops.pack_segments(srcs)
    for v, t in zip(layout.views(fresh), srcs):
        assert v.dtype == t.dtype and v.shape == t.shape and torch.equal(v.reshape(-1).view(torch.uint8), t.reshape(-1).view(torch.uint8))
    # unpack into other destinations with the same alignments, inside larger pre-filled backings
    dst = [_segment(device, n, dt, shift, seed=1000 + i) for i, (n, dt, shift) in enumerate(_cases(unit)[case])]
    want_backings = []
    for (t, backing, start), s in zip(dst, srcs):
        w = backing.clone()
        w[start:start + s.numel() * s.element_size()] = s.reshape(-1).view(torch.uint8)
        want_backings.append(w)
    ops.unpack_segments(packed, layout, [d[0] for d in dst])
    torch.cuda.synchronize()
    for (t, backing, _), w, s in zip(dst, want_backings, srcs):
        assert torch.equal(backing, w)                                            # guards on both sides unchanged
        assert torch.equal(t.reshape(-1).view(torch.uint8), s.reshape(-1).view(torch.uint8))  # unpack(pack(x)) == x
    assert torch.equal(out, want)                                                 # unpack does not write the packed buffer


def test_pack_segments_refuses_host_tensors(device):
    from ppeadepth import _abi, ops
    with pytest.raises(_abi.PpeaKernelError):
        ops.pack_segments([torch.zeros(4)])
    buf, layout = ops.pack_segments([torch.zeros(4, device=device)])
    with pytest.raises(_abi.PpeaKernelError):
        ops.unpack_segments(buf, layout, [torch.zeros(4)])
    with pytest.raises(_abi.PpeaKernelError):
        ops.unpack_segments(buf.cpu(), layout, [torch.zeros(4, device=device)])


# ---- resume -------------------------------------------------------------------------------------------------------------
B, H, W, STEPS, KEEP = 2, 64, 96, 4, 2


def _build(device, bf16, conditioned=True):
    from ppeadepth import networks, options
    from ppeadepth.dist import TrainEngine
    from ppeadepth.trainer import Trainer
    opt = options.default_options(height=H, width=W, batch_size=B, use_checkpoint=True)
    model = networks.RepDepth(opt)
    synth.fill_state_dict(model, conditioned=conditioned)
    model.to(device).train()
    tr = Trainer(opt, model, device, amp_dtype=torch.bfloat16 if bf16 else None)
    return model, tr, TrainEngine(tr, lr=1e-4, bf16_params=bf16)


@pytest.fixture(scope="module")
def batches(device):
    return [{k: v.to(device) for k, v in synth.make_rendered_inputs(B, H, W, seed=50 + i).items()} for i in range(STEPS)]


def _same(a, b, what):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what
    elif isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)) and any(torch.is_tensor(x) or isinstance(x, (dict, list, tuple)) for x in a):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert a == b, what


def _engine_state(eng):
    """Everything a resumed run must reproduce: the three documents (model with the fp32 masters and the BatchNorm
    statistics, moments and step by index, tracker, schedule, step, the random streams) and the engine-only tensors."""
    docs = eng.checkpoint_state()
    extra = {"W16": eng.W16.detach().cpu().clone(), "adam_state": eng.adam_state.detach().cpu().clone(),
             "tracker": torch.stack([eng.trainer.depth_bin_tracker.min_depth, eng.trainer.depth_bin_tracker.max_depth]).cpu(),
             "bins_updated": eng.trainer.depth_bin_tracker.updated, "step": eng.trainer.step}
    return {"model": docs.model, "track": docs.track, "adam": docs.adam, "engine": extra}


def _run(eng, batches, first, last, keep_after=None):
    kept, losses = None, []
    for i in range(first, last):
        _, out = eng.step(dict(batches[i]) if eng.graph is None else batches[i])
        torch.cuda.synchronize()
        losses.append({k: v.detach().cpu().clone() for k, v in out.items() if torch.is_tensor(v)})
        if keep_after is not None and i + 1 == keep_after:
            kept = eng.checkpoint_state()
    return kept, losses


@pytest.mark.parametrize("mode", ["reference", "device"])
@pytest.mark.parametrize("bf16", [False, True])
def test_resumed_eager_run_equals_the_uninterrupted_run_bit_for_bit(device, batches, bf16, mode):
    from ppeadepth import rng
    try:
        rng.set_mode(mode)
        model, tr, eng = _build(device, bf16)
        random.seed(7)
        torch.manual_seed(7)
        kept, losses_a = _run(eng, batches, 0, STEPS, keep_after=KEEP)
        final_a = _engine_state(eng)
        assert kept.track["ppea"]["step"] == KEEP and float(kept.adam["state"][0]["step"]) == KEEP
        del model, tr, eng
        # a fresh model with OTHER weights (frozen ones included), other seeds, the other rng mode: all of it is loaded
        rng.set_mode("device" if mode == "reference" else "reference")
        model, tr, eng = _build(device, bf16, conditioned=False)
        random.seed(99)
        torch.manual_seed(99)
        keys = eng.load_checkpoint_state(kept)
        assert not keys.missing_keys and not keys.unexpected_keys and rng.get_mode() == mode and tr.step == KEEP
        _, losses_b = _run(eng, batches, KEEP, STEPS)
        _same(losses_a[KEEP:], losses_b, "losses")
        _same(final_a, _engine_state(eng), "state")
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")


@pytest.mark.parametrize("mode", ["reference", "device"])
def test_resume_in_place_after_capture_equals_the_uninterrupted_replays_bit_for_bit(device, batches, mode):
    """bf16, the benchmarked launch mode.  B captures FIRST (its warm-up step moves every piece of state and consumes random
    numbers), then loads in place, then replays: the graph's addresses stay valid and the restored generator states are the
    ones the replays read."""
    from ppeadepth import rng
    try:
        rng.set_mode(mode)
        model, tr, eng = _build(device, True)
        eng.capture(batches[0], warmup=1, restore_state=True)
        random.seed(7)
        torch.manual_seed(7)
        kept, losses_a = _run(eng, batches, 0, STEPS, keep_after=KEEP)
        final_a = _engine_state(eng)
        del model, tr, eng
        model, tr, eng = _build(device, True)
        random.seed(99)
        torch.manual_seed(99)
        eng.capture(batches[1], warmup=1, restore_state=True)
        ptrs = (eng.P.data_ptr(), eng.W16.data_ptr(), eng.adam_state.data_ptr(), tr.depth_bin_tracker.min_depth.data_ptr())
        eng.load_checkpoint_state(kept)
        assert ptrs == (eng.P.data_ptr(), eng.W16.data_ptr(), eng.adam_state.data_ptr(),
                        tr.depth_bin_tracker.min_depth.data_ptr())
        _, losses_b = _run(eng, batches, KEEP, STEPS)
        _same(losses_a[KEEP:], losses_b, "losses")
        _same(final_a, _engine_state(eng), "state")
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")


def test_non_blocking_save_is_not_changed_by_later_replays_and_saves_are_serialised(device, batches):
    from ppeadepth import rng
    from ppeadepth.dist import PendingCheckpoint
    try:
        rng.set_mode("device")
        model, tr, eng = _build(device, True)
        eng.capture(batches[0], warmup=1, restore_state=True)
        _run(eng, batches, 0, 1)
        ref = eng.checkpoint_state()
        handle = eng.checkpoint_state(blocking=False)
        assert isinstance(handle, PendingCheckpoint)
        eng.step(batches[1])
        eng.step(batches[2])
        docs = handle.wait()
        _same(tuple(ref), tuple(docs), "non-blocking")
        torch.cuda.synchronize()
        moved = eng.checkpoint_state()
        assert not torch.equal(moved.adam["state"][0]["exp_avg"], ref.adam["state"][0]["exp_avg"])      # the replays ran
        # a second save while one is pending waits for the first: both hold the state of their own boundary
        first = eng.checkpoint_state(blocking=False)
        eng.step(batches[3])
        second = eng.checkpoint_state(blocking=False)
        assert first._done and eng._ckpt_pending is second
        torch.cuda.synchronize()
        after = eng.checkpoint_state()
        assert eng._ckpt_pending is None                                            # a blocking save waits as well
        _same(tuple(moved), tuple(first.wait()), "first")
        _same(tuple(after), tuple(second.wait()), "second")
    finally:
        rng.set_aug_buffer(None)
        rng.set_mode("device")


def test_learning_rate_schedule_survives_a_checkpoint(device):
    model, tr, eng = _build(device, False)
    for _ in range(tr.opt.scheduler_step_size):
        eng.scheduler_step(lr_quirk=False)
    lr = eng.optimizer.param_groups[0]["lr"]
    assert lr == pytest.approx(1e-5) and float(eng.adam_state[1]) == pytest.approx(1e-5)
    docs = eng.checkpoint_state()
    assert docs.track["ppea"]["lr"] == lr == docs.adam["param_groups"][0]["lr"]
    model2, tr2, eng2 = _build(device, False)
    assert eng2.optimizer.param_groups[0]["lr"] == pytest.approx(1e-4)
    eng2.load_checkpoint_state(docs)
    assert eng2.optimizer.param_groups[0]["lr"] == lr
    assert eng2.scheduler.last_epoch == eng.scheduler.last_epoch == tr.opt.scheduler_step_size
    assert float(eng2.adam_state[1]) == float(eng.adam_state[1]) and float(eng2.adam_state[0]) == 0.0
    eng2.scheduler_step(lr_quirk=False)                                    # and the schedule goes on from there
    assert eng2.optimizer.param_groups[0]["lr"] == pytest.approx(1e-5)
