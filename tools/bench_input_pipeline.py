"""Where the time of one `DeviceInputPipeline` call goes (B = 12 triplets, 375x1242 -> 192x640, as `bench.py --input_pipeline`).

    python tools/bench_input_pipeline.py [--reps 20] [--backend hip|torch] [--out FILE]
    python tools/bench_input_pipeline.py --ragged [--reps 20] [--out FILE]

Per call: the wall time with the parameters drawn inside the call (what bench.py times), the wall time with pre-drawn
parameters, the host-side draws alone (144 `randperm` / `uniform_` groups; no device work), the device time of every kernel
from the profiler, and the algorithmic HBM traffic computed from the shapes (raw uint8 frames read once, `color` and
`color_aug` written once in fp32 at every scale) with its streaming floor at 6.3 TB/s.  Prints ONE JSON line.

--ragged: the mixed-size call `DeviceInputPipeline(None, ...)` beside the fixed-size one, same B, target and scales, wall
and device time of each: the fixed-size call at 375x1242; the ragged call with all 36 frames at 375x1242; the ragged call
with the size mix of the first twelve lines of splits/eigen_zhou/train_files.txt; and that mix as one fixed-size call per
size present (what a caller had to do before).  The frames are resident on the device in all of them, as in the fixed-size
measurement; the ragged calls are also timed from a pinned host buffer, the copy of the frame bytes included.
"""
import argparse
import collections
import contextlib
import json
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppea-depth_amd")]

B, RAW_HW, H, W, SCALES, FRAMES = 12, (375, 1242), 192, 640, 4, (0, -1, 1)
HBM_BYTES_PER_S = 6.3e12


def algorithmic_bytes():
    """(read, written) per triplet."""
    read = len(FRAMES) * 3 * RAW_HW[0] * RAW_HW[1]
    pixels = sum((H >> s) * (W >> s) for s in range(SCALES))
    return read, len(FRAMES) * 3 * pixels * 4 * 2


def wall(fn, reps):
    fn()
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)


def kernel_us(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    per = collections.defaultdict(lambda: [0, 0.0])
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and e.name:
            m = re.search(r"lanczos_h_ragged3|lanczos_v_ragged|lanczos_h|lanczos_v|jitter_sum|jitter_out|repeat_rows|Memcpy \w+|Memset", e.name)
            name = m.group(0) if m else e.name[:48]
            per[name][0] += 1
            per[name][1] += e.time_range.elapsed_us()
    return {k: {"launches": n, "us": round(us, 1)} for k, (n, us) in sorted(per.items(), key=lambda kv: -kv[1][1])}


KITTI_DAY_HW = {"2011_09_26": (375, 1242), "2011_09_28": (370, 1224), "2011_09_29": (374, 1238), "2011_09_30": (370, 1226),
                "2011_10_03": (376, 1241)}
# the recording days of the first twelve lines of splits/eigen_zhou/train_files.txt: the first batch at --batch_size 12
FIRST_BATCH_DAYS = ["2011_09_26", "2011_09_29", "2011_09_26", "2011_09_30", "2011_10_03", "2011_10_03", "2011_09_30",
                    "2011_10_03", "2011_09_26", "2011_09_30", "2011_09_26", "2011_09_30"]


def emit(res, out):
    line = json.dumps(res)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def ragged_main(args):
    import numpy as np
    from ppeadepth import input_pipeline as ip
    dev = torch.device("cuda:0")
    g, rng = torch.Generator().manual_seed(77), np.random.default_rng(77)
    aug, flip = torch.rand(B, generator=g) > 0.5, torch.rand(B, generator=g) > 0.5
    aug[0], flip[0] = True, True
    jit = {(f, s): ip.draw_jitter_params(B, g) for f in FRAMES for s in range(SCALES)}

    def measure(fn):
        kernels = kernel_us(fn)
        return {"wall_ms": wall(fn, args.reps), "device_us": round(sum(v["us"] for v in kernels.values()), 1),
                "launches": sum(v["launches"] for v in kernels.values()), "kernels": kernels}

    def ragged_calls(sizes):
        raw = {f: [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in sizes] for f in FRAMES}
        pipe = ip.DeviceInputPipeline(None, H, W, dev)
        host = ip.pack_frames(raw, FRAMES)
        resident = ip.RaggedFrames(host.buf.to(dev), host.desc, host.sizes, host.batch)
        res = {"frames_on_device": measure(lambda: pipe(resident, aug, flip, jit)),
               "frames_in_pinned_host_memory": measure(lambda: pipe(host, aug, flip, jit))}
        assert (pipe.ragged.table_builds, pipe.ragged.table_uploads) == (len(set(sizes)), 1)
        return raw, res

    def fixed_call(raw, sizes, hw):
        """-> the fixed-size call on the items of size hw (planar frames on the device, as the fixed-size measurement)."""
        idx = [b for b, s in enumerate(sizes) if s == hw]
        planar = {f: torch.from_numpy(np.stack([raw[f][b] for b in idx])).permute(0, 3, 1, 2).contiguous().to(dev) for f in FRAMES}
        pipe = ip.DeviceInputPipeline(hw, H, W, dev)
        sub = {k: {n: t[idx] for n, t in p.items()} for k, p in jit.items()}
        return lambda: pipe(planar, aug[idx], flip[idx], sub)

    def level0_alone(raw, sizes):
        """Level 0 by itself, device events around `reps` calls, us per call: the ragged launch pair and, where the frames
        have one size, `ops.lanczos_resize_view_u8` on the same HWC bytes (lanczos_h_view3: the same staging and accumulation
        with the width, the table and the output row uniform over the launch)."""
        from ppeadepth import ops
        level0, frames = ip.RaggedLevel0((H, W), dev, "hip"), ip.pack_frames(raw, FRAMES)
        desc, (taps_h, taps_v), buf = level0.describe(frames), level0.tables(), frames.buf.to(dev)
        words = torch.cat([desc.reshape(-1), ops.ragged_row_prefix(desc)]).to(dev)
        fl = flip.to(torch.int32).repeat(len(FRAMES)).to(dev)
        nz = torch.empty(len(frames), dtype=torch.int32, device=dev)
        calls = {"ragged": lambda: ops.lanczos_resize_ragged_u8(buf, (desc, words), (H, W), taps_h, taps_v, fl, nz)}
        if len(set(sizes)) == 1:
            view, rs = buf.view(len(frames), sizes[0][0], sizes[0][1], 3), ip.LanczosResize(sizes[0], (H, W), dev, "hip", first=True)
            calls["view_one_size"] = lambda: rs.views(view, fl, nz)
            assert torch.equal(calls["view_one_size"](), calls["ragged"]())
        out = {}
        for name, fn in calls.items():
            runs = []
            for _ in range(3):
                fn()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(args.reps):
                    fn()
                e.record()
                torch.cuda.synchronize()
                runs.append(round(s.elapsed_time(e) * 1e3 / args.reps, 1))
            out[name] = {"us_per_call_runs": runs, "kernels": kernel_us(fn)}
        return out

    one = [RAW_HW] * B
    raw_one, ragged_one = ragged_calls(one)
    mix = [KITTI_DAY_HW[d] for d in FIRST_BATCH_DAYS]
    raw_mix, ragged_mix = ragged_calls(mix)
    per_class = [fixed_call(raw_mix, mix, hw) for hw in sorted(set(mix))]
    res = {"metric": "DeviceInputPipeline call, B=12 triplets -> 192x640, 4 scales, parameters pre-drawn; wall ms median (min, "
                     "max) over reps, device us = every device event of one call",
           "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "mix": {"%dx%d" % hw: mix.count(hw) for hw in sorted(set(mix))},
           "b_fixed_375x1242": measure(fixed_call(raw_one, one, RAW_HW)),
           "c_ragged_all_375x1242": ragged_one,
           "d_ragged_first_eigen_zhou_batch": ragged_mix,
           "e_one_fixed_call_per_size_of_d": measure(lambda: [fn() for fn in per_class]),
           "level0_alone": {"all_375x1242": level0_alone(raw_one, one), "first_eigen_zhou_batch": level0_alone(raw_mix, mix)},
           "command": "python tools/bench_input_pipeline.py --ragged --reps %d" % args.reps}
    emit(res, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--backend", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ragged", action="store_true")
    args = ap.parse_args()
    if args.ragged:
        return ragged_main(args)
    from ppeadepth import input_pipeline as ip
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(77)
    raw = {f: torch.randint(0, 256, (B, 3) + RAW_HW, generator=g, dtype=torch.uint8).to(dev) for f in FRAMES}
    kw = {} if args.backend is None else {"backend": args.backend}
    pipe = ip.DeviceInputPipeline(RAW_HW, H, W, dev, **kw)
    aug, flip = torch.rand(B, generator=g) > 0.5, torch.rand(B, generator=g) > 0.5
    aug[0], flip[0] = True, True
    jit = {(f, s): ip.draw_jitter_params(B, g) for f in FRAMES for s in range(SCALES)}

    def draws():
        for _ in range(len(FRAMES) * SCALES):
            ip.draw_jitter_params(B, g)

    t = time.perf_counter()
    for _ in range(args.reps):
        draws()
    draw_ms = (time.perf_counter() - t) * 1e3 / args.reps
    read, written = algorithmic_bytes()
    floor_us = B * (read + written) / HBM_BYTES_PER_S * 1e6
    kernels = kernel_us(lambda: pipe(raw, aug, flip, jit))
    device_us = sum(v["us"] for v in kernels.values())
    res = {"metric": "DeviceInputPipeline call, B=12 triplets 375x1242 -> 192x640, 4 scales; wall ms median (min, max)",
           "backend": getattr(pipe, "backend", "torch"), "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "call_ms_drawing_inside": wall(lambda: pipe(raw, generator=g), args.reps),
           "call_ms_predrawn": wall(lambda: pipe(raw, aug, flip, jit), args.reps),
           "host_draws_ms": round(draw_ms, 3),
           "bytes_per_triplet": {"read": read, "written": written},
           "hbm_floor_us_per_batch_at_6.3TBps": round(floor_us, 1),
           "device_us_per_batch": round(device_us, 1),
           "share_of_hbm_bound": round(floor_us / device_us, 4) if device_us else None,
           "kernels": kernels,
           "command": "python tools/bench_input_pipeline.py --reps %d" % args.reps}
    emit(res, args.out)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
