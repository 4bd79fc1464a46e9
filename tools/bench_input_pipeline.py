"""Where the time of one `DeviceInputPipeline` call goes (B = 12 triplets, 375x1242 -> 192x640, as `bench.py --input_pipeline`).

    python tools/bench_input_pipeline.py [--reps 20] [--backend hip|torch] [--out FILE]

Per call: the wall time with the parameters drawn inside the call (what bench.py times), the wall time with pre-drawn
parameters, the host-side draws alone (144 `randperm` / `uniform_` groups; no device work), the device time of every kernel
from the profiler, and the algorithmic HBM traffic computed from the shapes (raw uint8 frames read once, `color` and
`color_aug` written once in fp32 at every scale) with its streaming floor at 6.3 TB/s.  Prints ONE JSON line.
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
            m = re.search(r"lanczos_h|lanczos_v|jitter_sum|jitter_out|repeat_rows|Memcpy \w+|Memset", e.name)
            name = m.group(0) if m else e.name[:48]
            per[name][0] += 1
            per[name][1] += e.time_range.elapsed_us()
    return {k: {"launches": n, "us": round(us, 1)} for k, (n, us) in sorted(per.items(), key=lambda kv: -kv[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--backend", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
