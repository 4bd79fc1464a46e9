"""The two Cityscapes pipelines at their real sizes, B = 12: the view path (the first horizontal pass reads the decoder's
HWC frames in place, `ops.lanczos_resize_view_u8`) against the composite a caller could write before it existed, from the
older operators only: a device `permute().contiguous()` per frame, then the dense pass (`ops.lanczos_resize_u8`).

    python tools/bench_cityscapes_pipeline.py [--reps 100] [--runs 3] [--out profiles/cityscapes_pipeline.json]

    training     one wide image per item, uint8 [12, 384, 3072, 3] (42 MB) -> 192x512, 4 levels, flip + ColorJitter
    evaluation   frames 0 and -1, uint8 [12, 1024, 2048, 3] each (2 x 75 MB), top 768 rows -> 192x512, 4 levels

For each pipeline two things are timed, `--runs` runs of `--reps` calls each with the two paths ALTERNATING run by run
(device events around a run; every shape warmed first): the first level alone (where the two paths differ) and the whole
call with pre-drawn parameters; both paths of a call compute and upload the same per-sample intrinsics on the host.  A
whole call is bound by its host side (Python, 48 float32 `pinv`), so the device time of one call, summed over its kernels
and copies by the profiler in a run of its own, is reported beside it.  The outputs of the two paths are compared byte for
byte before anything is timed.  Prints ONE JSON line with every run, the medians and max - min."""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppea-depth_amd")]

B, H, W, SCALES = 12, 192, 512, 4
TRAIN_HW, TRAIN_FRAMES = (384, 1024), (0, -1, 1)
EVAL_HW, EVAL_FRAMES = (1024, 2048), (0, -1)


def run_ms(fn, reps):
    """ms per call of one run: device events around `reps` calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def alternate(paths, reps, runs):
    """{name: fn} -> {name: {"runs_ms": [...], "median_ms", "max_minus_min_ms"}}, the paths alternating run by run."""
    for fn in paths.values():
        for _ in range(3):
            fn()
    got = {k: [] for k in paths}
    for _ in range(runs):
        for k, fn in paths.items():
            got[k].append(run_ms(fn, reps))
    return {k: {"runs_ms": [round(v, 4) for v in ms], "median_ms": round(statistics.median(ms), 4),
                "max_minus_min_ms": round(max(ms) - min(ms), 4)} for k, ms in got.items()}


def device_us(fn):
    """Device time of one call: kernels, copies and memsets, from the profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and e.name]
    return {"launches": len(ev), "us": round(sum(e.time_range.elapsed_us() for e in ev), 1)}


def verdict(r):
    """The view path wins only if its slowest run beats the composite's fastest."""
    return max(r["view"]["runs_ms"]) < min(r["composite"]["runs_ms"])


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ppeadepth import input_pipeline as ip, ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(77)
    res = {"metric": "Cityscapes pipelines, B=12 -> 192x512, 4 levels: ms per call, view path vs permute().contiguous() + dense "
                     "pass; runs alternate",
           "device": torch.cuda.get_device_name(0), "reps_per_run": args.reps, "runs": args.runs,
           "command": "python tools/bench_cityscapes_pipeline.py --reps %d --runs %d" % (args.reps, args.runs)}

    # ---- training: the wide image ----
    Hraw, Wraw = TRAIN_HW
    trip = torch.randint(0, 256, (B, Hraw, 3 * Wraw, 3), dtype=torch.uint8, device=dev)
    trip[3, :, 2 * Wraw:] = 0                                      # a missing neighbour
    cams = torch.tensor([[1131.0, 0, 523.0], [0, 1130.0, 191.0], [0, 0, 1]]).repeat(B, 1, 1)
    aug, flip = torch.rand(B, generator=g) > 0.5, torch.rand(B, generator=g) > 0.5
    aug[0], flip[0] = True, True
    jit = {(f, s): ip.draw_jitter_params(B, g) for f in TRAIN_FRAMES for s in range(SCALES)}
    view_pipe = ip.CityscapesInputPipeline(dev, H, W, TRAIN_HW)
    dense_pipe = ip.DeviceInputPipeline(TRAIN_HW, H, W, dev, frame_idxs=TRAIN_FRAMES)      # its K is KITTI's: replaced below
    thirds = [trip[:, :, (f + 1) * Wraw:(f + 2) * Wraw] for f in TRAIN_FRAMES]
    rs = view_pipe.resize[0]
    flip_dev = flip.to(torch.int32).repeat(len(TRAIN_FRAMES)).to(dev)
    nz = torch.empty(len(TRAIN_FRAMES) * B, dtype=torch.int32, device=dev)

    def planar_thirds():
        return {f: t.permute(0, 3, 1, 2).contiguous() for f, t in zip(TRAIN_FRAMES, thirds)}

    level0 = {"view": lambda: ops.lanczos_resize_view_u8(thirds, (H, W), rs.taps_h, rs.taps_v, flip_dev, nz),
              "composite": lambda: ops.lanczos_resize_u8(list(planar_thirds().values()), (H, W), rs.taps_h, rs.taps_v,
                                                         flip_dev, nz)}

    def composite_train():
        out = dense_pipe(planar_thirds(), aug, flip, jit)
        kk = torch.from_numpy(ip.cityscapes_intrinsics(cams, Wraw, Hraw, W, H, SCALES)).to(dev)
        for s in range(SCALES):
            out[("K", s)], out[("inv_K", s)] = kk[s, 0], kk[s, 1]
        return out

    call = {"view": lambda: view_pipe(trip, cams, aug, flip, jit), "composite": composite_train}
    assert torch.equal(level0["view"](), level0["composite"]()) and same(call["view"](), call["composite"]())
    res["training"] = {"raw_bytes": trip.numel(), "level0": alternate(level0, args.reps, args.runs),
                       "call": alternate(call, args.reps, args.runs),
                       "call_device": {k: device_us(fn) for k, fn in call.items()}}
    del trip, thirds

    # ---- evaluation: the raw frames, cropped ----
    Hraw, Wraw = EVAL_HW
    raw = {f: torch.randint(0, 256, (B, Hraw, Wraw, 3), dtype=torch.uint8, device=dev) for f in EVAL_FRAMES}
    cams = torch.tensor([[2262.52, 0, 1096.98], [0, 2265.30, 513.137], [0, 0, 1]]).repeat(B, 1, 1)
    view_pipe = ip.CityscapesEvalPipeline(dev, H, W, EVAL_HW)
    rs, crop = view_pipe.resize, view_pipe.crop_h
    top = [raw[f][:, :crop] for f in EVAL_FRAMES]
    params = torch.zeros(len(EVAL_FRAMES) * B, ops.JITTER_PARAM_WORDS, device=dev, dtype=torch.int32)

    def planar_tops():
        return [t.permute(0, 3, 1, 2).contiguous() for t in top]

    def composite_call():
        """CityscapesEvalPipeline's call with the dense first level (the intrinsics' upload included)."""
        out = {}
        kk = torch.from_numpy(ip.cityscapes_intrinsics(cams, Wraw, Hraw * 0.75, W, H, SCALES)).to(dev)
        img = planar_tops()
        for s in range(SCALES):
            img = rs[s](img)
            color, aug_ = ops.color_jitter_u8(img, params)
            for fi, f in enumerate(EVAL_FRAMES):
                out[("color", f, s)], out[("color_aug", f, s)] = color[fi * B:(fi + 1) * B], aug_[fi * B:(fi + 1) * B]
            out[("K", s)], out[("inv_K", s)] = kk[s, 0], kk[s, 1]
        return out

    level0 = {"view": lambda: ops.lanczos_resize_view_u8(top, (H, W), rs[0].taps_h, rs[0].taps_v),
              "composite": lambda: ops.lanczos_resize_u8(planar_tops(), (H, W), rs[0].taps_h, rs[0].taps_v)}
    call = {"view": lambda: view_pipe(raw, cams), "composite": composite_call}
    assert torch.equal(level0["view"](), level0["composite"]()) and same(call["view"](), call["composite"]())
    res["evaluation"] = {"raw_bytes": sum(v.numel() for v in raw.values()), "level0": alternate(level0, args.reps, args.runs),
                         "call": alternate(call, args.reps, args.runs),
                         "call_device": {k: device_us(fn) for k, fn in call.items()}}

    res["outputs_equal"] = True
    res["view_wins"] = {k: {m: verdict(res[k][m]) for m in ("level0", "call")} for k in ("training", "evaluation")}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
