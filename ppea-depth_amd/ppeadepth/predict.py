"""From a checkpoint and a folder of KITTI raw frames to files on disk.

    python -m ppeadepth.predict --data_path KITTI --split_file splits/eigen/test_files.txt --load_weights_folder CKPT \
        --out OUT --batch_size 12 --adapter --depth_npy --benchmark --colour

Each product can be switched on alone; file n belongs to line n of the split file:
  --depth_npy   OUT/depth/<n>.npy       fp32 metres at the frame's own size (clamp 1e-3 .. 80, --pred_depth_scale_factor)
  --benchmark   OUT/benchmark/<n>.png   the KITTI depth benchmark's 16-bit PNG of depth * 256 at 352x1216, --scale (5.4)
                                        (eval_depth_ori.py:318-333)
  --colour      OUT/colour/<n>.png      the disparity through --cmap at the frame's own size, range minimum .. --percentile
  --ply         OUT/ply/<n>.ply         the frame's 3D points in the camera frame at its own size, coloured with the frame's
                                        bytes (binary PLY; same scale and clamp as --depth_npy; --ply_stride, --ply_edge)
--teacher predicts with the single-frame network instead of the multi-frame one.  Every other flag is a model option
(`options.MonodepthOptions`: --height, --width, --adapter, --num_matching_frames, ...) and must describe the checkpoint.

The frames are read by `datasets.KITTIRAWDataset` at their own sizes and resized by `DeviceInputPipeline(None, ...)`; the
per-pixel work of every product is a HIP launch (`DepthPredictor.depth` / `.render` / `.points`), one copy to the host per batch and
product, and Pillow writes the files.
"""
import argparse
import os

import numpy as np
import torch

BENCHMARK_HW = (352, 1216)


def _parser():
    p = argparse.ArgumentParser(description="PPEA-Depth prediction export; other flags: options.MonodepthOptions")
    a = p.add_argument
    a("--data_path", required=True)
    a("--split_file", required=True)
    a("--out", required=True)
    a("--teacher", action="store_true")
    a("--depth_npy", action="store_true")
    a("--benchmark", action="store_true")
    a("--scale", type=float, default=5.4)
    a("--colour", action="store_true")
    a("--cmap", default="plasma")
    a("--percentile", type=float, default=95.0)
    a("--ply", action="store_true")
    a("--ply_stride", type=int, default=1, help="every n-th row and column becomes a point")
    a("--ply_edge", type=float, default=0.0, help="drop points whose depth differs from a neighbour's by more than this share")
    a("--png", action="store_true", help="the frames are .png files (default .jpg)")
    a("--device", default=None)
    a("--fp32", action="store_true", help="predict in fp32 (default bf16)")
    return p


def _images(res, B):
    """What `depth` / `render` returned -> B host arrays: ONE copy of the whole batch, then views."""
    if isinstance(res, tuple):
        flat, table = res[0].cpu().numpy(), res[1].cpu().tolist()
        return [flat[o:o + h * w].reshape((h, w) + flat.shape[1:]) for o, h, w in table]
    host = res.cpu().numpy()
    return [host[b] for b in range(B)]


def save_png(path, array):
    """uint16 [H,W] -> a 16-bit grey PNG (mode I;16), uint8 [H,W,3] -> RGB."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(array)).save(path)


@torch.no_grad()
def main(argv=None):
    from . import datasets, networks, options
    from .inference import DepthPredictor
    from .input_pipeline import DeviceInputPipeline
    from .trainer import Trainer
    args, rest = _parser().parse_known_args(argv)
    opt = options.MonodepthOptions().parse(rest)
    options.apply_train_cs(opt)
    options.apply_ddad(opt)
    if not opt.load_weights_folder:
        raise SystemExit("--load_weights_folder is required")
    if not (args.depth_npy or args.benchmark or args.colour or args.ply):
        raise SystemExit("nothing to write: give --depth_npy, --benchmark, --colour and / or --ply")
    device = torch.device(args.device if args.device else ("cuda" if torch.cuda.is_available() else "cpu"))
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    model = networks.RepDepth(opt).to(device)
    trainer = Trainer(opt, model, device)
    trainer.load_model(opt.load_weights_folder)
    p = DepthPredictor(model, opt, amp_dtype=None if args.fp32 else torch.bfloat16)
    ids = [0] + ([] if args.teacher else p.lookup_ids)
    lines = datasets.readlines(args.split_file)
    data = datasets.KITTIRAWDataset(args.data_path, lines, ids, ".png" if args.png else ".jpg")
    pipe = DeviceInputPipeline(None, opt.height, opt.width, device, frame_idxs=tuple(ids), is_train=False)
    dirs = {k: os.path.join(args.out, k) for k, on in (("depth", args.depth_npy), ("benchmark", args.benchmark),
                                                       ("colour", args.colour), ("ply", args.ply)) if on}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    tracker = trainer.depth_bin_tracker
    for start in range(0, len(data), opt.batch_size):
        frames = datasets.collate_raw([data[i] for i in range(start, min(start + opt.batch_size, len(data)))])
        B = frames.batch
        desc = frames.desc.view(len(ids), B, 4)
        sizes = [(int(h), int(w)) for h, w in desc[0, :, 1:3].tolist()]
        if args.ply:
            # the frames' bytes go to the device here instead of inside the pipeline (still the one copy): the points take
            # their colour from them
            frames.buf = frames.buf.to(device, non_blocking=True)
        inputs = pipe(frames)
        color0 = inputs[("color", 0, 0)]
        if args.teacher:
            disp = p.predict_mono(color0)
        else:
            mn, mx = (tracker.min_depth, tracker.max_depth) if getattr(opt, "notadabins", False) else tracker.compute()
            looks = [inputs[("color", f, 0)] for f in ids[1:]]
            keep = (desc[1:, :, 1] > 0).t().contiguous()                   # [B,F]: a neighbour whose file does not exist
            disp = p.predict(color0, looks[0] if len(looks) == 1 else torch.stack(looks, 1), inputs[("K", 2)],
                             inputs[("inv_K", 2)], mn, mx, keep=None if bool(keep.all()) else keep.float())["disp"]
        names = ["{:010d}".format(start + b) for b in range(B)]
        if args.depth_npy:
            maps = _images(p.depth(disp, sizes, scale=opt.pred_depth_scale_factor), B)
            for n, m in zip(names, maps):
                np.save(os.path.join(dirs["depth"], n + ".npy"), m)
        if args.benchmark:
            maps = _images(p.depth(disp, BENCHMARK_HW, scale=args.scale, lo=0.0, hi=80.0, dtype=torch.uint16), B)
            for n, m in zip(names, maps):
                save_png(os.path.join(dirs["benchmark"], n + ".png"), m)
        if args.colour:
            imgs = _images(p.render(disp, sizes, percentile=args.percentile, cmap=args.cmap), B)
            for n, m in zip(names, imgs):
                save_png(os.path.join(dirs["colour"], n + ".png"), m)
        if args.ply:
            from . import vis
            from .input_pipeline import KITTI_K
            cloud = p.points(disp, sizes, p.full_inv_K(getattr(data, "K", KITTI_K), sizes), color=frames.buf,
                             color_offsets=desc[0, :, 0].to(device, torch.int64).contiguous(),
                             scale=opt.pred_depth_scale_factor, stride=args.ply_stride, edge=args.ply_edge)
            # one copy of the batch's points (and one of the B counts that split them)
            xyz, rgb, _, _ = (t.cpu().numpy() if torch.is_tensor(t) else t for t in cloud.trim())
            ends = np.cumsum(cloud.counts.cpu().numpy())
            for b, n in enumerate(names):
                lo_, hi_ = int(ends[b - 1]) if b else 0, int(ends[b])
                vis.write_ply(os.path.join(dirs["ply"], n + ".ply"), xyz[lo_:hi_], rgb[lo_:hi_])
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
