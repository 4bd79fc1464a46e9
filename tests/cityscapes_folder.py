"""A synthetic Cityscapes on disk for tests/test_cityscapes_run_{cpu,gpu}.py: preprocessed triplets (`<city>/<frame>.jpg` +
`_cam.txt`), raw evaluation frames with their `-2` sequence frames and `_camera.json`, the two split files and, on request,
the single-file ground truth.  Not a test module."""
import json
import os

import numpy as np

CITIES = ("aachen", "ulm")


def _image(g, h, w, phase):
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 100 * np.sin(x / 9.0 + phase + c) * np.cos(y / 7.0) for c in range(3)], -1)
    return np.clip(img + g.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


def train_names(n):
    """n lines "<city> <city>_<seq>_<frame>", the cities alternating."""
    return [f"{CITIES[i % 2]} {CITIES[i % 2]}_{i // 2:06d}_{19 + i:06d}" for i in range(n)]


def eval_names(n):
    """n evaluation lines; the frame numbers 100 and 12 lose a digit at -2 (000098, 000010): the zero fill is needed."""
    frames = [100, 12, 19, 7, 23]
    return [f"{CITIES[i % 2]} {CITIES[i % 2]}_{i:06d}_{frames[i % len(frames)]:06d}" for i in range(n)]


def make(root, triplet_hw, eval_hw, n_train, n_eval, gt_hw=None, seed=11):
    """-> {"root", "data" (triplets), "eval" (raw frames), "splits", "train" / "test" (the lines)}.  triplet_hw: one frame
    of the wide image."""
    from PIL import Image
    g = np.random.default_rng(seed)
    root = str(root)
    data, raw, splits = (os.path.join(root, d) for d in ("cs_triplets", "cityscapes", "splits"))
    train, test = train_names(n_train), eval_names(n_eval)
    for i, line in enumerate(train):
        city, name = line.split()
        os.makedirs(os.path.join(data, city), exist_ok=True)
        h, w = triplet_hw
        wide = np.concatenate([_image(g, h, w, i + 0.3 * k) for k in range(3)], 1)           # frames -1, 0, +1
        Image.fromarray(wide).save(os.path.join(data, city, name + ".jpg"), quality=95)
        with open(os.path.join(data, city, name + "_cam.txt"), "w") as f:
            f.write(f"{1131.25 + i},0.0,{523.5 - i},0.0,{1130.0 + 2 * i},{191.25 + i},0.0,0.0,1.0\n")
    for i, line in enumerate(test):
        city, name = line.split()
        c, seq, num = name.split("_")
        prev = f"{c}_{seq}_{int(num) - 2:06d}"
        for folder, frame, phase in (("leftImg8bit", name, i), ("leftImg8bit_sequence", prev, i - 0.4)):
            os.makedirs(os.path.join(raw, folder, "test", city), exist_ok=True)
            Image.fromarray(_image(g, *eval_hw, phase)).save(os.path.join(raw, folder, "test", city, frame + "_leftImg8bit.png"))
        os.makedirs(os.path.join(raw, "camera_trainvaltest", "camera", "test", city), exist_ok=True)
        with open(os.path.join(raw, "camera_trainvaltest", "camera", "test", city, name + "_camera.json"), "w") as f:
            json.dump({"extrinsic": {"baseline": 0.209313}, "intrinsic": {"fx": 2262.52 + i, "fy": 2265.3017905988554 - i,
                                                                         "u0": 1096.98 + i, "v0": 513.137 - i}}, f)
    os.makedirs(os.path.join(splits, "cityscapes_preprocessed"), exist_ok=True)
    for name, lines in (("train", train), ("test", test)):
        with open(os.path.join(splits, "cityscapes_preprocessed", f"{name}_files.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    if gt_hw is not None:
        os.makedirs(os.path.join(splits, "cityscapes", "gt_depths"), exist_ok=True)
        for i in range(n_eval):
            np.save(os.path.join(splits, "cityscapes", "gt_depths", str(i).zfill(3) + "_depth.npy"),
                    g.uniform(2.0, 60.0, gt_hw).astype(np.float32))
    return {"root": root, "data": data, "eval": raw, "splits": splits, "train": train, "test": test}
