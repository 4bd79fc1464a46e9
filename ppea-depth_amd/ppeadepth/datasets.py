"""KITTI raw from disk: the frames of a split file's lines, decoded and nothing else.

What the reference's `datasets/kitti_dataset.py` + `mono_dataset.py` do per item on CPU workers splits in two here: this
module finds and decodes the files (Pillow, `convert("RGB")`), and everything that follows -- flip, the LANCZOS pyramid,
ColorJitter, ToTensor, K / inv_K -- is `input_pipeline.DeviceInputPipeline(None, ...)` on the whole batch, which takes
frames of different sizes (KITTI raw has one frame size per recording day, and the shuffled split mixes the days in every
batch).  No resize, flip, jitter or intrinsics happen on the host.

    lines = readlines("splits/eigen_zhou/train_files.txt")
    data = KITTIRAWDataset(data_path, lines, frame_idxs=(0, -1, 1))
    loader = torch.utils.data.DataLoader(data, batch_size=12, collate_fn=collate_raw, num_workers=8, pin_memory=True)
    pipe = DeviceInputPipeline(None, 192, 640, "cuda")
    for frames in loader:
        inputs = pipe(frames)

Not served here: the stereo frame "s", the odometry and the depth-benchmark folder layouts (`KITTIOdomDataset`,
`KITTIDepthDataset`), and `get_depth` (ground truth comes from `DeviceGroundTruth.from_velodyne`).
"""
import os

import numpy as np


def readlines(filename):
    """The lines of a text file, without their line ends."""
    with open(filename, "r") as f:
        return f.read().splitlines()


class KITTIRAWDataset:
    """Items of a KITTI raw folder.  filenames: lines "<folder> <frame index> <l|r>" (a line of one word is frame 0 with
    no side, as the reference reads it); frame_idxs: temporal offsets, 0 first or anywhere.  An item is
    {frame id: uint8 [H,W,3] array, or None where that neighbour's file does not exist}."""

    side_map = {"2": 2, "3": 3, "l": 2, "r": 3}

    def __init__(self, data_path, filenames, frame_idxs, img_ext=".jpg"):
        if any(not isinstance(i, int) for i in frame_idxs):
            raise ValueError(f"frame_idxs {tuple(frame_idxs)}: temporal offsets only (the stereo frame 's' is not served)")
        self.data_path, self.filenames, self.frame_idxs, self.img_ext = data_path, list(filenames), tuple(frame_idxs), img_ext

    def __len__(self):
        return len(self.filenames)

    def index_to_folder_and_frame_idx(self, index):
        """-> (folder, frame index, side) of line `index`."""
        words = self.filenames[index].split()
        if len(words) == 3:
            return words[0], int(words[1]), words[2]
        return words[0], 0, None

    def get_image_path(self, folder, frame_index, side):
        name = "{:010d}{}".format(frame_index, self.img_ext)
        return os.path.join(self.data_path, folder, "image_0{}/data".format(self.side_map[side]), name)

    def get_color(self, folder, frame_index, side):
        """The decoded frame, uint8 [H,W,3]; FileNotFoundError when the file does not exist."""
        from PIL import Image
        with open(self.get_image_path(folder, frame_index, side), "rb") as f:
            with Image.open(f) as img:
                return np.array(img.convert("RGB"))

    def __getitem__(self, index):
        folder, frame_index, side = self.index_to_folder_and_frame_idx(index)
        item = {}
        for i in self.frame_idxs:
            try:
                item[i] = self.get_color(folder, frame_index + i, side)
            except FileNotFoundError as e:
                if i != 0:
                    item[i] = None              # a missing neighbour: the pipeline writes it as zeros and never jitters it
                    continue
                raise FileNotFoundError("Cannot find frame - make sure your --data_path is set correctly, or try adding "
                                        f"the --png flag. {e}") from e
        return item


def collate_raw(items, pin=False):
    """A list of `KITTIRAWDataset` items -> `input_pipeline.RaggedFrames`, what `DeviceInputPipeline(None, ...)` takes: the
    `collate_fn` of a DataLoader.  Host work only (pin=False: a worker process must not touch the GPU; the loader's
    `pin_memory=True` pins the buffer in the main process)."""
    from .input_pipeline import pack_frames
    frame_idxs = list(items[0])
    return pack_frames({f: [it[f] for it in items] for f in frame_idxs}, frame_idxs, pin=pin)
