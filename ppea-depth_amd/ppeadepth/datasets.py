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

Cityscapes has the same split: `CityscapesPreprocessedDataset` + `collate_cityscapes` feed `CityscapesInputPipeline` (the wide
training triplets), `CityscapesEvalDataset` + `collate_cityscapes_eval` feed `CityscapesEvalPipeline` (the raw test frames).
All files of a split have one size, the first item's; the pipeline is built with it.

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


def _decode_rgb(path):
    """The decoded file, uint8 [H,W,3] (the reference's `pil_loader`); FileNotFoundError names the path."""
    from PIL import Image
    with open(path, "rb") as f:
        with Image.open(f) as img:
            return np.array(img.convert("RGB"))


class _FixedSizeFolder:
    """What the two Cityscapes readers share: the split lines "<city> <frame_name>" and one frame size for the whole split,
    taken from its first item (`frame_hw`, read lazily); an item of another size is a ValueError that names the file."""

    def __init__(self, data_path, filenames):
        self.data_path, self.filenames = data_path, list(filenames)
        self._hw = None

    def __len__(self):
        return len(self.filenames)

    def index_to_folder_and_frame_idx(self, index):
        """-> (city, frame name, side = None) of line `index`."""
        city, frame_name = self.filenames[index].split()
        return city, frame_name, None

    def _first_hw(self):
        raise NotImplementedError

    @property
    def frame_hw(self):
        """(H, W) of one decoded file of this split: the first item's."""
        if self._hw is None:
            self._hw = self._first_hw()
        return self._hw

    def _sized(self, path):
        img = _decode_rgb(path)
        if tuple(img.shape[:2]) != self.frame_hw:
            raise ValueError(f"{path}: {img.shape[0]} x {img.shape[1]}, the split's first item is {self.frame_hw[0]} x "
                             f"{self.frame_hw[1]} and the pipeline is built for that size")
        return img


class CityscapesPreprocessedDataset(_FixedSizeFolder):
    """The preprocessed Cityscapes triplets (reference datasets/cityscapes_preprocessed_dataset.py): line "<city> <frame_name>"
    -> `<data_path>/<city>/<frame_name>.jpg`, one wide image that holds frames -1, 0, +1 side by side, and
    `<data_path>/<city>/<frame_name>_cam.txt`.  An item is {"triplet": uint8 [H, 3W, 3], "camera": float64 [3,3]}; the thirds
    are read in place by `CityscapesInputPipeline`, which is built with `raw_hw`."""

    def get_image_path(self, city, frame_name):
        return os.path.join(self.data_path, city, "{}.jpg".format(frame_name))

    def get_camera_path(self, city, frame_name):
        return os.path.join(self.data_path, city, "{}_cam.txt".format(frame_name))

    def _first_hw(self):
        city, frame_name, _ = self.index_to_folder_and_frame_idx(0)
        return tuple(_decode_rgb(self.get_image_path(city, frame_name)).shape[:2])

    @property
    def raw_hw(self):
        """(H, W) of ONE frame of the wide image (384 x 1024 for the real data)."""
        h, w3 = self.frame_hw
        if w3 % 3:
            city, frame_name, _ = self.index_to_folder_and_frame_idx(0)
            raise ValueError(f"{self.get_image_path(city, frame_name)}: {w3} columns do not hold three frames side by side")
        return h, w3 // 3

    def __getitem__(self, index):
        from .input_pipeline import read_cityscapes_cam_txt
        city, frame_name, _ = self.index_to_folder_and_frame_idx(index)
        return {"triplet": self._sized(self.get_image_path(city, frame_name)),
                "camera": read_cityscapes_cam_txt(self.get_camera_path(city, frame_name))}


class CityscapesEvalDataset(_FixedSizeFolder):
    """The raw Cityscapes test frames (reference datasets/cityscapes_evaldataset.py): frame 0 is
    `<data_path>/leftImg8bit/test/<city>/<frame_name>_leftImg8bit.png`, frame -1 the frame TWO before it in
    `leftImg8bit_sequence` (`get_offset_framename`), the camera `camera_trainvaltest/camera/test/<city>/<frame_name>_camera.json`.
    An item is {0: uint8 [H,W,3], -1: uint8 [H,W,3], "camera": float64 [3,3]}; the crop to the top three quarters is
    `CityscapesEvalPipeline`'s.  A missing file is a FileNotFoundError that names it: there is no blank-frame rule here."""

    def __init__(self, data_path, filenames, frame_idxs=(0, -1)):
        if any(f not in (0, -1) for f in frame_idxs) or 0 not in frame_idxs:
            raise ValueError(f"frame_idxs {tuple(frame_idxs)}: the evaluation loader holds frames 0 and -1")
        super().__init__(data_path, filenames)
        self.frame_idxs = tuple(frame_idxs)

    @staticmethod
    def get_offset_framename(frame_name, offset=-2):
        city, seq, frame_num = frame_name.split("_")
        return "{}_{}_{}".format(city, seq, str(int(frame_num) + offset).zfill(6))

    def get_image_path(self, city, frame_name, is_sequence=False):
        folder = "leftImg8bit_sequence" if is_sequence else "leftImg8bit"
        return os.path.join(self.data_path, folder, "test", city, frame_name + "_leftImg8bit.png")

    def get_camera_path(self, city, frame_name):
        return os.path.join(self.data_path, "camera_trainvaltest", "camera", "test", city, frame_name + "_camera.json")

    def _first_hw(self):
        city, frame_name, _ = self.index_to_folder_and_frame_idx(0)
        return tuple(_decode_rgb(self.get_image_path(city, frame_name)).shape[:2])

    raw_hw = _FixedSizeFolder.frame_hw

    def __getitem__(self, index):
        from .input_pipeline import read_cityscapes_camera_json
        city, frame_name, _ = self.index_to_folder_and_frame_idx(index)
        item = {}
        for f in self.frame_idxs:
            name = frame_name if f == 0 else self.get_offset_framename(frame_name, -2)
            item[f] = self._sized(self.get_image_path(city, name, is_sequence=f != 0))
        item["camera"] = read_cityscapes_camera_json(self.get_camera_path(city, frame_name))
        return item


def collate_cityscapes(items):
    """A list of `CityscapesPreprocessedDataset` items -> (triplets uint8 [B,H,3W,3], cameras float64 [B,3,3]), the two
    arguments of `CityscapesInputPipeline`.  Host work only, nothing is pinned in a worker."""
    import torch
    return (torch.from_numpy(np.stack([it["triplet"] for it in items])),
            torch.from_numpy(np.stack([it["camera"] for it in items])))


def collate_cityscapes_eval(items):
    """A list of `CityscapesEvalDataset` items -> ({frame id: uint8 [B,H,W,3]}, cameras float64 [B,3,3]), the two arguments
    of `CityscapesEvalPipeline`.  Host work only, nothing is pinned in a worker."""
    import torch
    frames = {f: torch.from_numpy(np.stack([it[f] for it in items])) for f in items[0] if f != "camera"}
    return frames, torch.from_numpy(np.stack([it["camera"] for it in items]))


def collate_raw(items, pin=False):
    """A list of `KITTIRAWDataset` items -> `input_pipeline.RaggedFrames`, what `DeviceInputPipeline(None, ...)` takes: the
    `collate_fn` of a DataLoader.  Host work only (pin=False: a worker process must not touch the GPU; the loader's
    `pin_memory=True` pins the buffer in the main process)."""
    from .input_pipeline import pack_frames
    frame_idxs = list(items[0])
    return pack_frames({f: [it[f] for it in items] for f in frame_idxs}, frame_idxs, pin=pin)
