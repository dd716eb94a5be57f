"""`resnet50-2d-lstm/src/data_config/dataset.py` drop-in: `VideoDataset(root_dir, split, sampling_method,
sequence_length, transform=None, logger=None)` (dataset.py:19-219) and `create_dataloaders`, the three
loaders of resnet50-2d-lstm/main.py:161-170.

Classes: `<root_dir>/<split>/non_referral` (label 0) first, then `referral` (label 1), in that order
(dataset.py:41-51; the folder name carries an underscore, unlike the other four families').  `labels`
is a list of ints: the trainer derives `pos_weight` from it.  Sampling: `random.seed(42)` on every call
(vclip_amd.sampling.LstmSampler, bit-exact).  The decoded span is the reference's
`get_clip(max(0, t0 - 0.01), min(duration, tN + 0.1))` with timestamps index / 30, the dataset's constant
fps (dataset.py:192-202).  The transform chain runs on the GPU: UniformTemporalSubsample(sequence_length),
then RandomShortSideScale(256, 320) / RandomCrop(224) / RandomHorizontalFlip for the train split,
ShortSideScale(256) / CenterCrop(224) otherwise, then Normalize(0.45, 0.225) on the raw 0..255 values:
the reference's dataset never divides by 255 (its inference script does).  Item: (clip f32
[3, sequence_length, 224, 224] on the GPU, label f32 scalar); torch's default collate, as the reference
passes none."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from .. import sampling, video_io
from ._device import DeviceClipLoader
from ._span import SpanVideoDataset

__all__ = ["VideoDataset", "create_dataloaders", "CLASS_NAMES"]

CLASS_NAMES = ["non_referral", "referral"]


class VideoDataset(SpanVideoDataset):
    def __init__(self, root_dir, split="train", sampling_method="uniform", sequence_length=32, transform=None,
                 logger=None):
        super().__init__(root_dir, split, sampling_method, sequence_length, 30, 0.5, logger, None)
        self.root_dir = Path(root_dir)
        self.split = split
        self.sequence_length = sequence_length
        # optional callable on {"video": f32 [3, F, H, W] (device, 0..255)} replacing the default chain
        self.custom_transform = transform
        self._sampler = sampling.LstmSampler(sequence_length, sampling_method, self.logger)
        self._setup_data_paths()

    def _setup_data_paths(self):
        self.video_paths, self.labels = [], []
        for label, name in enumerate(CLASS_NAMES):  # non_referral first (dataset.py:41-51)
            class_path = self.root_dir / self.split / name
            if class_path.exists():
                # the reference globs *.mp4; the build also reads its raw .npy clips and frame dirs
                for video_path in video_io.list_videos(class_path):
                    self.video_paths.append(str(video_path))
                    self.labels.append(label)
        self.logger.info(f"Found {len(self.video_paths)} videos for {self.split} split")
        self.logger.info(f"Class distribution: {sum(self.labels)} referral, "
                         f"{len(self.labels) - sum(self.labels)} non-referral")

    def get_sampling_indices(self, video_path, total_frames):
        """dataset.py:85-163."""
        return self._sampler.get_sampling_indices(video_path, total_frames)

    def _indices(self, video_path, src):
        return self.get_sampling_indices(video_path, src.total_frames)

    def _clip_window(self, src, frame_indices):
        duration = (src.total_frames / src.fps if src.fps > 0 else 0.0) or 10.0
        timestamps = sorted(i / self.fps for i in frame_indices)
        return max(0, timestamps[0] - 0.01), min(duration, timestamps[-1] + 0.1)

    def transform_span(self, frames, label):
        from .. import preprocess as pp
        if not torch.cuda.is_available():
            raise RuntimeError("vclip_amd: the clip transform runs on the GPU (MI355X); no CPU path")
        dev = torch.device("cuda", torch.cuda.current_device())
        fr = torch.from_numpy(np.ascontiguousarray(frames)).to(dev).unsqueeze(0)
        if self.custom_transform is not None:
            clip = self.custom_transform({"video": fr[0].permute(3, 0, 1, 2).float()})["video"]
            if clip.shape[1] > self.sequence_length:  # dataset.py:211-213
                idx = pp.uniform_temporal_subsample_indices(clip.shape[1], self.sequence_length).to(clip.device)
                clip = clip.index_select(1, idx)
        elif self.split == "train":
            clip = pp.video_train_transform(fr, self.sequence_length)[0][0]
        else:
            clip = pp.video_eval_transform(fr, self.sequence_length)[0]
        return clip, torch.tensor(label, dtype=torch.float32)


def create_dataloaders(args, logger, splits=("train", "val", "test")):
    """(datasets, dataloaders) of resnet50-2d-lstm/main.py:115-170: train shuffled, train and val with
    drop_last, test neither; `args.test_dir` (or `args.data_dir`) holds the test split."""
    datasets, dataloaders = {}, {}
    for split in splits:
        root = (args.test_dir or args.data_dir) if split == "test" else args.data_dir
        datasets[split] = VideoDataset(root_dir=root, split=split, sampling_method=getattr(args, f"{split}_sampling"),
                                       sequence_length=args.sequence_length, logger=logger)
        dataloaders[split] = DeviceClipLoader(datasets[split], batch_size=args.batch_size, shuffle=(split == "train"),
                                              num_workers=args.num_workers, drop_last=(split != "test"))
    return datasets, dataloaders
