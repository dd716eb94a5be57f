"""The reference's per-folder CLIs on libvclip: `<folder>/main.py` (train + test evaluation) and
`<folder>/inference.py` (one video), same flags, same outputs.

  vivit_transformer/main.py          vivit_main        (train: the HIP train step, §8 a16)
  vivit_transformer/inference.py     vivit_inference
  timesformer/main.py, inference.py  timesformer_main / timesformer_inference
  videoswintransformer/...           swin_main / swin_inference
  resnet50-3d-video/...              resnet3d_main / resnet3d_inference
  resnet50-2d-lstm/...               run_main_lstm / run_inference_lstm: that folder's own flags, loop and
                                     outputs (the last section of this file); inference over a directory
                                     of videos, several per forward (VideoResNet50LSTM.forward_ragged)

Launchers with the reference's folder layout live in `cli/<folder>/{main,inference}.py`.
Sampling is the bit-exact host sampler of each folder (vclip_amd.sampling); decode is host work
(vclip_amd.video_io); preprocessing and the model run on the GPU.  Outputs follow the reference:
`<log_dir>/<prefix>-YYYYmmdd_HHMMSS/` with `experiment.log`, `test_metrics_<method>.json`
(evaluator.py:99-120, metric keys of :257-401), best checkpoint dicts (trainer.py:291-305), and
`inference_results/<video>_result.json` (vivit_transformer/inference.py:225-248).
Only ViViT has a GPU backward; the other families' main.py evaluates a
checkpoint (`--skip_train` / `--checkpoint_path`, as resnet50-3d-video/main.py:53-56 offers) and
refuses to train rather than fall back to a CPU path.
"""
from __future__ import annotations

import argparse
import json
import logging
import random
import time
from datetime import datetime
from pathlib import Path

import numpy as np
import torch

from . import sampling, video_io

SAMPLING = ["random", "uniform", "random_window"]


# ------------------------------------------------------------------------- logging / bookkeeping
class ExperimentLogger:
    """Timestamped experiment dir with file + console handlers (vivit utils/logger.py:8-41)."""

    def __init__(self, log_dir, prefix="vivit-classifier"):
        self.exp_dir = Path(log_dir) / f"{prefix}-{datetime.now().strftime('%Y%m%d_%H%M%S')}"
        self.exp_dir.mkdir(parents=True, exist_ok=True)
        self.logger = logging.getLogger(f"{prefix}-{id(self)}")
        self.logger.setLevel(logging.INFO)
        self.logger.propagate = False
        fmt = logging.Formatter("%(asctime)s - %(levelname)s - %(message)s")
        for h in (logging.FileHandler(self.exp_dir / "experiment.log"), logging.StreamHandler()):
            h.setFormatter(fmt)
            self.logger.addHandler(h)

    def get_logger(self):
        return self.logger

    def get_experiment_dir(self):
        return self.exp_dir


def split_dir(root, mode):
    """The reference's data-dir resolution (vivit dataset.py:23-31)."""
    root = Path(root)
    if not (root / "dataset").exists():
        if (root / mode).exists():
            return root / mode
        return root / "dataset" / mode
    return root / "dataset" / mode


def scan_split(root, mode, logger):
    """(video paths, labels, class labels): class folders sorted by name (dataset.py:74-112)."""
    d = split_dir(root, mode)
    if not d.exists():
        raise FileNotFoundError(f"Data directory not found: {d}")
    classes = sorted(p.name for p in d.iterdir() if p.is_dir())
    paths, labels = [], []
    for ci, c in enumerate(classes):
        vids = video_io.list_videos(d / c)
        logger.info(f"Found {len(vids)} valid videos in class '{c}'")
        paths += vids
        labels += [ci] * len(vids)
    logger.info(f"Total videos for {mode}: {len(paths)}")
    return paths, labels, classes


def compute_metrics(labels, preds, probs, class_names):
    """evaluator.py:257-401 (binary: accuracy, confusion matrix, f1 / precision / recall,
    specificity, auroc + ROC / PR curves, optimal / best-F1 thresholds)."""
    from sklearn.metrics import (accuracy_score, average_precision_score, confusion_matrix, f1_score,
                                 precision_recall_curve, precision_score, recall_score, roc_auc_score, roc_curve)
    labels, preds, probs = np.asarray(labels), np.asarray(preds), np.asarray(probs)
    m = {}
    if len(labels) == 0:
        return dict(accuracy=0.0, f1_score=0.0, auroc=0.0, confusion_matrix=[])
    m["accuracy"] = float(accuracy_score(labels, preds))
    cm = confusion_matrix(labels, preds, labels=list(range(len(class_names))))
    m["confusion_matrix"] = cm.tolist()
    if len(class_names) == 2:
        m["f1_score"] = float(f1_score(labels, preds, zero_division=0))
        m["precision"] = float(precision_score(labels, preds, zero_division=0))
        m["recall"] = float(recall_score(labels, preds, zero_division=0))
        tn, fp = cm[0, 0], cm[0, 1]
        m["specificity"] = float(tn / (tn + fp)) if tn + fp > 0 else 0.0
        if len(np.unique(labels)) > 1:
            m["auroc"] = float(roc_auc_score(labels, probs[:, 1]))
            fpr, tpr, thr = roc_curve(labels, probs[:, 1])
            m["roc_curve"] = {"fpr": fpr.tolist(), "tpr": tpr.tolist(), "thresholds": thr.tolist()}
            m["optimal_threshold"] = float(thr[int(np.argmax(tpr - fpr))])
            pr, rc, pthr = precision_recall_curve(labels, probs[:, 1])
            m["pr_curve"] = {"precision": pr.tolist(), "recall": rc.tolist(), "thresholds": pthr.tolist()}
            m["average_precision"] = float(average_precision_score(labels, probs[:, 1]))
            f1s = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(pr[:-1], rc[:-1])]
            if f1s:
                m["best_f1_threshold"] = float(pthr[int(np.argmax(f1s))])
        else:
            m["auroc"] = 0.0
    else:
        m["f1_score"] = float(f1_score(labels, preds, average="weighted", zero_division=0))
    return m


class EarlyStopping:
    """utils/early_stopping.py:4-56: stop after `patience` epochs without a val-loss decrease of
    more than `delta`; checkpoint on every improvement."""

    def __init__(self, patience=7, delta=0.0, path="checkpoint.pt", logger=None):
        self.patience, self.delta, self.path, self.logger = patience, delta, path, logger
        self.counter, self.best_score, self.early_stop = 0, None, False

    def __call__(self, val_loss, save_fn):
        score = -val_loss
        if self.best_score is None or score >= self.best_score + self.delta:
            self.best_score = score
            save_fn(self.path)
            self.counter = 0
        else:
            self.counter += 1
            if self.counter >= self.patience:
                self.early_stop = True


# ------------------------------------------------------------------------- families
class Family:
    """What differs between the four folders: factory, sampler, decode span, GPU transform."""

    def __init__(self, name, prefix, model_dir, batch_size, epochs, lr, wd, optimizer):
        self.name, self.prefix, self.model_dir = name, prefix, model_dir
        self.batch_size, self.epochs, self.lr, self.wd, self.optimizer = batch_size, epochs, lr, wd, optimizer

    def load_clip(self, src, sampler, path, num_frames, want_indices=False):
        """Decoded uint8 frames the transform consumes: the sampled frames (ViViT/TimeSformer,
        resized to 224 as dataset.py:271-277), or every frame of the sampled span (Swin/ResNet3D
        `get_clip(idx0/fps, (idxN+1)/fps)`, then UniformTemporalSubsample on the GPU).
        want_indices: also the source-frame index of each frame the model sees (ViViT/TimeSformer: of each returned
        frame; Swin/ResNet3D: of the num_frames the subsample keeps of the span)."""
        idx = sampler.get_sampling_indices(str(path), src.total_frames)
        if isinstance(idx, tuple):
            idx = idx[0]
        if self.name in ("vivit", "timesformer"):
            fr = src.read(idx)  # resized to 224x224 on the GPU (to_model_input), as dataset.py:271-277
            used = [min(int(i), src.total_frames - 1) for i in idx][:len(fr)]  # read() clamps to the last frame
            if len(fr) < num_frames:  # pad by repeating the last frame (dataset.py:256-265)
                used += used[-1:] * (num_frames - len(fr))
                fr = np.concatenate([fr, np.repeat(fr[-1:], num_frames - len(fr), 0)])
            return (fr[:num_frames], used[:num_frames]) if want_indices else fr[:num_frames]
        lo, hi = int(min(idx)), int(max(idx))
        fr = src.read(list(range(lo, hi + 1)))
        if want_indices:  # the frames of the span that UniformTemporalSubsample keeps (to_model_input)
            from .preprocess import uniform_temporal_subsample_indices
            keep = uniform_temporal_subsample_indices(len(fr), num_frames)
            return fr, [min(lo + int(i), src.total_frames - 1) for i in keep]
        return fr

    def to_model_input(self, frames_u8: torch.Tensor, num_frames, div255=False, train=False):
        """train: the Swin / ResNet3D train chain (RandomShortSideScale, RandomCrop, RandomHorizontalFlip;
        dataset.py:151-163 / :176-182) instead of the eval chain; ViViT / TimeSformer have one chain."""
        from . import preprocess as pp
        if self.name in ("vivit", "timesformer") and tuple(frames_u8.shape[-3:-1]) != (224, 224):
            frames_u8 = pp.cv2_resize_u8(frames_u8, (224, 224))  # cv2.resize INTER_LINEAR (dataset.py:271-277)
        if self.name == "vivit":
            return pp.vivit_preprocess(frames_u8)
        if self.name == "timesformer":
            return pp.timesformer_preprocess(frames_u8)
        if train:
            return pp.video_train_transform(frames_u8, num_frames, div255=div255)[0]
        return pp.video_eval_transform(frames_u8, num_frames, div255=div255)

    def create_model(self, args, class_labels, device, logger):
        if self.name == "vivit":
            from .vivit import create_model
            return create_model(args.model_name, args.num_classes, class_labels, args.num_frames, device, logger)
        if self.name == "timesformer":
            from .timesformer import create_model
            return create_model(args.model_name, args.num_classes, class_labels, args.num_frames, device, logger)
        if self.name == "swin":
            from .swin3d import create_model
            return create_model(logger, args.model_size, getattr(args, "pretrained", True), args.num_classes, device=device)
        from .resnet3d import create_model
        return create_model(logger, device=device)

    def logits(self, model, x):
        if self.name in ("vivit", "timesformer"):
            return model(pixel_values=x).logits
        return model(x)


FAMILIES = {
    "vivit": Family("vivit", "vivit-classifier", "vivit-models", 4, 40, 1e-3, 0.01, "adamw"),
    "timesformer": Family("timesformer", "timesformer-classifier", "timesformer-models", 4, 40, 1e-3, 0.01, "adamw"),
    "swin": Family("swin", "swin3d-classifier", "swin-models", 8, 30, 1e-4, 0.05, "adamw"),
    "resnet3d": Family("resnet3d", "resnet3d-classifier", "resnet3d-models", 8, 30, 1e-3, 0.0, "adam"),
    # resnet50-2d-lstm: its own flags, loop and outputs (build_parser_lstm, run_main_lstm, run_inference_lstm)
    "lstm": Family("lstm", "resnet50_lstm_enhanced", "models", 4, 30, 1e-3, 0.0, "adam"),
}


VIVIT_SALIENCY_HELP = (
    "absent (default): the label only, as the reference.  rollout: attention rollout of the CLS token over every "
    "layer (VivitForVideoClassification.explain); cls_attention: the last layer's head-mean CLS attention; "
    "grad_rollout: the class-specific gradient-weighted rollout (Chefer et al. 2021) for --saliency_class.  Writes "
    "<video>_saliency.npy (f32 [T/kt, H/kh, W/kw], sums to 1) beside the result JSON, which gains a \"saliency\" "
    "object with each tubelet's importance and the source-frame indices it covers.")


TIMESFORMER_SALIENCY_HELP = (
    "absent (default): the label only, as the reference.  rollout: attention rollout of the CLS token through the "
    "divided space-time attention of every layer (TimesformerForVideoClassification.explain); cls_attention: the last "
    "layer's head-mean spatial CLS attention.  Writes <video>_saliency.npy (f32 [T, H/ps, W/ps], sums to 1) beside the "
    "result JSON, which gains a \"saliency\" object with each frame's importance and its source-frame index.")
SWIN_SALIENCY_HELP = (
    "absent (default): the label only, as the reference.  rollout: attention rollout from the pooled tokens back "
    "through every block's shifted-window attention and every PatchMerging (Swin3d.explain).  Writes "
    "<video>_saliency.npy (f32 [T/2, H/4, W/4], sums to 1) beside the result JSON, which gains a \"saliency\" object "
    "with each time step's importance and the two source-frame indices it covers.  class_rollout: the class-specific "
    "gradient-weighted rollout (Chefer et al. 2021) through the same blocks (Swin3d.explain_class) for "
    "--saliency_class; the \"saliency\" object then names target_class / target_label.")


RESNET3D_SALIENCY_HELP = (
    "absent (default): the label only, as the reference.  gradcam: Grad-CAM (Selvaraju et al. 2017); hirescam: HiResCAM "
    "(Draelos & Carin 2020), the gradient times the activation per position (ResNet3d.explain), for --saliency_class at "
    "--saliency_layer.  Writes <video>_saliency.npy (f32 [T, H/32, W/32] at res5, [T, H/16, W/16] at res4; the positive "
    "part of the map, sums to 1, or all zero when the map has nothing positive) beside the result JSON, which gains a "
    "\"saliency\" object with each frame's importance and its source-frame index.")
SALIENCY_CHECK_HELP = (
    "with --saliency: score the map with the perturbation test (vclip_amd.faithfulness) in STEPS steps: the class score "
    "as the map's cells are deleted from the clip and inserted into a zero clip in the map's order, and deleted in a "
    "random order.  The result JSON's \"saliency\" object gains a \"faithfulness\" object with the three curves and "
    "their areas (deletion_gain = random_deletion_auc - deletion_auc: positive when the map beats chance).")
RISE_SALIENCY_HELP = (
    "  rise: RISE (Petsiuk et al. 2018), the class-specific black-box map at pixel resolution (vclip_amd.rise_map): the "
    "score-weighted mean of --rise_masks smooth random masks, for --saliency_class; <video>_saliency.npy is then f32 "
    "[T, H, W] and the \"saliency\" object names masks, cells, keep and seed.")
# per family: the --saliency methods that take --saliency_class
CLASS_SPECIFIC_SALIENCY = {"vivit": ("grad_rollout", "rise"), "timesformer": ("rise",), "swin": ("rise", "class_rollout"),
                           "resnet3d": ("gradcam", "hirescam", "rise")}


def _positive_int(text: str) -> int:
    v = int(text)  # a ValueError is argparse's "invalid value"
    if v < 1:
        raise argparse.ArgumentTypeError(f"{text}: must be at least 1")
    return v


class _SaliencyCheckParser(argparse.ArgumentParser):
    """The inference parser as run_inference builds it: --saliency_check without --saliency is an error, and so is
    TimeSformer's and Swin's --saliency_class with a method that is not class-specific (`class_methods`, set by
    build_parser for those two; ViViT's and ResNet3D's is checked by run_inference, as before)"""
    class_methods = None

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if getattr(a, "saliency_check", None) is not None and getattr(a, "saliency", None) is None:
            self.error("--saliency_check needs --saliency")
        if (self.class_methods is not None and getattr(a, "saliency_class", None) is not None
                and getattr(a, "saliency", None) not in self.class_methods):
            self.error(f"--saliency_class needs --saliency {' or '.join(self.class_methods)}")
        return a


def _temporal_patch(model) -> int:
    """sampled frames per time step of the family's saliency map: ViViT's tubelet depth, Swin's patch_size[0],
    1 for TimeSformer (per-frame patches)"""
    cfg = getattr(model, "config", None)
    if cfg is not None and hasattr(cfg, "tubelet_size"):
        return int(cfg.tubelet_size[0])
    if isinstance(getattr(model, "cfg", None), dict) and "patch_size" in model.cfg:
        return int(model.cfg["patch_size"][0])
    return 1


def build_parser(fam: Family, inference: bool, saliency: bool = False):
    """The folder's reference flags (plus ViViT's --saliency / --saliency_class).  saliency=True, as run_inference
    builds it: the TimeSformer, Swin and ResNet3D inference parsers also get their own --saliency (ResNet3D's with
    --saliency_class and --saliency_layer), and all four the method `rise` with --rise_masks and --rise_seed (and
    TimeSformer and Swin the --saliency_class that only `rise` and Swin's `class_rollout` take); the two-argument form keeps the flag surface
    those families had before their `explain` existed."""
    if fam.name == "lstm":
        return build_parser_lstm(inference)
    cls = _SaliencyCheckParser if inference and saliency else argparse.ArgumentParser
    p = cls(description=f"{fam.name} video classifier (libvclip, MI355X)")
    if inference:
        p.add_argument("--video_path", type=str, required=True)
        p.add_argument("--model_path", type=str, required=True)
        p.add_argument("--log_dir", type=str, default="logs")
        p.add_argument("--num_frames", type=int, default=32)
        p.add_argument("--sampling_method", type=str, default="uniform", choices=SAMPLING)
        if fam.name != "resnet3d":
            p.add_argument("--num_classes", type=int, default=2)
        if fam.name == "swin":
            p.add_argument("--model_size", type=str, default="tiny", choices=["tiny", "small", "base", "base_in22k"])
        if fam.name in ("vivit", "timesformer"):
            p.add_argument("--save_viz", action="store_true")
        else:
            p.add_argument("--visualize", action="store_true")
        rise = ["rise"] if saliency else []
        more = RISE_SALIENCY_HELP if saliency else ""
        if fam.name == "vivit":
            # not in the reference, whose HF model can return its attentions: which tubelets produced the label
            p.add_argument("--saliency", type=str, default=None,
                           choices=["rollout", "cls_attention", "grad_rollout"] + rise, help=VIVIT_SALIENCY_HELP + more)
            p.add_argument("--saliency_class", type=int, default=None,
                           help="with --saliency grad_rollout: the class index whose evidence is mapped (absent: the "
                                "predicted class); the result JSON's \"saliency\" object names it as target_class / "
                                "target_label")
        elif fam.name in ("timesformer", "swin") and saliency:
            own = ["rollout", "cls_attention"] if fam.name == "timesformer" else ["rollout", "class_rollout"]
            p.add_argument("--saliency", type=str, default=None, choices=own + rise,
                           help=(TIMESFORMER_SALIENCY_HELP if fam.name == "timesformer" else SWIN_SALIENCY_HELP) + more)
            p.add_argument("--saliency_class", type=int, default=None,
                           help=f"with --saliency {' or '.join(CLASS_SPECIFIC_SALIENCY[fam.name])}: the class index whose "
                                "evidence is mapped (absent: the predicted class); the result JSON's \"saliency\" object "
                                "names it as target_class / target_label")
            p.class_methods = CLASS_SPECIFIC_SALIENCY[fam.name]
        elif fam.name == "resnet3d" and saliency:
            p.add_argument("--saliency", type=str, default=None, choices=["gradcam", "hirescam"] + rise,
                           help=RESNET3D_SALIENCY_HELP + more)
            p.add_argument("--saliency_class", type=int, default=None,
                           help="with --saliency: the class index whose evidence is mapped (absent: the predicted "
                                "class); the result JSON's \"saliency\" object names it as target_class / target_label")
            p.add_argument("--saliency_layer", type=str, default="res5", choices=["res5", "res4"],
                           help="with --saliency: the stage whose output is explained (res4: twice the spatial "
                                "resolution, through the res5 data-gradient chain)")
        if saliency:
            p.add_argument("--rise_masks", type=_positive_int, default=4000, metavar="N",
                           help="with --saliency rise: the number of random masks, one forward each (4000: the paper's)")
            p.add_argument("--rise_seed", type=int, default=0, help="with --saliency rise: the seed of the mask sampler")
            p.add_argument("--saliency_check", type=_positive_int, default=None, metavar="STEPS",
                           help=SALIENCY_CHECK_HELP)
        return p
    required = fam.name in ("swin", "resnet3d")
    p.add_argument("--data_dir", type=str, required=True)
    p.add_argument("--test_data_dir", type=str, default=None)
    p.add_argument("--log_dir", type=str, default=None if required else "logs", required=required)
    p.add_argument("--model_dir", type=str, default=None if required else fam.model_dir, required=required)
    for s in ("train", "val", "test"):
        p.add_argument(f"--{s}_sampling", type=str, default="uniform", choices=SAMPLING)
    p.add_argument("--num_frames", type=int, default=32)
    if fam.name == "vivit":
        p.add_argument("--model_name", type=str, default="google/vivit-b-16x2-kinetics400")
    elif fam.name == "timesformer":
        p.add_argument("--model_name", type=str, default="facebook/timesformer-base-finetuned-k400")
    elif fam.name == "swin":
        p.add_argument("--model_size", type=str, default="tiny", choices=["tiny", "small", "base", "base_in22k"])
        p.add_argument("--pretrained", action="store_true")
    if fam.name != "resnet3d":
        p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--batch_size", type=int, default=fam.batch_size)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--epochs", type=int, default=fam.epochs)
    p.add_argument("--learning_rate", type=float, default=fam.lr)
    if fam.name != "resnet3d":
        p.add_argument("--weight_decay", type=float, default=fam.wd)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--patience", type=int, default=7)
    p.add_argument("--early_stopping_delta", type=float, default=0.001)
    # resnet50-3d-video/main.py:53-58, offered by every family here (evaluate a checkpoint, no training)
    p.add_argument("--skip_train", action="store_true")
    p.add_argument("--checkpoint_path", type=str, default=None)
    if fam.name == "resnet3d":
        p.add_argument("--weighted_sampling", action="store_true")
    if fam.name == "vivit":
        # not in the reference: LoRA fine-tuning (vclip_amd/lora.py) -- the base frozen, rank-R adapters trained
        p.add_argument("--lora_rank", type=int, default=0, metavar="R",
                       help="train rank-R LoRA adapters (and the classifier) on a frozen base instead of every weight "
                            "(0: off); the checkpoint's model_state_dict has them folded in")
        p.add_argument("--lora_alpha", type=float, default=None, metavar="A", help="LoRA scale alpha (absent: 2R)")
        p.add_argument("--lora_targets", type=str, default="q,v",
                       help="comma-separated projections that get adapters, out of q,k,v,o,fc1,fc2")
        p.add_argument("--lora_layers", type=int, default=0, metavar="N",
                       help="adapters on the last N encoder layers only (0: all)")
    return p


def _device():
    import os
    if not torch.cuda.is_available():
        raise RuntimeError("vclip_amd runs on the GPU only (MI355X); no CPU execution path")
    return torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))


def _loaders(fam, args, logger, exp_dir):
    """({split: loader}, class labels) from the folder's own data_config drop-in, so `--num_workers`
    decode workers run as in the reference (vivit_transformer/main.py:93, videoswintransformer/
    main.py:105, resnet50-3d-video/main.py:94-97 with the sampled-index CSVs in the experiment dir).
    `--skip_train` builds the test split only (resnet50-3d-video/main.py:53-58 evaluates a checkpoint)."""
    from torch.utils.data import DataLoader

    from .data_config import FOLDERS, DeviceClipLoader, swin
    mod = FOLDERS[fam.name]
    methods = {s: getattr(args, f"{s}_sampling") for s in ("train", "val", "test")}
    hf = fam.name in ("vivit", "timesformer")
    binary = ["non-referral", "referral"]  # Swin3D / ResNet3D label = (folder == 'referral')
    if not args.skip_train:
        if hf:
            return mod.create_dataloaders(args, methods, logger)
        if fam.name == "swin":
            return mod.create_dataloaders(args, logger), binary
        return mod.create_dataloaders(args, logger, log_dir=str(exp_dir))[1], binary
    if fam.name == "resnet3d":
        # resnet50-3d-video/main.py:94-98 builds every split with the experiment dir before it looks
        # at --skip_train, so the sampled-index CSVs (its only golden artefact) are written for train,
        # val and test; a dataset without train/val splits still gets its test CSV
        try:
            return {"test": mod.create_dataloaders(args, logger, log_dir=str(exp_dir))[1]["test"]}, binary
        except Exception as e:  # noqa: BLE001 - the reference raises here; evaluating the test split is still possible
            logger.warning(f"create_dataloaders failed ({e}); building the test split only")
            ds = mod.VideoDataset(args.test_data_dir or args.data_dir, mode="test", sampling_method=methods["test"],
                                  num_frames=args.num_frames, logger=logger, log_dir=str(exp_dir))
            ds.save_sampled_indices()
            return {"test": DeviceClipLoader(ds, batch_size=args.batch_size, num_workers=args.num_workers,
                                             collate_fn=swin.video_collate_fn)}, binary
    root = args.test_data_dir or args.data_dir
    ds = mod.VideoDataset(root, mode="test", sampling_method=methods["test"], num_frames=args.num_frames,
                          logger=logger)
    if hf:
        loader = DataLoader(ds, batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers,
                            collate_fn=mod.video_collate_fn)
        return {"test": loader}, ds.class_labels
    return {"test": DeviceClipLoader(ds, batch_size=args.batch_size, num_workers=args.num_workers,
                                     collate_fn=swin.video_collate_fn)}, binary


def _batches(fam, loader, args, device):
    """(model input, labels) on the device per loader batch: the HF folders' uint8 clips through the
    GPU processor (trainer.py:62-104), the Swin3D / ResNet3D clips [B, n, C, T, H, W] flattened to
    [B * n, C, T, H, W] (videoswintransformer/.../trainers/trainer.py:105-111)."""
    for batch in loader:
        if isinstance(batch, dict):
            pv = batch["pixel_values"]
            fr = torch.from_numpy(np.stack(pv)) if isinstance(pv, (list, tuple)) else torch.as_tensor(pv)
            x = fam.to_model_input(fr.to(device), args.num_frames)
            yield x, batch["labels"].reshape(-1).to(device)
        else:
            clips, labels = batch
            yield clips.reshape(-1, *clips.shape[2:]).to(device), labels.reshape(-1).to(device)


def _load_weights(model, path, logger, fam):
    from .checkpoint import load_reference_checkpoint
    ck, sd = load_reference_checkpoint(path, vivit_keys=fam.name == "vivit")
    model.load_state_dict(sd)
    logger.info(f"Loaded weights from {path}")
    return ck


@torch.no_grad()
def evaluate(fam, model, loader, args, device, class_names, exp_dir, method, logger):
    model.eval()
    probs, preds, labels = [], [], []
    for x, y in _batches(fam, loader, args, device):
        try:
            p = torch.softmax(fam.logits(model, x).float(), dim=1)
        except Exception as e:  # noqa: BLE001 - evaluator.py: log and skip the batch
            logger.error(f"Error in test batch: {str(e)}")
            continue
        probs.append(p.cpu().numpy())
        preds += p.argmax(1).tolist()
        labels += y.tolist()
    probs = np.concatenate(probs) if probs else np.zeros((0, len(class_names)))
    m = compute_metrics(labels, preds, probs, class_names)
    with open(Path(exp_dir) / f"test_metrics_{method}.json", "w") as f:
        json.dump(m, f, indent=4)
    logger.info(f"Test accuracy {m['accuracy']:.4f}  F1 {m.get('f1_score', 0):.4f}  AUROC {m.get('auroc', 0):.4f}")
    return m


def run_main(fam_name, argv=None):
    if fam_name == "lstm":
        return run_main_lstm(argv)
    fam = FAMILIES[fam_name]
    args = build_parser(fam, inference=False).parse_args(argv)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    exp = ExperimentLogger(args.log_dir, prefix=fam.prefix)
    logger = exp.get_logger()
    logger.info(f"Arguments: {vars(args)}")
    device = _device()
    loaders, class_labels = _loaders(fam, args, logger, exp.get_experiment_dir())
    if not hasattr(args, "num_classes"):
        args.num_classes = len(class_labels)
    model = fam.create_model(args, class_labels, device, logger)
    if args.checkpoint_path:
        _load_weights(model, args.checkpoint_path, logger, fam)
    use_lora = fam.name == "vivit" and getattr(args, "lora_rank", 0) > 0 and not args.skip_train
    if use_lora:
        from . import lora
        lora.attach(model, rank=args.lora_rank, alpha=2.0 * args.lora_rank if args.lora_alpha is None else args.lora_alpha,
                    targets=args.lora_targets, layers=args.lora_layers or None, seed=args.seed)
        logger.info(f"LoRA: {lora.state_dict(model)['lora_config']}, {lora.trainable_parameters(model)} trainable "
                    f"parameters")
    history = {"train_loss": [], "train_acc": [], "val_loss": [], "val_acc": []}
    if not args.skip_train:
        from .optim import AdamW
        # ResNet3D: torch.optim.Adam(model.parameters(), lr) (resnet50-3d-video/main.py:153) = AdamW with
        # weight decay 0; its BatchNorm running statistics carry no gradient and are skipped
        opt = AdamW([q for q in model.parameters() if q.requires_grad], lr=args.learning_rate,
                    weight_decay=getattr(args, "weight_decay", 0.0))
        crit = torch.nn.CrossEntropyLoss()
        model_dir = Path(args.model_dir)
        model_dir.mkdir(parents=True, exist_ok=True)
        best_path = model_dir / f"best_model_{args.train_sampling}.pth"
        stopper = EarlyStopping(args.patience, args.early_stopping_delta, exp.get_experiment_dir() / "checkpoint.pt")
        best_val = float("inf")
        for epoch in range(args.epochs):
            model.train()
            tl, tc, tn = 0.0, 0, 0
            for x, y in _batches(fam, loaders["train"], args, device):
                try:  # trainer.py:133-167: a failing batch is logged and skipped
                    opt.zero_grad()
                    logits = fam.logits(model, x)
                    loss = crit(logits, y)
                    loss.backward()
                    opt.step()
                    tl += loss.item() * len(y)
                    tc += int((logits.argmax(1) == y).sum())
                    tn += len(y)
                except Exception as e:  # noqa: BLE001
                    logger.error(f"Error in training batch: {str(e)}")
                    continue
            model.eval()
            vl, vc, vn = 0.0, 0, 0
            with torch.no_grad():
                for x, y in _batches(fam, loaders["val"], args, device):
                    try:  # trainer.py:192-210
                        logits = fam.logits(model, x)
                        vl += float(crit(logits, y)) * len(y)
                        vc += int((logits.argmax(1) == y).sum())
                        vn += len(y)
                    except Exception as e:  # noqa: BLE001
                        logger.error(f"Error in validation batch: {str(e)}")
                        continue
            # a batch that fails is logged and skipped (trainer.py:165-167), but an epoch in which EVERY
            # batch failed (e.g. a kernel fault on each launch) must not go on to save a "best" model
            if tn == 0 and len(loaders["train"]) > 0:
                raise RuntimeError(f"epoch {epoch + 1}: every training batch failed (see the log)")
            if vn == 0 and len(loaders["val"]) > 0:
                raise RuntimeError(f"epoch {epoch + 1}: every validation batch failed (see the log)")
            tr_loss, tr_acc = tl / max(tn, 1), tc / max(tn, 1)
            va_loss, va_acc = vl / max(vn, 1), vc / max(vn, 1)
            for k, v in (("train_loss", tr_loss), ("train_acc", tr_acc), ("val_loss", va_loss), ("val_acc", va_acc)):
                history[k].append(v)
            logger.info(f"Epoch {epoch + 1}/{args.epochs}: train loss {tr_loss:.4f} acc {tr_acc:.4f} | "
                        f"val loss {va_loss:.4f} acc {va_acc:.4f}")

            def save(path, epoch=epoch, va_loss=va_loss, va_acc=va_acc):
                ck = {"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": opt.state_dict(),
                      "val_loss": va_loss, "val_acc": va_acc, "history": history}
                if hasattr(model, "config"):  # HF families: vivit trainer.py:291-305 (and TimeSformer's)
                    ck.update({"config": model.config.to_dict(), "id2label": model.config.id2label,
                               "label2id": model.config.label2id, "num_frames": args.num_frames,
                               "train_sampling": args.train_sampling, "val_sampling": args.val_sampling,
                               "test_sampling": args.test_sampling})
                if use_lora:  # the adapters folded in: inference.py and --checkpoint_path read it as any checkpoint
                    ck["model_state_dict"] = lora.merged_state_dict(model)
                    ck["lora_state_dict"] = lora.state_dict(model)
                    ck["lora_config"] = ck["lora_state_dict"]["lora_config"]
                # (Swin3D: videoswintransformer/.../trainers/trainer.py:191-198 saves the six keys above)
                torch.save(ck, path)

            if va_loss < best_val:  # trainer.py:231-236 + _save_best_model
                best_val = va_loss
                save(best_path)
                logger.info(f"Saved best model to {best_path}")
            stopper(va_loss, save)
            if stopper.early_stop:
                logger.info("Early stopping triggered")
                break
        if use_lora:
            lora.detach(model)  # the best checkpoint's weights already hold its adapters
        _load_weights(model, best_path, logger, fam)
    m = evaluate(fam, model, loaders["test"], args, device, class_labels, exp.get_experiment_dir(),
                 args.test_sampling, logger)
    logger.info("Training and evaluation pipeline completed successfully")
    return m, history, exp.get_experiment_dir()


def run_inference(fam_name, argv=None):
    if fam_name == "lstm":
        return run_inference_lstm(argv)
    fam = FAMILIES[fam_name]
    parser = build_parser(fam, inference=True, saliency=True)
    args = parser.parse_args(argv)
    saliency_class = getattr(args, "saliency_class", None)
    class_methods = CLASS_SPECIFIC_SALIENCY.get(fam.name, ())
    if saliency_class is not None and getattr(args, "saliency", None) not in class_methods:
        parser.error(f"--saliency_class needs --saliency {' or '.join(class_methods)}")
    exp = ExperimentLogger(args.log_dir, prefix=f"{fam.prefix}-inference")
    logger = exp.get_logger()
    device = _device()
    from .checkpoint import load_reference_checkpoint
    ck, sd = load_reference_checkpoint(args.model_path, vivit_keys=fam.name == "vivit")
    id2label = {int(k): v for k, v in (ck.get("id2label") or {0: "non-referral", 1: "referral"}).items()}
    if saliency_class is not None and saliency_class not in id2label:
        parser.error(f"--saliency_class {saliency_class} is not one of the checkpoint's labels {sorted(id2label)}")
    class_labels = [id2label[i] for i in sorted(id2label)]
    args.num_classes = len(class_labels)
    if fam.name in ("vivit", "timesformer"):
        args.model_name = "checkpoint"
        if ck.get("config"):
            cfg = dict(ck["config"])
            if fam.name == "vivit":
                from .vivit import VivitConfig, VivitForVideoClassification
                model = VivitForVideoClassification(VivitConfig.from_dict(cfg)).to(device).eval()
            else:
                from .timesformer import TimesformerConfig, TimesformerForVideoClassification
                model = TimesformerForVideoClassification(TimesformerConfig.from_dict(cfg)).to(device).eval()
        else:
            model = fam.create_model(args, class_labels, device, logger)
    else:
        model = fam.create_model(args, class_labels, device, logger)
    model.load_state_dict(sd)
    model.eval()  # the reference inference scripts' model.eval()
    src = video_io.open_video(args.video_path)
    if fam.name in ("vivit", "timesformer"):
        sampler = sampling.VivitSampler(args.num_frames, args.sampling_method, logger)
    elif fam.name == "swin":
        sampler = _SwinInferenceSampler(args.num_frames, args.sampling_method, logger, src.fps)
    else:
        sampler = sampling.Resnet3dInferenceSampler(args.num_frames, args.sampling_method, logger,
                                                    fps_of=lambda p: src.fps)
    saliency = getattr(args, "saliency", None)
    clip = fam.load_clip(src, sampler, args.video_path, args.num_frames, want_indices=bool(saliency))
    clip, frame_idx = clip if saliency else (clip, None)
    frames = torch.from_numpy(clip).to(device)
    # the Swin / ResNet3D inference scripts divide by 255 before Normalize (resnet50-3d-video/inference.py:382-394)
    x = fam.to_model_input(frames.unsqueeze(0), args.num_frames, div255=True)
    t0 = time.perf_counter()
    with torch.no_grad():
        probs = torch.softmax(fam.logits(model, x).float(), dim=1)
    torch.cuda.synchronize()
    pred = int(probs.argmax(1))
    conf = float(probs[0, pred])
    name = id2label[pred]
    logger.info(f"Prediction: {name}  Confidence: {conf:.4f}  ({(time.perf_counter() - t0) * 1e3:.1f} ms)")
    print(f"Predicted class: {name}")
    print(f"Confidence: {conf:.4f}")
    res = {"video_path": str(args.video_path), "predicted_class": name,
           "class_id": id2label.get(name, -1),  # (sic) the reference looks the name up in id2label: -1
           "confidence": conf, "class_mapping": {str(k): v for k, v in id2label.items()}}
    out = exp.get_experiment_dir() / "inference_results"
    out.mkdir(parents=True, exist_ok=True)
    if saliency:
        # the label above is the ordinary forward's, the same with and without the flag; the map is explain's
        if saliency == "rise":  # black box: the same call for every family, the asked class or the label printed above
            from .rise import rise_map
            ex = rise_map(model, x, target=pred if saliency_class is None else saliency_class, masks=args.rise_masks,
                          seed=args.rise_seed)
        elif fam.name == "resnet3d":
            ex = model.explain(x, method=saliency, target=pred if saliency_class is None else saliency_class,
                               layer=args.saliency_layer)
        elif saliency == "class_rollout":  # Swin's class-specific map: the asked class, or the label printed above
            ex = model.explain_class(x, target=pred if saliency_class is None else saliency_class)
        elif saliency == "grad_rollout":  # class-specific: the asked class, or the label printed above
            ex = model.explain(x, method=saliency, target=pred if saliency_class is None else saliency_class)
        else:
            ex = model.explain(x, method=saliency)
        sal = ex.saliency[0].numpy()
        kt = 1 if saliency == "rise" else _temporal_patch(model)  # RISE's map is per sampled frame
        npy = f"{Path(args.video_path).stem}_saliency.npy"
        np.save(out / npy, sal)
        res["saliency"] = {"method": saliency, "file": npy, "shape": list(sal.shape),
                           "temporal_importance": [float(v) for v in ex.temporal[0]],
                           "tubelet_frame_indices": [frame_idx[i:i + kt] for i in range(0, len(frame_idx), kt)]}
        if ex.target is not None:
            res["saliency"].update(target_class=ex.target[0], target_label=id2label[ex.target[0]])
        if saliency == "rise":
            res["saliency"].update(masks=ex.masks, cells=list(ex.cells), keep=ex.keep, seed=ex.seed)
        elif fam.name == "resnet3d":
            res["saliency"]["layer"] = args.saliency_layer
            if not sal.any():  # the map has nothing positive: no evidence for the class at this layer
                res["saliency"]["empty"] = True
        logger.info(f"Saliency ({saliency}): {out / npy}, most important tubelet {int(ex.temporal[0].argmax())}")
        if args.saliency_check:
            # does the label move when what the map points at is taken away?  scored for the class the map explains
            from .faithfulness import faithfulness
            chk = faithfulness(model, x, ex, steps=args.saliency_check, baseline="zero",
                               target=pred if ex.target is None else ex.target[0])
            areas = {k: float(chk[k][0]) for k in ("deletion_auc", "insertion_auc", "random_deletion_auc", "deletion_gain")}
            res["saliency"]["faithfulness"] = dict(
                steps=chk["steps"], baseline=chk["baseline"], target_class=chk["target"][0], **areas,
                fractions=[float(v) for v in chk["deletion"].fractions],
                **{k: [float(v) for v in chk[k].score[0]] for k in ("deletion", "insertion", "random_deletion")})
            logger.info(f"Saliency check ({args.saliency_check} steps): deletion AUC {areas['deletion_auc']:.4f}, "
                        f"random-order {areas['random_deletion_auc']:.4f}, insertion AUC {areas['insertion_auc']:.4f}")
    with open(out / f"{Path(args.video_path).stem}_result.json", "w") as f:
        json.dump(res, f, indent=4)
    return res


class _SwinInferenceSampler:
    """videoswintransformer/inference.py:94-185 (module function, reseeds 42 per call)."""

    def __init__(self, num_frames, method, logger, fps):
        self.num_frames, self.method, self.logger, self.fps = num_frames, method, logger, fps

    def get_sampling_indices(self, video_path, total_frames):
        return sampling.swin_inference_sampling_indices(video_path, total_frames, self.num_frames, self.method,
                                                        self.logger, fps_of=lambda p: self.fps)


# ------------------------------------------------------------------------- resnet50-2d-lstm
# The fifth folder's application is its own: one logit under BCEWithLogitsLoss(pos_weight), Adam over the
# trainable parameters, ReduceLROnPlateau on the validation AUROC, a composite (loss, AUROC) model
# selection, plain state_dict checkpoints, and an inference script that walks a directory of videos
# (resnet50-2d-lstm/main.py, src/trainer/trainer.py, src/evaluators/evaluator.py, inference.py).
LSTM_SEED = 42  # src/config/config.py:4
LSTM_CLASS_NAMES = ["non_referral", "referral"]
LSTM_HISTORY_KEYS = ("train_loss", "val_loss", "train_acc", "val_acc", "train_auroc", "val_auroc")
# batched ragged inference: the smallest batch within 5 % of the best measured rate, which was the largest
# measured (16 videos per call 2211 videos/s, 8 per call 1907, one at a time 656)
LSTM_VIDEOS_PER_BATCH = 16
LSTM_STREAM_CHUNK_HELP = (
    "0 (default): off, the sampled-frames inference of the reference.  N >= 1: every frame of every video goes "
    "through the model, up to --videos_per_batch videos in lockstep, at most N frames of each per forward_stream "
    "call with the LSTM state carried between calls (--sampling_method and --sequence_length are ignored); also "
    "writes frame_probabilities/<video>.csv.  128 is the smallest chunk within 5 %% of the best measured rate "
    "(4 videos of 256 frames: 41.0k frames/s at 9.2 GB peak; 32: 36.9k at 2.9 GB; 256: 41.9k at 17.1 GB, "
    "DESIGN.md section 5.11).")
LSTM_SALIENCY_HELP = (
    "off by default.  gradcam / hirescam: per-frame Grad-CAM (Selvaraju et al. 2017) or HiResCAM (Draelos & Carin 2020) "
    "on the 2D backbone with the gradient taken through the head and the recurrence by exact BPTT "
    "(VideoResNet50LSTM.explain), for --saliency_class at --saliency_layer; at res5 the two coincide.  Writes "
    "saliency/<video>.npy (f32 [T, 7, 7] at res5, [T, 14, 14] at res4: the positive part of the map divided by its sum, "
    "all zero when nothing is positive) and adds saliency_file, saliency_target and frame_importance (the map summed over "
    "space, aligned with frame_indices) to the video's result row.  With --stream_chunk: whole recordings through the "
    "explain session, no spatial maps; frame_probabilities/<video>.csv gains the columns relevance (the signed gradient x "
    "input of the frame's pooled features) and importance (its positive part divided by the recording's sum).")
LSTM_TBPTT_CHUNK_HELP = (
    "0 (default): off, the reference's training on --sequence_length sampled frames.  N >= 1: training and validation "
    "use every frame of every video; --batch_size videos advance in lockstep, at most N frames of each per round, "
    "with the LSTM state carried between rounds and detached (truncated backpropagation through time: one "
    "backward per round, one optimiser step per batch of videos).  --train_sampling, --val_sampling and "
    "--sequence_length are ignored for training and validation; the backbone's BatchNorm keeps its running "
    "statistics.")


def build_parser_lstm(inference: bool):
    sampling3 = ["uniform", "random", "random_window"]
    if inference:  # resnet50-2d-lstm/inference.py:206-223
        p = argparse.ArgumentParser(description="ResNet50-LSTM inference over a directory of videos (libvclip, MI355X)")
        p.add_argument("--videos_dir", type=str, required=True)
        p.add_argument("--model_path", type=str, required=True)
        p.add_argument("--output_dir", type=str, default="inference_results")
        p.add_argument("--sampling_method", type=str, default="uniform", choices=sampling3)
        p.add_argument("--sequence_length", type=int, default=32)
        p.add_argument("--visualize", action="store_true")
        p.add_argument("--batch_mode", action="store_true")
        p.add_argument("--single_video", type=str, default=None)
        # not in the reference, which runs one video per forward: videos per forward_ragged call
        p.add_argument("--videos_per_batch", type=int, default=LSTM_VIDEOS_PER_BATCH)
        # not in the reference either: whole-video streaming inference (forward_stream with the LSTM state carried)
        p.add_argument("--stream_chunk", type=int, default=0, help=LSTM_STREAM_CHUNK_HELP)
        # not in the reference: which frames, and where in them, produced the prediction (VideoResNet50LSTM.explain)
        p.add_argument("--saliency", type=str, default=None, choices=["gradcam", "hirescam"], help=LSTM_SALIENCY_HELP)
        p.add_argument("--saliency_class", type=int, default=None, choices=[0, 1],
                       help="with --saliency: 1 maps the evidence for referral (+logit), 0 for non_referral (-logit); "
                            "absent: each video's predicted class")
        p.add_argument("--saliency_layer", type=str, default="res5", choices=["res5", "res4"],
                       help="with --saliency and without --stream_chunk: the backbone stage whose output is explained "
                            "(res4: twice the spatial resolution, through the res5 bottlenecks' data gradients)")
        return p
    p = argparse.ArgumentParser(description="ResNet50-LSTM video classification training (libvclip, MI355X)")
    p.add_argument("--data_dir", type=str, default="dataset")  # resnet50-2d-lstm/main.py:22-62
    p.add_argument("--test_dir", type=str, default=None)
    p.add_argument("--log_dir", type=str, default="logs")
    p.add_argument("--model_dir", type=str, default="models")
    for s in ("train", "val", "test"):
        p.add_argument(f"--{s}_sampling", type=str, default="uniform", choices=sampling3)
    p.add_argument("--loss_weight", type=float, default=0.3)
    p.add_argument("--learning_rate", type=float, default=0.001)
    p.add_argument("--batch_size", type=int, default=4)
    p.add_argument("--epochs", type=int, default=30)
    p.add_argument("--patience", type=int, default=10)
    p.add_argument("--hidden_size", type=int, default=256)
    p.add_argument("--num_layers", type=int, default=2)
    p.add_argument("--dropout", type=float, default=0.5)
    p.add_argument("--sequence_length", type=int, default=32)
    p.add_argument("--skip_train", action="store_true")
    p.add_argument("--checkpoint_path", type=str, default=None)
    p.add_argument("--num_workers", type=int, default=2)
    # not in the reference, which trains on --sequence_length sampled frames: truncated BPTT over whole videos
    p.add_argument("--tbptt_chunk", type=int, default=0, help=LSTM_TBPTT_CHUNK_HELP)
    return p


class LstmExperimentLogger:
    """src/utils/logger.py:6-58: the given directory itself is the experiment directory, log file
    `<prefix>.log`."""

    def __init__(self, log_dir, prefix="resnet50-lstm-training"):
        self.exp_dir = Path(log_dir)
        if self.exp_dir.exists() and not self.exp_dir.is_dir():
            raise ValueError(f"Log directory path exists but is not a directory: {log_dir}")
        self.exp_dir.mkdir(parents=True, exist_ok=True)
        self.logger = logging.getLogger(f"ResNet50LSTM-{id(self)}")
        self.logger.setLevel(logging.INFO)
        self.logger.propagate = False
        fh = logging.FileHandler(self.exp_dir / f"{prefix}.log")
        fh.setFormatter(logging.Formatter("%(asctime)s - %(levelname)s - %(message)s"))
        ch = logging.StreamHandler()
        ch.setFormatter(logging.Formatter("%(levelname)s: %(message)s"))
        self.logger.addHandler(fh)
        self.logger.addHandler(ch)
        self.logger.info(f"Experiment directory created: {self.exp_dir}")

    def get_logger(self):
        return self.logger

    def get_experiment_dir(self):
        return self.exp_dir


def lstm_pos_weight(labels) -> float:
    """trainer.py:35-41: (n / (2 n1)) / (n / (2 n0)) * 1.5 from the train split's labels."""
    n = len(labels)
    n1 = int(sum(labels))
    n0 = n - n1
    if n1 == 0:
        raise ValueError("pos_weight is undefined: the train split holds no 'referral' video (label 1)")
    if n0 == 0:
        raise ValueError("pos_weight is undefined: the train split holds no 'non_referral' video (label 0)")
    return n / (2 * n1) / (n / (2 * n0)) * 1.5


class LstmModelSelector:
    """trainer.py:66-77, 99-122, 288-298: the composite (loss, AUROC) model selection and the early-stopping
    counter.  `update(val_loss, val_auroc)` -> True when the model is the best so far (save it)."""

    def __init__(self, loss_weight=0.3, patience=10):
        self.loss_weight, self.auroc_weight = loss_weight, 1.0 - loss_weight
        self.patience = patience
        self.best_composite_score = -float("inf")
        self.best_val_loss = float("inf")
        self.best_val_auroc = 0.0
        self.counter = 0
        self.early_stop = False

    def should_save(self, val_loss, val_auroc):
        best_val_loss = min(self.best_val_loss, val_loss)
        normalized_loss = best_val_loss / max(val_loss, 1e-10)
        composite_score = self.loss_weight * normalized_loss + self.auroc_weight * val_auroc
        if composite_score > self.best_composite_score:
            self.best_composite_score = composite_score
            self.best_val_loss = val_loss
            self.best_val_auroc = val_auroc
            return True
        return False

    def update(self, val_loss, val_auroc):
        if self.should_save(val_loss, val_auroc):
            self.counter = 0
            return True
        self.counter += 1
        if self.counter >= self.patience:
            self.early_stop = True
        return False


def _lstm_auroc(labels, scores, what, logger):
    """roc_auc_score, or 0.5 when the epoch saw one class only (the reference raises there and the per-epoch
    code has no handler: a deliberate deviation, logged)."""
    from sklearn.metrics import roc_auc_score
    if len(np.unique(labels)) < 2:
        logger.warning(f"{what} AUROC is undefined (one class only in this epoch): recording 0.5")
        return 0.5
    return float(roc_auc_score(labels, scores))


def lstm_test_metrics(labels, preds, probs, class_names, logger):
    """evaluator.py:102-173: the dict written to test_metrics.json."""
    from sklearn.metrics import accuracy_score, confusion_matrix, f1_score, precision_score, recall_score, roc_auc_score
    labels, preds = np.asarray(labels, dtype=np.int64), np.asarray(preds, dtype=np.int64)
    probs = np.asarray(probs, dtype=np.float64)
    try:
        auroc = roc_auc_score(labels, probs)
        if not np.isfinite(auroc):
            raise ValueError("one class only")
    except Exception as e:  # noqa: BLE001 - evaluator.py:104-108
        logger.error(f"Error calculating AUROC: {str(e)}")
        auroc = 0.5
    class_metrics = {}
    for ci, name in enumerate(class_names):
        mask = labels == ci
        class_metrics[name] = {
            "accuracy": float(accuracy_score(mask[mask], preds[mask] == ci)) if np.any(mask) else 0.0,
            "precision": float(precision_score(labels, preds, pos_label=ci, zero_division=0)),
            "recall": float(recall_score(labels, preds, pos_label=ci, zero_division=0)),
            "f1_score": float(f1_score(labels, preds, pos_label=ci, zero_division=0))}
    return {"auroc": float(auroc), "f1_score": float(f1_score(labels, preds, zero_division=0)),
            "accuracy": float(accuracy_score(labels, preds)),
            "precision": float(precision_score(labels, preds, zero_division=0)),
            "recall": float(recall_score(labels, preds, zero_division=0)),
            "confusion_matrix": confusion_matrix(labels, preds).tolist(), "class_metrics": class_metrics}


def _lstm_load_state(model, path, logger):
    sd = torch.load(path, map_location="cpu", weights_only=True)  # a plain state_dict (trainer.py:290)
    model.load_state_dict(sd)
    logger.info(f"Loaded weights from {path}")


def _lstm_clip_step(model, batch, crit, device, opt):
    """The reference's step on one batch of sampled clips (trainer.py:156-170): (logits, labels, loss)."""
    videos, labels = batch
    videos, labels = videos.to(device), labels.to(device)
    if opt is not None:
        opt.zero_grad()
    outputs = model(videos)
    loss = crit(outputs, labels.unsqueeze(1))
    if opt is not None:
        loss.backward()
        opt.step()
    return outputs.detach(), labels, loss.item()


def _lstm_tbptt_rounds(frame_counts, chunk):
    """Rounds in which each video is live when videos of `frame_counts` frames advance <= chunk frames per round."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    rounds = [-(-int(n) // chunk) for n in frame_counts]
    if not rounds or min(rounds) < 0 or max(rounds) == 0:
        raise ValueError(f"no frames to train on: frame counts {list(frame_counts)}")
    return rounds


def lstm_tbptt_pairs(frame_counts, chunk) -> int:
    """The (video, round) pairs of a batch, P = sum_v ceil(frames_v / chunk): video v is live in rounds
    0 .. ceil(frames_v / chunk) - 1.  Known from the frame counts before the first frame is read."""
    return sum(_lstm_tbptt_rounds(frame_counts, chunk))


def lstm_tbptt_round_weights(frame_counts, chunk):
    """The weight of each round's loss: every (video, round) pair weighs 1 / P (lstm_tbptt_pairs).  The
    criterion averages over a round's live videos, so times live / P it becomes that round's share of the mean
    over all P pairs: the weights add up to 1 and the batch loss keeps the scale of the default trainer's,
    whatever the lengths.  Returns one weight per round, the longest video's rounds."""
    rounds = _lstm_tbptt_rounds(frame_counts, chunk)
    pairs = sum(rounds)
    return [sum(1 for r in rounds if r > k) / pairs for k in range(max(rounds))]


class LstmWholeVideoBatches:
    """The --tbptt_chunk loader: batches ([paths], [labels]) of `batch_size` whole videos of a VideoDataset,
    a short last batch dropped as the default train / val loaders do.  shuffle: a new permutation of the
    dataset's video_paths per pass, seeded by (LSTM_SEED, pass number)."""

    def __init__(self, dataset, batch_size, shuffle):
        self.paths, self.labels = list(dataset.video_paths), list(dataset.labels)
        self.batch_size, self.shuffle, self.epoch = int(batch_size), shuffle, 0

    def __len__(self):
        return len(self.paths) // self.batch_size

    def __iter__(self):
        order = list(range(len(self.paths)))
        if self.shuffle:
            order = [int(i) for i in np.random.RandomState([LSTM_SEED, self.epoch]).permutation(len(order))]
            self.epoch += 1
        for k in range(len(self)):
            idx = order[k * self.batch_size:(k + 1) * self.batch_size]
            yield [self.paths[i] for i in idx], [self.labels[i] for i in idx]


def lstm_tbptt_step(chunk):
    """The step of `_lstm_epoch` for --tbptt_chunk: one batch of whole videos in rounds of <= chunk frames.
    With `opt`: forward_train_stream from the carried, detached state, the criterion on the videos live in the round
    times its lstm_tbptt_round_weights share, backward() per round (the round's graph is freed there), one
    opt.step() per batch.  Without: forward_stream over the same rounds.  Returns (each video's logit after
    its own last frame, labels, the criterion on those logits), which the epoch's loss and AUROC are made of."""
    def step(model, batch, crit, device, opt):
        paths, labels = batch
        sources = [video_io.open_video(p) for p in paths]
        weights = lstm_tbptt_round_weights([s.total_frames for s in sources], chunk)
        labels = torch.tensor(labels, dtype=torch.float32, device=device)
        final = torch.zeros(len(paths), 1, dtype=torch.float32, device=device)
        if opt is not None:
            opt.zero_grad()
        state = None
        for w, (clip, lens) in zip(weights, lstm_stream_rounds(sources, chunk, device)):
            live = torch.tensor([b for b, n in enumerate(lens) if n], device=device)
            if opt is not None:
                logits, state = model.forward_train_stream(clip, lens, state)
                (crit(logits[live], labels[live].unsqueeze(1)) * w).backward()
                state = state.detach()
            else:
                logits, state = model.forward_stream(clip, lens, state)
            final[live] = logits.detach()[live]
        if opt is not None:
            opt.step()
        return final, labels, crit(final, labels.unsqueeze(1)).item()
    return step


def _lstm_epoch(model, loader, crit, device, opt, logger, what, step=_lstm_clip_step):
    """One pass over a loader (trainer.py:146-199 with `opt`, :202-249 without): (loss, acc, auroc, number of
    videos seen).  `step` runs one batch and returns (logits, labels, loss).  A failing batch is logged and
    skipped."""
    from sklearn.metrics import accuracy_score
    total, scores, labels_all = 0.0, [], []
    for batch in loader:
        try:
            outputs, labels, loss = step(model, batch, crit, device, opt)
            total += loss * labels.numel()
            scores.extend(torch.sigmoid(outputs).float().cpu().numpy().reshape(-1))
            labels_all.extend(labels.cpu().numpy().reshape(-1))
        except Exception as e:  # noqa: BLE001
            logger.error(f"Error in {what} batch: {str(e)}")
            continue
    n = len(labels_all)
    if n == 0:
        return 0.0, 0.0, 0.5, 0
    scores, labels_all = np.asarray(scores), np.asarray(labels_all)
    preds = (scores >= 0.5).astype(int)
    return total / n, float(accuracy_score(labels_all, preds)), _lstm_auroc(labels_all, scores, what, logger), n


@torch.no_grad()
def evaluate_lstm(model, loader, device, exp_dir, logger, class_names=None):
    """evaluator.py:24-173 without the plots: sigmoid, threshold 0.5, test_metrics.json."""
    class_names = class_names or LSTM_CLASS_NAMES
    model.eval()
    preds, labels_all, probs = [], [], []
    logger.info("Starting model evaluation...")
    for i, (videos, labels) in enumerate(loader):
        try:
            p = torch.sigmoid(model(videos.to(device))).float().cpu().numpy().reshape(-1)
            probs.extend(p)
            preds.extend((p >= 0.5).astype(int))
            labels_all.extend(labels.cpu().numpy().reshape(-1))
        except Exception as e:  # noqa: BLE001 - evaluator.py:56-59
            logger.error(f"Error processing batch {i}: {str(e)}")
            continue
    if not preds:
        logger.error("No valid predictions were made during evaluation.")
        return None
    m = lstm_test_metrics(labels_all, preds, probs, class_names, logger)
    with open(Path(exp_dir) / "test_metrics.json", "w") as f:
        json.dump(m, f, indent=4)
    logger.info(f"AUROC: {m['auroc']:.4f}  F1 Score: {m['f1_score']:.4f}  Accuracy: {m['accuracy']:.4f}")
    logger.info(f"Confusion Matrix:\n{np.asarray(m['confusion_matrix'])}")
    return m


def train_lstm(model, loaders, labels, device, config, exp_dir, logger, step=_lstm_clip_step):
    """trainer.py:124-398 without wandb and the plots: returns (history, best model path or None).  `step` is
    `_lstm_epoch`'s: the reference's step on sampled clips, or lstm_tbptt_step(chunk) on LstmWholeVideoBatches."""
    from .optim import AdamW
    exp_dir = Path(exp_dir)
    pos_weight = torch.tensor([lstm_pos_weight(labels)], dtype=torch.float32, device=device)
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=pos_weight)
    # torch.optim.Adam over the trainable parameters (trainer.py:45-48) = AdamW with weight decay 0
    opt = AdamW([q for q in model.parameters() if q.requires_grad], lr=config["learning_rate"], weight_decay=0.0)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max", factor=0.5, patience=5)
    select = LstmModelSelector(config["loss_weight"], config["patience"])
    logger.info(f"Model selection weights - Loss: {select.loss_weight:.2f}, AUROC: {select.auroc_weight:.2f}")
    with open(exp_dir / "training_config.json", "w") as f:
        json.dump({k: str(v) if isinstance(v, Path) else v for k, v in config.items()}, f, indent=4)
    history = {k: [] for k in LSTM_HISTORY_KEYS}
    Path(config["model_dir"]).mkdir(parents=True, exist_ok=True)
    best_path = Path(config["model_dir"]) / f"model_{datetime.now().strftime('%Y%m%d_%H%M%S')}.pth"
    for epoch in range(config["epochs"]):
        model.train()
        tr_loss, tr_acc, tr_auroc, tn = _lstm_epoch(model, loaders["train"], crit, device, opt, logger, "training", step)
        model.eval()
        with torch.no_grad():
            va_loss, va_acc, va_auroc, vn = _lstm_epoch(model, loaders["val"], crit, device, None, logger, "validation", step)
        # a failing batch is logged and skipped, but an epoch in which EVERY batch failed must not go on to
        # save a "best" model (as run_main)
        if tn == 0:
            raise RuntimeError(f"epoch {epoch + 1}: every training batch failed or the train loader is empty (see the log)")
        if vn == 0:
            raise RuntimeError(f"epoch {epoch + 1}: every validation batch failed or the val loader is empty (see the log)")
        sched.step(va_auroc)
        for k, v in zip(LSTM_HISTORY_KEYS, (tr_loss, va_loss, tr_acc, va_acc, tr_auroc, va_auroc)):
            history[k].append(float(v))
        if select.update(va_loss, va_auroc):
            logger.info(f"Saving best model at epoch {epoch + 1} with val_loss: {va_loss:.4f}, val_auroc: {va_auroc:.4f}")
            torch.save(model.state_dict(), best_path)
        else:
            logger.info(f"Early stopping counter: {select.counter}/{select.patience}")
            if select.early_stop:
                logger.info(f"Early stopping triggered at epoch {epoch + 1}")
                break
        logger.info(f"Epoch {epoch + 1}/{config['epochs']} - Train Loss: {tr_loss:.4f}, Train Acc: {tr_acc:.4f}, "
                    f"Train AUROC: {tr_auroc:.4f} | Val Loss: {va_loss:.4f}, Val Acc: {va_acc:.4f}, "
                    f"Val AUROC: {va_auroc:.4f} | lr {opt.param_groups[0]['lr']:.2e}")
    if best_path.exists():
        _lstm_load_state(model, best_path, logger)
    else:
        logger.warning("No best model saved, using final model state")
        best_path = None
    with open(exp_dir / "training_history.json", "w") as f:
        json.dump(history, f, indent=4)
    logger.info(f"Training completed. Best validation results: Loss: {select.best_val_loss:.4f} "
                f"AUROC: {select.best_val_auroc:.4f}")
    return history, best_path


def run_main_lstm(argv=None):
    """resnet50-2d-lstm/main.py: returns (test metrics or None, history, experiment dir).  With --tbptt_chunk N >= 1
    training and validation run on whole videos in rounds of <= N frames (LstmWholeVideoBatches, lstm_tbptt_step:
    truncated BPTT with the LSTM state carried); the rest of the run is the same code."""
    import os
    args = build_parser_lstm(inference=False).parse_args(argv)
    if args.tbptt_chunk < 0:
        raise ValueError("--tbptt_chunk must be >= 0 (0: off)")
    random.seed(LSTM_SEED)  # src/utils/logging_utils.py set_seed(SEED)
    np.random.seed(LSTM_SEED)
    torch.manual_seed(LSTM_SEED)
    Path(args.log_dir).mkdir(parents=True, exist_ok=True)
    Path(args.model_dir).mkdir(parents=True, exist_ok=True)
    fam = FAMILIES["lstm"]
    exp = LstmExperimentLogger(Path(args.log_dir) / f"{fam.prefix}_{datetime.now().strftime('%Y%m%d_%H%M%S')}")
    logger = exp.get_logger()
    logger.info("Starting enhanced ResNet50-LSTM training")
    test_dir = args.test_dir if args.test_dir else args.data_dir
    config = {k: getattr(args, k) for k in ("data_dir", "model_dir", "train_sampling", "val_sampling", "test_sampling",
                                            "loss_weight", "learning_rate", "batch_size", "epochs", "patience",
                                            "hidden_size", "num_layers", "dropout", "sequence_length", "tbptt_chunk")}
    config.update(test_dir=test_dir, log_dir=exp.get_experiment_dir())
    device = _device()
    logger.info(f"Using device: {device}")
    from .data_config import lstm as data
    from .resnet50_lstm import create_model
    use_ckpt = bool(args.checkpoint_path and os.path.isfile(args.checkpoint_path))
    train = not use_ckpt and not args.skip_train  # main.py:180-199
    datasets, loaders = data.create_dataloaders(args, logger, splits=("train", "val", "test") if train else ("test",))
    logger.info(f"Using training/validation data from: {args.data_dir}")
    logger.info(f"Using test data from: {test_dir}")
    model = create_model(args.hidden_size, args.num_layers, args.dropout, device=device)
    history = {k: [] for k in LSTM_HISTORY_KEYS}
    if use_ckpt:
        logger.info(f"Loading checkpoint from {args.checkpoint_path}")
        _lstm_load_state(model, args.checkpoint_path, logger)
        best_path = args.checkpoint_path
    elif train:
        step = _lstm_clip_step
        if args.tbptt_chunk:
            logger.info(f"--tbptt_chunk {args.tbptt_chunk}: training and validation use every frame of every video, "
                        "--train_sampling, --val_sampling and --sequence_length are ignored for them")
            # a round holds a handful of videos: batch statistics would drift the running ones round by round
            model.freeze_backbone_bn = True
            logger.info("--tbptt_chunk: freeze_backbone_bn = True, the backbone's BatchNorm keeps its running statistics")
            loaders = dict(loaders, train=LstmWholeVideoBatches(datasets["train"], args.batch_size, shuffle=True),
                           val=LstmWholeVideoBatches(datasets["val"], args.batch_size, shuffle=False))
            step = lstm_tbptt_step(args.tbptt_chunk)
        history, best_path = train_lstm(model, loaders, datasets["train"].labels, device, config,
                                        exp.get_experiment_dir(), logger, step)
        logger.info(f"Training completed. Best model saved to {best_path}")
    else:
        logger.info("Skipping training as requested")
        best_path = None
    if not best_path:
        logger.error("No model available for evaluation")
        return None, history, exp.get_experiment_dir()
    logger.info(f"Evaluating model from {best_path}")
    m = evaluate_lstm(model, loaders["test"], device, exp.get_experiment_dir(), logger, LSTM_CLASS_NAMES)
    return m, history, exp.get_experiment_dir()


def lstm_inference_videos(args):
    """inference.py:250-267: the three ways the reference lists its videos; besides its extensions the
    formats vclip_amd.video_io decodes (`.npy` clips)."""
    import glob
    import os
    if args.single_video:
        return [args.single_video] if os.path.exists(args.single_video) else None
    files = []
    if args.batch_mode:
        for ext in ("*.mp4", "*.avi", "*.mov", "*.npy"):
            files.extend(glob.glob(os.path.join(args.videos_dir, "**", ext), recursive=True))
    else:
        for dir_name in ("referral", "non_referral"):
            for ext in ("*.mp4", "*.npy"):
                files.extend(glob.glob(os.path.join(args.videos_dir, dir_name, ext)))
    return files


LSTM_INFERENCE_SAMPLERS = {"random": sampling.lstm_random_sampling, "random_window": sampling.lstm_random_window_sampling,
                           "uniform": sampling.lstm_uniform_sampling}


def lstm_model_from_checkpoint(path, device):
    """VideoResNet50LSTM of the checkpoint's own LSTM shape (the reference's inference script builds
    DEFAULT_CONFIG's 256 x 2, which a checkpoint trained with other --hidden_size / --num_layers cannot load)."""
    from .resnet50_lstm import VideoResNet50LSTM
    sd = torch.load(path, map_location="cpu", weights_only=True)
    sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
    hidden = int(sd["lstm.weight_hh_l0"].shape[1])
    layers = sum(1 for k in sd if k.startswith("lstm.weight_hh_l"))
    model = VideoResNet50LSTM(hidden, layers, 0.5)
    model.load_state_dict(sd)
    return model.to(device).eval()


def _lstm_load_video(path, method, sequence_length, device):
    """inference.py:132-178 up to the model: (clip f32 [1, 3, T, 224, 224], frame indices, total frames) with
    T = min(sequence_length, total frames)."""
    from . import preprocess as pp
    src = video_io.open_video(path)
    total = src.total_frames
    idx = [int(i) for i in LSTM_INFERENCE_SAMPLERS.get(method, sampling.lstm_uniform_sampling)(total, sequence_length)]
    frames = torch.from_numpy(np.ascontiguousarray(src.read(idx))).to(device)
    frames = pp.cv2_resize_u8(frames, (224, 224))
    return pp.lstm_inference_preprocess(frames), idx, total


def lstm_stream_rounds(sources, chunk, device):
    """Opened videos (video_io sources) in lockstep: every round reads the next <= chunk frames of each, resizes
    and normalises them on the GPU as _lstm_load_video does, and yields (clip f32 [1, 3, N, 224, 224], the
    frames of each video in it); a finished video takes length 0.  The layout of forward_stream and
    forward_train_stream."""
    from . import preprocess as pp
    totals = [int(s.total_frames) for s in sources]
    pos = [0] * len(sources)
    while any(p < t for p, t in zip(pos, totals)):
        lens = [min(chunk, t - p) for p, t in zip(pos, totals)]
        parts = [np.ascontiguousarray(s.read(list(range(p, p + n)))) for s, p, n in zip(sources, pos, lens) if n]
        sizes = {a.shape[1:3] for a in parts}
        if len(sizes) == 1:  # one resize over the round's frames
            frames = pp.cv2_resize_u8(torch.from_numpy(np.concatenate(parts)).to(device), (224, 224))
        else:
            frames = torch.cat([pp.cv2_resize_u8(torch.from_numpy(a).to(device), (224, 224)) for a in parts])
        pos = [p + n for p, n in zip(pos, lens)]
        yield pp.lstm_inference_preprocess(frames), lens


def lstm_stream_videos(model, sources, chunk, device, saliency_class="off"):
    """Whole-video inference over opened videos in lockstep (lstm_stream_rounds): one forward_stream call per
    round with the carried state; a finished video keeps its logit.
    Returns (probabilities, one per video; per-frame probability lists, total_frames entries each).
    saliency_class None / 0 / 1 (instead of "off"): the rounds go through an explain session
    (VideoResNet50LSTM.explain_stream_begin: the same launches, bit-identical logits) and its Explanation is returned
    as a third value."""
    frame_probs = [[] for _ in sources]
    state, logits = None, None
    sess = None if saliency_class == "off" else model.explain_stream_begin(len(sources))
    for clip, lens in lstm_stream_rounds(sources, chunk, device):
        if sess is None:
            logits, state, fl = model.forward_stream(clip, lens, state, frame_logits=True)
        else:
            logits, fl = sess.push(clip, lens)
        fp = torch.sigmoid(fl.float()).reshape(-1).tolist()
        at = 0
        for b, n in enumerate(lens):
            frame_probs[b].extend(fp[at:at + n])
            at += n
    probs = torch.sigmoid(logits.float()).reshape(-1).tolist()
    return (probs, frame_probs) if sess is None else (probs, frame_probs, sess.finish(target=saliency_class))


def _write_csv(rows, path):
    """pd.DataFrame(rows).to_csv(path, index=False) (inference.py:310-321); the csv module where pandas is absent."""
    try:
        import pandas as pd
    except ImportError:
        import csv
        with open(path, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
            w.writeheader()
            w.writerows(rows)
        return
    pd.DataFrame(rows).to_csv(path, index=False)


def run_inference_lstm(argv=None):
    """resnet50-2d-lstm/inference.py on batched ragged inference: up to --videos_per_batch videos, each with
    its own (clamped) frame count, go through one `forward_ragged`.  With --stream_chunk N >= 1 instead every
    video is read whole and the videos of a batch advance in lockstep through `forward_stream`, <= N frames each
    per call (lstm_stream_videos); frame_probabilities/<video>.csv and summary["stream_chunk"] are added.
    With --saliency each batch goes through `explain(..., lengths=...)` instead (the same logits): saliency/<video>.npy
    (f32 [T, h, w]) and the row fields saliency_file, saliency_target and frame_importance; with --stream_chunk through the
    explain session: the relevance and importance columns of frame_probabilities/<video>.csv and saliency_target.
    Returns the summary dict (None when no video was found or none succeeded), with the experiment directory
    under "output_dir"."""
    import os
    parser = build_parser_lstm(inference=True)
    args = parser.parse_args(argv)
    if args.saliency is None and args.saliency_class is not None:
        parser.error("--saliency_class needs --saliency gradcam or hirescam")
    if args.saliency is None and args.saliency_layer != "res5":
        parser.error("--saliency_layer needs --saliency gradcam or hirescam")
    if args.saliency is not None and args.stream_chunk and args.saliency_layer != "res5":
        parser.error("--saliency_layer does not apply with --stream_chunk: a streamed recording gets per-frame relevance, "
                     "no spatial maps")
    exp = LstmExperimentLogger(os.path.join(args.output_dir, f"inference_{datetime.now().strftime('%Y%m%d_%H%M%S')}"),
                               prefix="inference")
    logger = exp.get_logger()
    out_dir = exp.get_experiment_dir()
    if args.visualize:
        logger.warning("--visualize: plots are not part of this build; the CSV / JSON results are written as usual")
    if args.videos_per_batch < 1:
        raise ValueError("--videos_per_batch must be >= 1")
    if args.stream_chunk < 0:
        raise ValueError("--stream_chunk must be >= 0 (0: off)")
    if args.stream_chunk:
        logger.info(f"--stream_chunk {args.stream_chunk}: every frame of every video goes through the model, "
                    "--sampling_method and --sequence_length are ignored")
    device = _device()
    model = lstm_model_from_checkpoint(args.model_path, device)
    video_files = lstm_inference_videos(args)
    if video_files is None:
        logger.error(f"Video file not found: {args.single_video}")
        return None
    if not video_files:
        logger.error("No video files found to process")
        return None
    logger.info(f"Found {len(video_files)} videos to process")
    results = [None] * len(video_files)

    def error_row(path, e):
        print(f"Error processing video {path}: {str(e)}")
        return {"video_path": path, "prediction": None, "probability": None, "status": f"error: {str(e)}"}

    def unique_name(folder, k, suffix):
        name = os.path.basename(video_files[k])
        if (folder / f"{name}{suffix}").exists():  # the same file name in two folders
            name = f"{k}_{name}"
        return f"{name}{suffix}"

    def flush(batch):
        if not batch:
            return
        ex = None
        try:
            clips, lens = torch.cat([c for _, c, _, _ in batch], dim=2), [len(i) for _, _, i, _ in batch]
            with torch.no_grad():
                if args.saliency:
                    ex = model.explain(clips, method=args.saliency, target=args.saliency_class, layer=args.saliency_layer,
                                       lengths=lens)
                    logits = ex.logits
                else:
                    logits = model.forward_ragged(clips, lens)
            probs = torch.sigmoid(logits.float()).reshape(-1).tolist()
        except Exception as e:  # noqa: BLE001 - the whole call failed: its videos get the error row
            for k, _, _, _ in batch:
                results[k] = error_row(video_files[k], e)
            return
        for (k, _, idx, total), p in zip(batch, probs):
            results[k] = {"video_path": video_files[k], "prediction": "referral" if p >= 0.5 else "non_referral",
                          "probability": float(p), "sampled_frames": len(idx), "total_frames": total,
                          "frame_indices": idx, "status": "success"}
        if ex is not None:
            sal_dir = out_dir / "saliency"
            sal_dir.mkdir(exist_ok=True)
            for b, (k, _, _, _) in enumerate(batch):
                name = unique_name(sal_dir, k, ".npy")
                np.save(sal_dir / name, ex.saliency[b].numpy())
                results[k].update(saliency_file=f"saliency/{name}", saliency_target=int(ex.target[b]),
                                  frame_importance=[float(v) for v in ex.temporal[b].tolist()])

    def flush_stream(batch):
        if not batch:
            return
        ex = None
        try:
            if args.saliency:
                probs, frame_probs, ex = lstm_stream_videos(model, [src for _, src in batch], args.stream_chunk, device,
                                                            saliency_class=args.saliency_class)
            else:
                probs, frame_probs = lstm_stream_videos(model, [src for _, src in batch], args.stream_chunk, device)
        except Exception as e:  # noqa: BLE001 - the whole group failed: its videos get the error row
            for k, _ in batch:
                results[k] = error_row(video_files[k], e)
            return
        fp_dir = out_dir / "frame_probabilities"
        fp_dir.mkdir(exist_ok=True)
        for b, ((k, src), p, fp) in enumerate(zip(batch, probs, frame_probs)):
            name = unique_name(fp_dir, k, ".csv")
            rows = [{"frame": i, "probability": v} for i, v in enumerate(fp)]
            if ex is not None:
                for row, r, t in zip(rows, ex.frame_relevance[b].tolist(), ex.temporal[b].tolist()):
                    row.update(relevance=r, importance=t)
            _write_csv(rows, fp_dir / name)
            results[k] = {"video_path": video_files[k], "prediction": "referral" if p >= 0.5 else "non_referral",
                          "probability": float(p), "sampled_frames": src.total_frames, "total_frames": src.total_frames,
                          "frame_indices": "all", "status": "success"}
            if ex is not None:
                results[k]["saliency_target"] = int(ex.target[b])

    batch = []
    for k, path in enumerate(video_files):
        try:  # a video that fails to open or decode does not take its batch down (inference.py:196-203)
            if args.stream_chunk:
                src = video_io.open_video(path)
                if src.total_frames < 1:
                    raise ValueError("the video has no frames")
                batch.append((k, src))
            else:
                clip, idx, total = _lstm_load_video(path, args.sampling_method, args.sequence_length, device)
                batch.append((k, clip, idx, total))
        except Exception as e:  # noqa: BLE001
            results[k] = error_row(path, e)
            continue
        if len(batch) == args.videos_per_batch:
            (flush_stream if args.stream_chunk else flush)(batch)
            batch = []
    (flush_stream if args.stream_chunk else flush)(batch)
    for r in results:
        name = os.path.basename(r["video_path"])
        if r["status"] == "success":
            conf = r["probability"] if r["prediction"] == "referral" else 1 - r["probability"]
            logger.info(f"Video: {name}, Prediction: {r['prediction']}, Confidence: {conf:.4f}")
        else:
            logger.error(f"Error processing {name}: {r['status']}")
    ok = [r for r in results if r["status"] == "success"]
    failed = [r for r in results if r["status"] != "success"]
    if not ok:
        logger.error("No successful predictions were made")
        return None
    summary = {"total_videos": len(results), "successful_predictions": len(ok), "failed_predictions": len(failed),
               "referral_cases": sum(1 for r in ok if r["prediction"] == "referral"),
               "non_referral_cases": sum(1 for r in ok if r["prediction"] == "non_referral"),
               "sampling_method": args.sampling_method, "sequence_length": args.sequence_length,
               "model_path": args.model_path}
    if args.stream_chunk:
        summary["stream_chunk"] = args.stream_chunk
    _write_csv(ok, out_dir / "inference_results.csv")
    if failed:
        _write_csv(failed, out_dir / "inference_failures.csv")
    with open(out_dir / "inference_summary.json", "w") as f:
        json.dump(summary, f, indent=4)
    _write_csv([summary], out_dir / "inference_summary.csv")
    logger.info(f"Total videos processed: {len(results)}  successful: {len(ok)}  failed: {len(failed)}  "
                f"referral: {summary['referral_cases']}  non-referral: {summary['non_referral_cases']}")
    logger.info(f"Results saved to {out_dir}")
    return dict(summary, output_dir=str(out_dir))
