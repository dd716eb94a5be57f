"""Host-side scaffolding the explain paths of the five families share around their kernels: the result type, the
argument checks with their messages, the per-clip normalisation and the small buffer cache.  What is kept during the
forward and how the relevance walks back differ per family and stay in the family files.
"""
from __future__ import annotations

import operator

import numpy as np
import torch


class Explanation:
    """What VivitForVideoClassification.explain returns: `logits` f32 [B, labels] on the device;
    `token_relevance` f32 [B, S] (column 0 is CLS), `saliency` f32 [B, T/kt, H/kh, W/kw] (the patch tokens'
    relevance divided by its per-clip sum) and `temporal` f32 [B, T/kt] (saliency summed over space) on the host.
    `target`: the B class indices a class-specific method ("grad_rollout"; ResNet3d.explain's Grad-CAM / HiResCAM, whose
    `token_relevance` is the signed map with no CLS column) explained, None for the others.
    `frame_relevance`: VideoResNet50LSTM.explain's signed gradient x input per frame, f32 [B, T] on the host (a list
    of per-video tensors for ragged batches and streamed recordings); None for every other family."""

    def __init__(self, logits, token_relevance, saliency, temporal, method, target=None, frame_relevance=None):
        self.logits, self.token_relevance, self.saliency, self.temporal = logits, token_relevance, saliency, temporal
        self.method = method
        self.target = target
        self.frame_relevance = frame_relevance


def check_targets(target, num_labels: int, who: str = "explain"):
    """`target` of a class-specific method checked against `num_labels` labels: (None or a list of class indices,
    whether it was one int for every clip).  `who` names the method in the messages."""
    if target is None:
        return None, False
    if isinstance(target, torch.Tensor):
        if target.is_floating_point() or target.dtype == torch.bool:
            raise ValueError(f"{who}: target must hold integers")
        target = target.tolist()
    if isinstance(target, bool):
        raise ValueError(f"{who}: target must be None, an int or a sequence of B ints")
    scalar = not isinstance(target, (list, tuple, np.ndarray))
    try:
        target = [operator.index(target)] if scalar else [operator.index(t) for t in target]
    except TypeError:
        raise ValueError(f"{who}: target must be None, an int or a sequence of B ints") from None
    if any(not 0 <= t < num_labels for t in target):
        raise ValueError(f"{who}: target {target} out of range for {num_labels} labels")
    return target, scalar


def expand_targets(target, scalar: bool, B: int, who: str = "explain", what: str = "clips"):
    """check_targets' pair as B class indices (None stays None): one int is repeated, a sequence must hold B"""
    if target is None:
        return None
    target = target * B if scalar else target
    if len(target) != B:
        raise ValueError(f"{who + ': ' if who else ''}target has {len(target)} entries for {B} {what}")
    return target


def require_method(method, methods, who: str = "explain"):
    if method not in methods:
        raise ValueError(f"{who}: method must be one of {methods}, not {method!r}")


def require_residual(residual, who: str = "explain"):
    if not 0.0 < float(residual) <= 1.0:
        raise ValueError(f"{who}: residual must be in (0, 1], not {residual}")


def require_explainable(model, x, who: str = "explain", what: str = "the clip batch"):
    """The refusals every explain path starts from (no fallback): training mode, anything but a tensor on the GPU"""
    if model.training:
        raise RuntimeError(f"{who}: inference only; call model.eval() first")
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError(f"{who} runs on the GPU only: move {what} to cuda")


def normalise(rel: torch.Tensor, zero_ok: bool) -> torch.Tensor:
    """rel (double, [B, ...]) over its per-clip sum, as f32.  zero_ok: a clip whose sum is not positive gets an all-zero
    map; otherwise the plain division (the caller knows, or has checked, that every sum is positive)."""
    total = rel.sum(dim=tuple(range(1, rel.dim())), keepdim=True)
    if not zero_ok:
        return (rel / total).float()
    pos = total > 0
    return torch.where(pos, rel / torch.where(pos, total, torch.ones_like(total)), torch.zeros_like(rel)).float()


def cached_explain(cache: dict, key, build, limit: int = 2):
    """cache[key], made by build() on first use; the cache is emptied first when it already holds `limit` entries
    (an entry is hundreds of MB: the last shapes explained stay, nothing accumulates)"""
    if key not in cache:
        if len(cache) >= limit:
            cache.clear()
        cache[key] = build()
    return cache[key]
