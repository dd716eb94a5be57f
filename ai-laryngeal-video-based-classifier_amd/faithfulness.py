"""Saliency faithfulness: the perturbation test (Samek et al. 2017) as the deletion and insertion games of Petsiuk et
al. 2018 (RISE), for every family and any saliency map.

The cells of a map [B, Tg, Hg, Wg] are ranked on the host; step i of `steps` removes the first k_i = i*N // steps
cells of that order from the clip (deletion: their pixels take the baseline) or puts only those into the baseline
(insertion), and the model's ordinary eval forward scores every step.  The result is the class score as a curve over
the removed fraction and its area: a map that points at what the model used makes the deletion curve fall, and the
insertion curve rise, faster than a random order does.

One vc_perturb_clips launch builds the (steps + 1) * B clips (csrc/perturb.hip); the blurred baseline is
vc_gaussian_blur_planes.  No `explain` is called here: a map made elsewhere is scored the same way.  There is no CPU
path and no fallback: what cannot be scored raises.
"""
from __future__ import annotations

import torch

from . import explaining, ops

MODES = ("deletion", "insertion")
BASELINES = ("zero", "blur")
ORDERS = ("relevance", "random")
BLUR_KSIZE, BLUR_SIGMA = 11, 5.0  # RISE's canvas


class PerturbationCurve:
    """What perturbation_curve returns, all on the host: `fractions` f64 [steps+1] (k_i / N), `logits` f32
    [B, steps+1, labels], `score` f32 [B, steps+1] (the target's probability), `auc` f64 [B] (the trapezoid of score
    over fractions), `target` (the B class indices scored) and the `mode`, `baseline` and `order` it was run with."""

    def __init__(self, fractions, logits, score, auc, target, mode, baseline, order):
        self.fractions, self.logits, self.score, self.auc = fractions, logits, score, auc
        self.target, self.mode, self.baseline, self.order = target, mode, baseline, order


def step_counts(N: int, steps: int) -> list:
    """k_i = i*N // steps for i = 0..steps: k_0 = 0, k_steps = N, nondecreasing (repeats when N < steps)."""
    if steps < 1:
        raise ValueError("steps must be at least 1")
    return [(i * N) // steps for i in range(steps + 1)]


def cell_ranks(saliency: torch.Tensor, order: str = "relevance", seed: int = 0) -> torch.Tensor:
    """int32 [B, N]: rank[b, cell] = the position of `cell` in clip b's order of removal.  "relevance": the stable
    descending argsort of the flattened map, so equal cells go lower index first; "random": one permutation per clip
    from a torch.Generator seeded with `seed`, drawn in clip order.  saliency: host [B, ...]."""
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, not {order!r}")
    flat = saliency.reshape(saliency.shape[0], -1)
    B, N = flat.shape
    if order == "relevance":
        perm = torch.argsort(flat, dim=1, descending=True, stable=True)
    else:
        g = torch.Generator().manual_seed(int(seed))
        perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    rank = torch.empty(B, N, dtype=torch.int32)
    rank.scatter_(1, perm, torch.arange(N, dtype=torch.int32).expand(B, N).contiguous())
    return rank


def trapezoid(score: torch.Tensor, fractions: torch.Tensor) -> torch.Tensor:
    """f64 [B]: sum_i (x_{i+1} - x_i) * (y_{i+1} + y_i) / 2 of score [B, n] over fractions [n]."""
    y, x = score.double(), fractions.double()
    return ((x[1:] - x[:-1]) * (y[:, 1:] + y[:, :-1]) / 2.0).sum(dim=1)


def _family(model):
    """(clip layout, logits(model, clips), label count; 1 = the LSTM's single referral logit)"""
    from .resnet3d import ResNet3d
    from .resnet50_lstm import VideoResNet50LSTM
    from .swin3d import Swin3d
    from .timesformer import TimesformerForVideoClassification
    from .vivit import VivitForVideoClassification
    if isinstance(model, (VivitForVideoClassification, TimesformerForVideoClassification)):
        return "btchw", lambda m, x: m(pixel_values=x).logits, int(model.config.num_labels)
    if isinstance(model, Swin3d):
        return "bcthw", lambda m, x: m(x), int(model.num_classes)
    if isinstance(model, ResNet3d):
        return "bcthw", lambda m, x: m(x), int(model.cfg["num_classes"])
    if isinstance(model, VideoResNet50LSTM):
        return "bcthw", lambda m, x: m(x), 1
    raise TypeError(f"faithfulness: no clip family for {type(model).__name__}")


def _host_map(saliency, B: int, thw) -> torch.Tensor:
    sal = saliency.saliency if isinstance(saliency, explaining.Explanation) else saliency
    if not isinstance(sal, torch.Tensor):
        raise ValueError("saliency must be an Explanation of a dense batch or a [B, Tg, Hg, Wg] tensor")
    if sal.dim() != 4 or sal.shape[0] != B:
        raise ValueError(f"saliency {tuple(sal.shape)} does not fit {B} clips: [B, Tg, Hg, Wg] wanted")
    if sal.dtype != torch.float32:
        raise ValueError("saliency must be float32")
    if sal.numel() == 0 or any(g > n for g, n in zip(sal.shape[1:], thw)):
        raise ValueError(f"saliency grid {tuple(sal.shape[1:])} is empty or larger than the clip's (T, H, W) = {tuple(thw)}")
    sal = sal.detach().cpu()
    if not bool(torch.isfinite(sal).all()):
        raise ValueError("saliency holds a non-finite value")
    return sal


def _targets(target, B: int, labels: int):
    return explaining.expand_targets(*explaining.check_targets(target, max(labels, 2)), B, who="")


def _score(logits: torch.Tensor, target: list, labels: int) -> torch.Tensor:
    """f32 [B, steps+1] from host logits [B, steps+1, labels]"""
    t = torch.tensor(target, dtype=torch.int64)
    if labels == 1:
        p = torch.sigmoid(logits[:, :, 0])
        return torch.where(t[:, None] == 1, p, 1.0 - p)
    return torch.softmax(logits, dim=2).gather(2, t[:, None, None].expand(-1, logits.shape[1], 1))[:, :, 0].contiguous()


def perturbation_curve(model, clip: torch.Tensor, saliency, *, mode: str = "deletion", steps: int = 10,
                       baseline: str = "zero", order: str = "relevance", seed: int = 0, target=None,
                       chunk: int | None = None) -> PerturbationCurve:
    """The class score of `model` on `clip` as the cells of `saliency` are removed (mode "deletion") or inserted into
    the baseline ("insertion") in `order`, in steps + 1 points from none of the cells to all of them.

    clip: what the model's forward takes, f32 on the GPU: [B,T,C,H,W] for ViViT and TimeSformer, [B,C,T,H,W] (dense) for
    Swin3d, ResNet3d and VideoResNet50LSTM.  saliency: an Explanation or a f32 [B, Tg, Hg, Wg] tensor on either device;
    pixel (t, y, x) belongs to cell ((t*Tg//T)*Hg + y*Hg//H)*Wg + x*Wg//W.  baseline "zero": 0 in the model's normalised
    input; "blur": the clip under an 11-tap sigma-5 Gaussian.  order "relevance" (ties: lower cell first) or "random"
    (seeded by `seed`).  target: None (the unperturbed clip's argmax; the LSTM: logit > 0), an int or B ints.  chunk:
    clips per forward (default B, one step).  The model must be in eval mode; nothing of it is changed."""
    layout, logits_of, labels = _family(model)
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, not {mode!r}")
    if baseline not in BASELINES:
        raise ValueError(f"baseline must be one of {BASELINES}, not {baseline!r}")
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, not {order!r}")
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise ValueError("steps must be an int, at least 1")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError("chunk must be None or an int, at least 1")
    if model.training:
        raise RuntimeError("faithfulness scores the eval-mode forward: call model.eval() first")
    if not isinstance(clip, torch.Tensor) or clip.dim() != 5:
        raise ValueError("clip must be [B,T,C,H,W] (ViViT, TimeSformer) or [B,C,T,H,W] (Swin3d, ResNet3d, VideoResNet50LSTM)")
    B = clip.shape[0]
    T = clip.shape[1] if layout == "btchw" else clip.shape[2]
    sal = _host_map(saliency, B, (T, clip.shape[3], clip.shape[4]))
    target = _targets(target, B, labels)
    if clip.device.type != "cuda":
        raise RuntimeError("faithfulness runs on the GPU only: move the clip batch to cuda")
    x = clip.detach().float().contiguous()
    grid = tuple(int(g) for g in sal.shape[1:])
    N = grid[0] * grid[1] * grid[2]
    ks = step_counts(N, steps)
    rank = cell_ranks(sal, order, seed).to(x.device)
    k = torch.tensor(ks, dtype=torch.int32, device=x.device)
    with torch.no_grad():
        base = ops.gaussian_blur_planes(x, BLUR_KSIZE, BLUR_SIGMA) if baseline == "blur" else None
        clips = ops.perturb_clips(x, rank, k, grid, layout, mode, base=base)
        flat = clips.view(((steps + 1) * B,) + tuple(x.shape[1:]))
        n = B if chunk is None else chunk
        # every forward's logits go to the host at once: a family's forward may return its workspace buffer
        rows = [logits_of(model, flat[i:i + n]).detach().float().cpu() for i in range(0, flat.shape[0], n)]
    logits = torch.cat(rows).reshape(steps + 1, B, -1).transpose(0, 1).contiguous()
    if target is None:
        whole = logits[:, 0 if mode == "deletion" else steps]  # the step with every pixel the clip's own
        target = (whole[:, 0] > 0).long().tolist() if labels == 1 else whole.argmax(dim=1).tolist()
    fractions = torch.tensor([kk / N for kk in ks], dtype=torch.float64)
    score = _score(logits, target, labels)
    return PerturbationCurve(fractions, logits, score, trapezoid(score, fractions), target, mode, baseline, order)


def faithfulness(model, clip: torch.Tensor, saliency, *, steps: int = 10, baseline: str = "zero", target=None,
                 seed: int = 0) -> dict:
    """Deletion and insertion in relevance order and deletion in a random order (seeded by `seed`), all scoring the
    same classes (target None: the unperturbed clip's prediction).  Per clip (f64 [B]): deletion_auc (lower: the map
    points at what the model used), insertion_auc (higher), random_deletion_auc and deletion_gain =
    random_deletion_auc - deletion_auc (positive: better than chance); plus the three PerturbationCurve objects as
    deletion, insertion and random_deletion, and target, steps and baseline."""
    kw = dict(steps=steps, baseline=baseline)
    dele = perturbation_curve(model, clip, saliency, mode="deletion", target=target, **kw)
    ins = perturbation_curve(model, clip, saliency, mode="insertion", target=dele.target, **kw)
    rnd = perturbation_curve(model, clip, saliency, mode="deletion", order="random", seed=seed, target=dele.target, **kw)
    return dict(deletion_auc=dele.auc, insertion_auc=ins.auc, random_deletion_auc=rnd.auc,
                deletion_gain=rnd.auc - dele.auc, deletion=dele, insertion=ins, random_deletion=rnd,
                target=dele.target, steps=steps, baseline=baseline)
