"""RISE saliency (Randomized Input Sampling for Explanation, Petsiuk et al. 2018): a class-specific, black-box map at
pixel resolution for every family.

The clip is put under N smooth random masks, the model's ordinary eval forward scores each masked clip, and the map is
the score-weighted sum of the masks: S = sum_n p_n(target) * m_n.  Nothing inside the model is used: no gradient, no
kept activation, so one implementation serves ViViT, TimeSformer, Swin3d, ResNet3d and VideoResNet50LSTM, and Swin and
TimeSformer get the class-specific map their `explain` does not have.

The masks (fixed here so that the kernels and tests/rise_ref.py agree).  For the clip extent (T, H, W) and `cells` =
(ct, ch, cw), 1 <= c <= extent, the cell size per axis is S = ceil(extent / c).  Mask n is a bit grid uint8
[ct+2, ch+2, cw+2], each bit 1 with probability `keep`, and a shift (dt, dy, dx), 0 <= d < S.  For pixel (t, y, x):
u = t + dt, i = u // St, f = float32(u % St) / float32(St), likewise for y and x, and m_n(t, y, x) is the trilinear
interpolation of the eight bits at [i..i+1, j..j+1, k..k+1], along x, then y, then t, each step fmaf(f, b - a, a).
The + 2 keeps i + 1 inside the grid (u <= T - 1 + St - 1 < (ct + 1) * St); S == 1 gives shift 0 and f == 0.  The grid
corners sit on cell corners: this is not the alignment of the paper's skimage.resize of a (c + 1)-cell grid followed
by a random crop, only the same family of masks (bilinear blobs of cell size S at a uniformly random offset).  All
clips of a batch share one mask set.

Drawing order (rise_masks): one torch.Generator().manual_seed(seed); first all bits, `torch.rand((masks, ct+2, ch+2,
cw+2), dtype=float32) < keep`; then the shifts, one `torch.randint(0, S, (masks,))` per axis in the order t, y, x.

Device work: vc_rise_apply builds a chunk's masked clips in one pass over the clip, vc_rise_accumulate adds the chunk's
score-weighted masks to the map (csrc/rise.hip).  There is no CPU path and no fallback: what cannot be mapped raises.
"""
from __future__ import annotations

import torch

from . import ops
from .faithfulness import BASELINES, BLUR_KSIZE, BLUR_SIGMA, _family, _score, _targets
from .explaining import Explanation

# masks per rise_apply launch and clips per forward when rise_map's `chunk` is None, per family.  The rule is the
# project's for the LSTM's --videos_per_batch: the smallest value whose masks/s is within 5 % of the best of the sweep
# 4, 8, 16, 32, 64 of tools/rise_time.py at the family's benchmark shape, B = 1 (profiles/rise_time.json).
DEFAULT_CHUNK = {"VivitForVideoClassification": 32, "TimesformerForVideoClassification": 32, "Swin3d": 32, "ResNet3d": 16,
                 "VideoResNet50LSTM": 64}


def default_chunk(model) -> int:
    """the family's DEFAULT_CHUNK (a subclass takes its family's)"""
    return next(DEFAULT_CHUNK[c.__name__] for c in type(model).__mro__ if c.__name__ in DEFAULT_CHUNK)


class RiseExplanation(Explanation):
    """What rise_map returns: an Explanation with method "rise".  `logits`: the unperturbed clips' logits, f32
    [B, labels] on the device.  On the host: `token_relevance` f32 [B, T*H*W], the weighted mask sum over masks * keep
    (the paper's normalisation; no CLS column); `saliency` f32 [B, T, H, W], the sum divided by its per-clip total (all
    zero when that is 0); `temporal` f32 [B, T]; `mask_logits` f32 [B, masks, labels] and `mask_scores` f32 [B, masks],
    the model on every masked clip and the target's probability there.  `target`: the B classes mapped; `masks`,
    `cells` (as used: no None), `keep`, `seed` and `baseline` as the map was made."""

    def __init__(self, logits, token_relevance, saliency, temporal, target, mask_logits, mask_scores, masks, cells, keep,
                 seed, baseline):
        super().__init__(logits, token_relevance, saliency, temporal, "rise", target=target)
        self.mask_logits, self.mask_scores = mask_logits, mask_scores
        self.masks, self.cells, self.keep, self.seed, self.baseline = masks, cells, keep, seed, baseline


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _check_cells(cells, T: int, H: int, W: int) -> tuple:
    if not isinstance(cells, (tuple, list)) or len(cells) != 3:
        raise ValueError("cells must be (ct, ch, cw)")
    ct = max(1, T // 8) if cells[0] is None else cells[0]  # eight frames per temporal cell: a choice nobody has measured
    out = (ct, cells[1], cells[2])
    if not all(_is_int(c) and 1 <= c <= n for c, n in zip(out, (T, H, W))):
        raise ValueError(f"cells {tuple(cells)} must be ints from 1 to the clip's (T, H, W) = {(T, H, W)} (cells[0] may be None)")
    return out


def cell_sizes(T: int, H: int, W: int, cells) -> tuple:
    """(St, Sh, Sw) = ceil(extent / cells) per axis"""
    return tuple(-(-n // c) for n, c in zip((T, H, W), cells))


def rise_masks(T: int, H: int, W: int, cells, keep: float, masks: int, seed: int = 0):
    """The host sampler: (bits uint8 [masks, ct+2, ch+2, cw+2], shifts int32 [masks, 3]) for the extent (T, H, W), drawn
    from one torch.Generator seeded with `seed` in the order the module docstring gives.  cells[0] None: max(1, T // 8)."""
    if not all(_is_int(n) and n >= 1 for n in (T, H, W)):
        raise ValueError("T, H and W must be positive ints")
    cells = _check_cells(cells, T, H, W)
    if isinstance(keep, bool) or not isinstance(keep, (int, float)) or not 0.0 < float(keep) < 1.0:
        raise ValueError("keep must be a probability strictly between 0 and 1")
    if not _is_int(masks) or masks < 1:
        raise ValueError("masks must be an int, at least 1")
    if not _is_int(seed):
        raise ValueError("seed must be an int")
    g = torch.Generator().manual_seed(seed)
    ct, ch, cw = cells
    bits = (torch.rand((masks, ct + 2, ch + 2, cw + 2), generator=g, dtype=torch.float32) < float(keep)).to(torch.uint8)
    shifts = torch.stack([torch.randint(0, s, (masks,), generator=g) for s in cell_sizes(T, H, W, cells)], dim=1)
    return bits.contiguous(), shifts.to(torch.int32).contiguous()


def rise_map(model, clip: torch.Tensor, *, target=None, masks: int = 4000, cells=(None, 7, 7), keep: float = 0.5,
             baseline: str = "zero", seed: int = 0, chunk: int | None = None) -> RiseExplanation:
    """The RISE map of `model` on `clip` for the class `target`: sum over `masks` random masks of the target's score on
    the masked clip times the mask.

    clip: what the model's forward takes, f32 on the GPU: [B,T,C,H,W] for ViViT and TimeSformer, [B,C,T,H,W] (dense) for
    Swin3d, ResNet3d and VideoResNet50LSTM.  target: None (the unperturbed clip's argmax; the LSTM: logit > 0), an int
    or B ints; the score is the softmax probability of the target (the LSTM's single logit: the sigmoid, or its
    complement for target 0).  masks = 4000, cells (., 7, 7) and keep = 0.5 are the paper's setup for images; cells[0] =
    None means max(1, T // 8) temporal cells, a choice nobody has measured.  baseline: what a masked-out pixel shows,
    "zero" (0 in the model's normalised input) or "blur" (the clip under faithfulness's 11-tap sigma-5 Gaussian).
    chunk: masks per rise_apply launch, and clips per forward at most (default: the family's DEFAULT_CHUNK); the map
    does not depend on it beyond the model's own batch-size dependence.  The model must be in eval mode; nothing of it
    is changed.
    The result goes straight into faithfulness(model, clip, result), whose grid is then the pixel grid."""
    layout, logits_of, labels = _family(model)
    if baseline not in BASELINES:
        raise ValueError(f"baseline must be one of {BASELINES}, not {baseline!r}")
    if chunk is not None and (not _is_int(chunk) or chunk < 1):
        raise ValueError("chunk must be None or an int, at least 1")
    if model.training:
        raise RuntimeError("RISE scores the eval-mode forward: call model.eval() first")
    if not isinstance(clip, torch.Tensor) or clip.dim() != 5:
        raise ValueError("clip must be [B,T,C,H,W] (ViViT, TimeSformer) or [B,C,T,H,W] (Swin3d, ResNet3d, VideoResNet50LSTM)")
    B = clip.shape[0]
    T = clip.shape[1] if layout == "btchw" else clip.shape[2]
    H, W = clip.shape[3], clip.shape[4]
    bits, shifts = rise_masks(T, H, W, cells, keep, masks, seed)  # checks cells, keep, masks and seed
    cells = _check_cells(cells, T, H, W)
    target = _targets(target, B, labels)
    if clip.device.type != "cuda":
        raise RuntimeError("RISE runs on the GPU only: move the clip batch to cuda")
    x = clip.detach().float().contiguous()
    n = default_chunk(model) if chunk is None else chunk
    bits, shifts = bits.to(x.device), shifts.to(x.device)
    acc = torch.zeros((B, T, H, W), dtype=torch.float32, device=x.device)
    rows, scores = [], []
    with torch.no_grad():
        # a family's forward may return its workspace buffer: every result is copied before the next forward
        whole = logits_of(model, x).detach().float().clone()
        if target is None:
            target = (whole[:, 0] > 0).long().tolist() if labels == 1 else whole.argmax(dim=1).tolist()
        base = ops.gaussian_blur_planes(x, BLUR_KSIZE, BLUR_SIGMA) if baseline == "blur" else None
        for f0 in range(0, masks, n):
            cb, cs = bits[f0:f0 + n], shifts[f0:f0 + n]
            F = cb.shape[0]
            flat = ops.rise_apply(x, cb, cs, cells, layout, base=base).view((F * B,) + tuple(x.shape[1:]))
            lg = torch.cat([logits_of(model, flat[i:i + n]).detach().float().cpu() for i in range(0, F * B, n)])
            lg = lg.reshape(F, B, -1).transpose(0, 1).contiguous()  # [B, F, labels]
            sc = _score(lg, target, labels)                         # [B, F]
            ops.rise_accumulate(acc, cb, cs, sc.t().contiguous().to(x.device), cells)
            rows.append(lg)
            scores.append(sc)
        acc = acc.cpu()
    total = acc.double().sum(dim=(1, 2, 3), keepdim=True)
    saliency = torch.where(total != 0, acc.double() / torch.where(total != 0, total, torch.ones_like(total)),
                           torch.zeros_like(acc, dtype=torch.float64)).float()
    relevance = (acc / (masks * float(keep))).reshape(B, -1)
    return RiseExplanation(whole, relevance, saliency, saliency.sum(dim=(2, 3)), target, torch.cat(rows, dim=1),
                           torch.cat(scores, dim=1), masks, cells, float(keep), seed, baseline)
