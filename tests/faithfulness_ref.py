"""Plain-torch CPU reference of the saliency faithfulness test (vclip_amd/faithfulness.py, csrc/perturb.hip): the cell
of every pixel, the perturbed clips by indexing, the separable Gaussian blur as F.conv2d on replicate-padded planes in a
chosen dtype, and the trapezoid.  Nothing here calls the package."""
import math

import torch
import torch.nn.functional as F

LAYOUTS = ("btchw", "bcthw")


def cell_index(T, H, W, grid):
    """int64 [T, H, W]: the cell ((t*Tg//T)*Hg + y*Hg//H)*Wg + x*Wg//W of every pixel"""
    Tg, Hg, Wg = grid
    t = torch.arange(T) * Tg // T
    y = torch.arange(H) * Hg // H
    x = torch.arange(W) * Wg // W
    return (t[:, None, None] * Hg + y[None, :, None]) * Wg + x[None, None, :]


def ranks_of(saliency):
    """int32 [B, N]: rank[b, cell] = position of the cell in the stable descending order of saliency [B, ...]"""
    flat = saliency.reshape(saliency.shape[0], -1)
    out = torch.empty(flat.shape, dtype=torch.int32)
    for b in range(flat.shape[0]):
        order = sorted(range(flat.shape[1]), key=lambda c: (-float(flat[b, c]), c))
        for pos, c in enumerate(order):
            out[b, c] = pos
    return out


def step_counts(N, steps):
    return [(i * N) // steps for i in range(steps + 1)]


def perturb(clip, base, rank, k, grid, layout, mode):
    """[F, *clip.shape] by indexing: clip [B,T,C,H,W] ("btchw") or [B,C,T,H,W] ("bcthw"), base the same or None (0.0),
    rank int [B, N], k a list of F ints"""
    B = clip.shape[0]
    T = clip.shape[1] if layout == "btchw" else clip.shape[2]
    H, W = clip.shape[3:]
    cell = cell_index(T, H, W, grid)
    r = torch.stack([rank[b].long()[cell] for b in range(B)])  # [B, T, H, W]
    r = r[:, :, None] if layout == "btchw" else r[:, None]     # broadcast over the channels
    base = torch.zeros_like(clip) if base is None else base
    out = []
    for kf in k:
        touched = (r < kf).expand_as(clip)
        out.append(torch.where(touched, base, clip) if mode == "deletion" else torch.where(touched, clip, base))
    return torch.stack(out)


def taps(ksize, sigma):
    """f32 [ksize]: exp(-d^2 / (2 sigma^2)) / sum in double, rounded"""
    s = float(torch.tensor(float(sigma), dtype=torch.float32))
    w = [math.exp(-(float(j - ksize // 2) ** 2) / (2.0 * s * s)) for j in range(ksize)]
    tot = 0.0
    for v in w:
        tot += v
    return torch.tensor([v / tot for v in w], dtype=torch.float64).float()


def blur(x, w, dtype):
    """x [..., H, W] blurred with the f32 taps w along W, then along H, edges replicated, computed in `dtype`"""
    H, W = x.shape[-2:]
    R = w.numel() // 2
    z = x.reshape(-1, 1, H, W).to(dtype)
    wd = w.to(dtype)

    def pad(t, dim):  # replicate by index: F.pad's replicate mode refuses a pad wider than the plane
        n = t.shape[dim]
        return t.index_select(dim, (torch.arange(n + 2 * R) - R).clamp(0, n - 1))

    z = F.conv2d(pad(z, 3), wd.reshape(1, 1, 1, -1))
    z = F.conv2d(pad(z, 2), wd.reshape(1, 1, -1, 1))
    return z.reshape(x.shape)


def trapezoid(score, fractions):
    y, x = score.double(), fractions.double()
    return ((x[1:] - x[:-1]) * (y[:, 1:] + y[:, :-1]) / 2.0).sum(dim=1)
