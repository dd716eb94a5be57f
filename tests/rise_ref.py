"""Plain-torch float64 reference of RISE saliency (vclip_amd/rise.py, csrc/rise.hip): the host sampler, the mask by
its definition, the masked clips and the weighted mask sum.  Everything here is exact arithmetic on small integers up
to the final float64 roundings: the fractions are u % S / S in float64, the interpolation is a + f * (b - a) in
float64 in the order x, y, t."""
import torch

LAYOUTS = ("btchw", "bcthw")
# The planted scorer's seed.  Seed 0 does not satisfy the two properties on this reference (256 masks leave one frame's
# argmax outside the box); seeds 1, 2 and 3 do.  Chosen here, on the CPU reference, before any kernel ran.
PLANTED_SEED = 1


def cell_sizes(T, H, W, cells):
    return tuple((n + c - 1) // c for n, c in zip((T, H, W), cells))


def sample(T, H, W, cells, keep, masks, seed):
    """(bits uint8 [masks, ct+2, ch+2, cw+2], shifts int32 [masks, 3]): one generator; all the bits first (float32
    uniforms below `keep`), then one randint per axis in the order t, y, x"""
    g = torch.Generator().manual_seed(seed)
    ct, ch, cw = cells
    u = torch.rand((masks, ct + 2, ch + 2, cw + 2), generator=g, dtype=torch.float32)
    bits = (u < keep).to(torch.uint8)
    cols = [torch.randint(0, s, (masks,), generator=g) for s in cell_sizes(T, H, W, cells)]
    return bits, torch.stack(cols, dim=1).to(torch.int32)


def _axis(n, d, S):
    u = torch.arange(n, dtype=torch.int64) + int(d)
    return u // S, (u % S).double() / float(S)


def mask(bits, shifts, n, T, H, W, cells):
    """m_n f64 [T, H, W]"""
    St, Sh, Sw = cell_sizes(T, H, W, cells)
    g = bits[n].double()
    dt, dy, dx = (int(v) for v in shifts[n])
    assert 0 <= dt < St and 0 <= dy < Sh and 0 <= dx < Sw
    i, ft = _axis(T, dt, St)
    j, fy = _axis(H, dy, Sh)
    k, fx = _axis(W, dx, Sw)
    I, J, K = i[:, None, None], j[None, :, None], k[None, None, :]
    FT, FY, FX = ft[:, None, None], fy[None, :, None], fx[None, None, :]

    def lerp(f, a, b):
        return a + f * (b - a)

    a00 = lerp(FX, g[I, J, K], g[I, J, K + 1])
    a01 = lerp(FX, g[I, J + 1, K], g[I, J + 1, K + 1])
    a10 = lerp(FX, g[I + 1, J, K], g[I + 1, J, K + 1])
    a11 = lerp(FX, g[I + 1, J + 1, K], g[I + 1, J + 1, K + 1])
    return lerp(FT, lerp(FY, a00, a01), lerp(FY, a10, a11))


def corners_equal(bits, shifts, n, T, H, W, cells):
    """bool [T, H, W]: the eight corner bits of the pixel under mask n are all the same"""
    St, Sh, Sw = cell_sizes(T, H, W, cells)
    g = bits[n].long()
    i = (torch.arange(T) + int(shifts[n, 0])) // St
    j = (torch.arange(H) + int(shifts[n, 1])) // Sh
    k = (torch.arange(W) + int(shifts[n, 2])) // Sw
    I, J, K = i[:, None, None], j[None, :, None], k[None, None, :]
    s = sum(g[I + a, J + b, K + c] for a in (0, 1) for b in (0, 1) for c in (0, 1))
    return (s == 0) | (s == 8)


def masks_all(bits, shifts, T, H, W, cells):
    """f64 [F, T, H, W]"""
    return torch.stack([mask(bits, shifts, n, T, H, W, cells) for n in range(bits.shape[0])])


def _spread(m, layout):
    """[F, T, H, W] -> broadcastable against [F, B, <clip layout>]"""
    return m[:, None, :, None] if layout == "btchw" else m[:, None, None]


def apply(clip, base, m, layout):
    """f64 [F, B, <clip layout>] = m * clip + (1 - m) * base (base None: zeros), m f64 [F, T, H, W]"""
    mm = _spread(m, layout)
    x = clip.double()[None]
    out = mm * x
    if base is not None:
        out = out + (1.0 - mm) * base.double()[None]
    return out


def accumulate(acc, m, w):
    """f64 [B, T, H, W] = acc + sum_f w[f][b] * m[f];  w [F, B], m f64 [F, T, H, W]"""
    return acc.double() + torch.einsum("fb,fthw->bthw", w.double(), m)


def planted(seed, shape=(1, 3, 4, 32, 32), cells=(2, 4, 4), masks=256, keep=0.5, box=(8, 20, 10, 22)):
    """The planted scorer: a clip of ones [B, C, T, H, W]; the score of a masked clip is its mean inside the box
    (rows y0..y1-1, columns x0..x1-1, every frame and channel).  Returns (bits, shifts, scores f64 [F, B], map f64
    [B, T, H, W])."""
    B, C, T, H, W = shape
    bits, shifts = sample(T, H, W, cells, keep, masks, seed)
    m = masks_all(bits, shifts, T, H, W, cells)
    masked = apply(torch.ones(shape), None, m, "bcthw")
    y0, y1, x0, x1 = box
    scores = masked[..., y0:y1, x0:x1].mean(dim=(2, 3, 4, 5))
    return bits, shifts, scores, accumulate(torch.zeros(B, T, H, W), m, scores)


def planted_holds(sal, box=(8, 20, 10, 22)):
    """the two properties asked of a planted map [B, T, H, W]: every frame's argmax lies in the box, and the mean
    inside the box exceeds the mean outside"""
    y0, y1, x0, x1 = box
    B, T, H, W = sal.shape
    flat = sal.reshape(B, T, H * W).argmax(dim=2)
    ys, xs = flat // W, flat % W
    inside = bool(((ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)).all())
    sel = torch.zeros(H, W, dtype=torch.bool)
    sel[y0:y1, x0:x1] = True
    return inside and bool((sal[..., sel].mean(dim=2) > sal[..., ~sel].mean(dim=2)).all())
