"""Reference side of the Video Swin saliency tests (test_window_rollout_{cpu,gpu}.py), plain torch on the CPU.

  oracle_probs      the loop of oracle/swin3d_ref.swin3d_forward restated to keep every block's probabilities,
                    scattered as the head-mean into a dense [B, N_s, N_s] matrix in the token layout (row
                    (t*H + h)*W + w); optionally with q and k rounded to bf16 before each softmax (the yardstick of
                    the model bound), and with the wrong-rule variants of the discrimination check beside the right
                    one (the forward itself always runs the right rule)
  hop_matrix        PatchMerging's hop as a dense [N_s, N_{s-1}] matrix
  rollout_dense     the uniform row times the product of the dense step and hop matrices, the product formed
                    matrix by matrix
  rollout_stepwise  the same as vector steps and index hops, the way the GPU runs it
  step_ref          one block step's formula from bf16 q'|k rows, in a chosen dtype
  spread_ref        the hop by index
  sharpen           a state dict with sharper attention
  E                 the error measure of the model tests

MODEL_FACTOR is the model bound's factor over the bf16-q/k yardstick (test_window_rollout_gpu.py's docstring has the
measured ratios it comes from); the CPU discrimination check uses the same figure.
"""
import math

import torch
import torch.nn.functional as F

from oracle import swin3d_ref as O

LOG2E = 1.4426950408889634
MODEL_FACTOR = 8.0
TINY = dict(patch_size=(2, 4, 4), embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=(2, 3, 3),
            mlp_ratio=4.0, layer_norm_eps=1e-5, num_classes=2)
VARIANTS = ("ref", "no_shift", "no_bias")


def _partition(z, window, shift):
    """torchvision's roll by -shift and window partition: [b, t, h, w, c] -> [b * nw, vol, c]"""
    b, t, h, w, c = z.shape
    if sum(shift) > 0:
        z = torch.roll(z, shifts=(-shift[0], -shift[1], -shift[2]), dims=(1, 2, 3))
    z = z.view(b, t // window[0], window[0], h // window[1], window[1], w // window[2], window[2], c)
    return z.permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, window[0] * window[1] * window[2], c)


def _unpartition(z, b, thw, window, shift):
    t, h, w = thw
    c = z.shape[-1]
    z = z.view(b, t // window[0], h // window[1], w // window[2], window[0], window[1], window[2], c)
    z = z.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(b, t, h, w, c)
    if sum(shift) > 0:
        z = torch.roll(z, shifts=(shift[0], shift[1], shift[2]), dims=(1, 2, 3))
    return z


def window_tokens(thw, window, shift):
    """[nw, vol] token index (t*H + h)*W + w of every window slot, by the oracle's own roll and partition"""
    t, h, w = thw
    ids = torch.arange(t * h * w).view(1, t, h, w, 1)
    return _partition(ids, window, shift)[:, :, 0]


def region_mask(thw, window, shift):
    """[nw, vol, vol] bool: True where the two slots lie in different shift regions (torchvision adds -100 there)"""
    m = O.shift_region_labels(thw, window, shift).view(1, *thw, 1)
    m = _partition(m, window, [0, 0, 0])[:, :, 0]  # the labels are defined on the rolled grid
    return m.unsqueeze(1) != m.unsqueeze(2)


def scatter_dense(pm, tok, n):
    """head-mean probabilities [B, nw, vol, vol] fp64 -> dense [B, n, n] in the token layout"""
    dense = torch.zeros(pm.shape[0], n, n, dtype=torch.float64)
    for wi in range(tok.shape[0]):
        dense[:, tok[wi][:, None], tok[wi][None, :]] = pm[:, wi]
    return dense


def _window_attention_probs(x, p, prefix, heads, full_window, shift_size, round_qk, variants):
    """oracle/swin3d_ref.window_attention_3d keeping the probabilities: (attention output [B, T, H, W, C],
    {variant: dense head-mean [B, N, N] fp64})"""
    b, t, h, w, c = x.shape
    window, shift = O.window_and_shift((t, h, w), full_window, shift_size)
    assert t % window[0] == 0 and h % window[1] == 0 and w % window[2] == 0, "whole windows only"
    vol = window[0] * window[1] * window[2]
    nw = t * h * w // vol
    bias = O.relative_position_bias(p[prefix + "relative_position_bias_table"], full_window, window)
    xw = _partition(x, window, shift)
    qkv = F.linear(xw, p[prefix + "qkv.weight"], p[prefix + "qkv.bias"])
    qkv = qkv.reshape(xw.size(0), vol, 3, heads, c // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = q * (c // heads) ** -0.5
    if round_qk:
        q, k = q.bfloat16().float(), k.bfloat16().float()
    s = q.matmul(k.transpose(-2, -1))  # [b*nw, heads, vol, vol]
    shifted = sum(shift) > 0
    neg = None
    if shifted:
        neg = torch.zeros(nw, vol, vol).masked_fill(region_mask((t, h, w), window, shift), -100.0)
        neg = neg.unsqueeze(1).repeat(b, 1, 1, 1)  # [b*nw, 1, vol, vol]

    def soft(with_bias, with_mask):
        a = s + bias.unsqueeze(0) if with_bias else s
        if shifted and with_mask:
            a = a + neg
        return F.softmax(a, dim=-1)

    attn = soft(True, True)
    out = attn.matmul(v).transpose(1, 2).reshape(b * nw, vol, c)
    out = F.linear(out, p[prefix + "proj.weight"], p[prefix + "proj.bias"])
    out = _unpartition(out, b, (t, h, w), window, shift)
    tok = window_tokens((t, h, w), window, shift)
    dense = {}
    for name in variants:
        a = attn if name == "ref" else soft(name != "no_bias", name != "no_shift")
        dense[name] = scatter_dense(a.double().mean(1).view(b, nw, vol, vol), tok, t * h * w)
    return out, dense


def oracle_probs(sd, cfg, video, round_qk=False, variants=("ref",)):
    """(logits [B, classes], grids [(T_s, H_s, W_s)], mats[stage][block] = {variant: dense [B, N_s, N_s] fp64})"""
    eps = cfg.get("layer_norm_eps", 1e-5)
    pt, ph, pw = cfg["patch_size"]
    x = F.conv3d(video, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=(pt, ph, pw))
    x = x.permute(0, 2, 3, 4, 1)
    x = F.layer_norm(x, (x.shape[-1],), sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"], eps)
    win = tuple(cfg["window_size"])
    grids, mats = [], []
    for s, depth in enumerate(cfg["depths"]):
        heads = cfg["num_heads"][s]
        grids.append(tuple(x.shape[1:4]))
        mats.append([])
        for i in range(depth):
            pre = f"features.{2 * s}.{i}."
            shift = [0 if i % 2 == 0 else k // 2 for k in win]
            y = F.layer_norm(x, (x.shape[-1],), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
            y, dense = _window_attention_probs(y, sd, pre + "attn.", heads, win, shift, round_qk, variants)
            mats[-1].append(dense)
            x = x + y
            y = F.layer_norm(x, (x.shape[-1],), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], eps)
            y = F.gelu(F.linear(y, sd[pre + "mlp.0.weight"], sd[pre + "mlp.0.bias"]))
            x = x + F.linear(y, sd[pre + "mlp.3.weight"], sd[pre + "mlp.3.bias"])
        if s < len(cfg["depths"]) - 1:
            x = O.patch_merging(x, sd, f"features.{2 * s + 1}.", eps)
    x = F.layer_norm(x, (x.shape[-1],), sd["norm.weight"], sd["norm.bias"], eps)
    return F.linear(x.mean(dim=(1, 2, 3)), sd["head.weight"], sd["head.bias"]), grids, mats


def sharpen(sd, qk=4.0, table=8.0):
    """a copy of the state dict with the q and k rows of every attn.qkv weight and bias multiplied by `qk` and every
    relative-position bias table by `table`: the synthetic weights alone give almost uniform attention, under which a
    wrong rule cannot be told from the right one"""
    out = {k: v.clone() for k, v in sd.items()}
    for k, v in out.items():
        if k.endswith("attn.qkv.weight") or k.endswith("attn.qkv.bias"):
            v[:2 * (v.shape[0] // 3)] *= qk
        elif k.endswith("relative_position_bias_table"):
            v *= table
    return out


def hop_matrix(grid_child):
    """[N_parent, N_child] fp64: merged token (t, i, j) gives 1 / (number of existing children) to each child"""
    T, H, W = grid_child
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    M = torch.zeros(T * H2 * W2, T * H * W, dtype=torch.float64)
    for t in range(T):
        for i in range(H2):
            for j in range(W2):
                kids = [(2 * i + di, 2 * j + dj) for di in (0, 1) for dj in (0, 1) if 2 * i + di < H and 2 * j + dj < W]
                for hh, ww in kids:
                    M[(t * H2 + i) * W2 + j, (t * H + hh) * W + ww] = 1.0 / len(kids)
    return M


def spread_ref(r_parent, B, grid_child):
    """the hop by index: r_parent [B * T*H2*W2] -> [B * T*H*W], in r_parent's dtype"""
    T, H, W = grid_child
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    rp = r_parent.reshape(B, T, H2, W2)
    hi, wi = torch.arange(H) // 2, torch.arange(W) // 2
    cnt_h = torch.tensor([2 if 2 * i + 1 < H else 1 for i in range(H2)])[hi]
    cnt_w = torch.tensor([2 if 2 * j + 1 < W else 1 for j in range(W2)])[wi]
    cnt = (cnt_h[:, None] * cnt_w[None, :]).to(r_parent.dtype)
    return (rp[:, :, hi][:, :, :, wi] / cnt).reshape(-1)


def step_matrices(mats, alpha, variant="ref"):
    """[stage][block] dense step matrices alpha * A + (1 - alpha) * I, fp64 [B, N_s, N_s]"""
    out = []
    for st in mats:
        out.append([])
        for d in st:
            A = d[variant]
            out[-1].append(alpha * A + (1 - alpha) * torch.eye(A.shape[-1], dtype=torch.float64))
    return out


def rollout_dense(mats, grids, alpha=0.5, variant="ref"):
    """uniform row over the last stage times the matrix product of every step and hop, the product formed first:
    fp64 [B, N_0]"""
    steps = step_matrices(mats, alpha, variant)
    total = None
    for s in reversed(range(len(grids))):
        for M in reversed(steps[s]):
            total = M if total is None else total @ M
        if s > 0:
            total = total @ hop_matrix(grids[s - 1])
    n = total.shape[1]
    return torch.full((total.shape[0], 1, n), 1.0 / n, dtype=torch.float64).matmul(total)[:, 0]


def rollout_stepwise(mats, grids, alpha=0.5, variant="ref"):
    """the same as vector steps and index hops, last block first: fp64 [B, N_0]"""
    B = mats[0][0][variant].shape[0]
    t, h, w = grids[-1]
    r = torch.full((B, t * h * w), 1.0 / (t * h * w), dtype=torch.float64)
    for s in reversed(range(len(grids))):
        for d in reversed(mats[s]):
            r = alpha * torch.einsum("bi,bij->bj", r, d[variant]) + (1 - alpha) * r
        if s > 0:
            r = spread_ref(r.reshape(-1), B, grids[s - 1]).reshape(B, -1)
    return r


def step_ref(qkv, table, r_in, B, grid, heads, window, shift, full_window, alpha, dtype):
    """vc_window_rollout_step's formula in `dtype` from bf16 q'|k|v rows [>= B*T*H*W, >= 3*heads*32] (q' pre-scaled,
    base 2), the bias table [ntab, heads] of the full window and r_in [B*T*H*W]; window / shift the effective ones.
    Pairs of different shift regions are excluded outright.  The rows past B*T*H*W are not touched."""
    T, H, W = grid
    n = T * H * W
    C = heads * 32
    vol = window[0] * window[1] * window[2]
    rows = qkv[:B * n].to(dtype).reshape(B, T, H, W, -1)
    xw = _partition(rows, window, shift)  # [B*nw, vol, cols]
    q = xw[:, :, :C].reshape(-1, vol, heads, 32).transpose(1, 2)
    k = xw[:, :, C:2 * C].reshape(-1, vol, heads, 32).transpose(1, 2)
    bias = O.relative_position_bias(table.to(dtype), full_window, window)  # [heads, vol, vol]
    s = q @ k.transpose(-1, -2) + LOG2E * bias.unsqueeze(0)
    if sum(shift) > 0:
        s = s.masked_fill(region_mask(grid, window, shift).unsqueeze(1).repeat(B, 1, 1, 1), -math.inf)
    e = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    p = e / e.sum(dim=-1, keepdim=True)  # [B*nw, heads, vol, vol]
    rw = _partition(r_in.to(dtype).reshape(B, T, H, W, 1), window, shift)[:, :, 0]  # [B*nw, vol]
    u = torch.einsum("wi,whij->wj", rw, p) / heads
    u = _unpartition(u.unsqueeze(-1), B, grid, window, shift).reshape(-1)
    return alpha * u + (1 - alpha) * r_in.to(dtype)


def E(x, ref):
    """max|(x - u) - (ref - u)| / max|ref - u| with u = 1/N_0: the deviation from uniform is the signal"""
    u = 1.0 / ref.shape[-1]
    return float((x.double() - ref.double()).abs().max() / (ref.double() - u).abs().max())
