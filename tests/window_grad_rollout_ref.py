"""Reference side of the class-specific Video Swin saliency tests (test_window_grad_rollout_{cpu,gpu}.py), plain torch
on the CPU.  The geometry helpers, the fixture and `sharpen` are window_rollout_ref's.

  grad_step_ref     vc_window_grad_rollout_step's formula in a chosen dtype from bf16 q'|k|v and dO rows
  oracle_grads      the loop of oracle/swin3d_ref.swin3d_forward under autograd, keeping every block's probabilities P,
                    its v and its attention output O (before attn.proj) with retain_grad, then one backward of the
                    target logits: per block the dense head-mean of max(P * dP, 0) with dP = dO . v^T (the rule), and
                    autograd's own dlogit/dP beside it; optionally with q, k rounded to bf16 before every softmax and
                    v, dO rounded to bf16 before dP (the yardstick of the model bound)
  rollout_dense     the a / base rollout with the matrix products formed first
  rollout_stepwise  the same as vector steps and index hops, the way the GPU runs it: (a, base) at stage 0
  saliency          a / sum a per clip (all zero where the sum is exactly 0)
  E                 max|x - ref| / max|ref|, the error measure of the model tests (on the normalised maps)

MODEL_FACTOR: the model bound's factor over the bf16 yardstick; test_window_grad_rollout_gpu.py's docstring has the
measured ratios it comes from, and the CPU discrimination check uses the same figure.
"""
import math

import torch
import torch.nn.functional as F

import window_rollout_ref as R
from oracle import swin3d_ref as O

LOG2E = R.LOG2E
TINY = R.TINY
MODEL_FACTOR = 16.0


def bf16(x):
    return x.bfloat16().to(x.dtype)


def grad_step_ref(qkv, dout, table, r_in, a_in, B, grid, heads, window, shift, full_window, alpha, beta, dtype):
    """a_out of vc_window_grad_rollout_step in `dtype`: qkv bf16 [>= B*T*H*W, >= 3*heads*32] (q' pre-scaled, base 2),
    dout bf16 [>= B*T*H*W, >= heads*32], the bias table [ntab, heads] of the full window, r_in / a_in [B*T*H*W].  The
    rows past B*T*H*W and the columns past the ones named are not touched."""
    T, H, W = grid
    n = T * H * W
    C = heads * 32
    vol = window[0] * window[1] * window[2]
    rows = qkv[:B * n, :3 * C].to(dtype).reshape(B, T, H, W, -1)
    xw = R._partition(rows, window, shift)  # [B*nw, vol, 3C]
    part = lambda z: z.reshape(-1, vol, heads, 32).transpose(1, 2)  # noqa: E731
    q, k, v = part(xw[:, :, :C]), part(xw[:, :, C:2 * C]), part(xw[:, :, 2 * C:])
    do = part(R._partition(dout[:B * n, :C].to(dtype).reshape(B, T, H, W, -1), window, shift))
    bias = O.relative_position_bias(table.to(dtype), full_window, window)  # [heads, vol, vol]
    s = q @ k.transpose(-1, -2) + LOG2E * bias.unsqueeze(0)
    if sum(shift) > 0:
        s = s.masked_fill(R.region_mask(grid, window, shift).unsqueeze(1).repeat(B, 1, 1, 1), -math.inf)
    e = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    p = e / e.sum(dim=-1, keepdim=True)  # [B*nw, heads, vol, vol]
    dp = (do @ v.transpose(-1, -2)).clamp_min(0)
    rw = R._partition(r_in.to(dtype).reshape(B, T, H, W, 1), window, shift)[:, :, 0]  # [B*nw, vol]
    u = torch.einsum("wi,whij->wj", rw, p * dp) / heads
    u = R._unpartition(u.unsqueeze(-1), B, grid, window, shift).reshape(-1)
    return alpha * u + beta * a_in.to(dtype)


def _window_attention_kept(x, p, prefix, heads, full_window, shift_size, round16):
    """oracle/swin3d_ref.window_attention_3d keeping (P [b*nw, heads, vol, vol], v [b*nw, heads, vol, d], the attention
    output before attn.proj [b*nw, heads, vol, d]) in the graph: (block output [B, T, H, W, C], kept dict)"""
    b, t, h, w, c = x.shape
    window, shift = O.window_and_shift((t, h, w), full_window, shift_size)
    assert t % window[0] == 0 and h % window[1] == 0 and w % window[2] == 0, "whole windows only"
    vol = window[0] * window[1] * window[2]
    nw = t * h * w // vol
    bias = O.relative_position_bias(p[prefix + "relative_position_bias_table"], full_window, window)
    xw = R._partition(x, window, shift)
    qkv = F.linear(xw, p[prefix + "qkv.weight"], p[prefix + "qkv.bias"])
    qkv = qkv.reshape(xw.size(0), vol, 3, heads, c // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = q * (c // heads) ** -0.5
    if round16:
        q, k = bf16(q), bf16(k)
    s = q.matmul(k.transpose(-2, -1)) + bias.unsqueeze(0)
    if sum(shift) > 0:
        neg = torch.zeros(nw, vol, vol, dtype=s.dtype).masked_fill(R.region_mask((t, h, w), window, shift), -100.0)
        s = s + neg.unsqueeze(1).repeat(b, 1, 1, 1)
    attn = F.softmax(s, dim=-1)
    o = attn.matmul(v)
    if attn.requires_grad:
        attn.retain_grad()
    if o.requires_grad:
        o.retain_grad()
    out = F.linear(o.transpose(1, 2).reshape(b * nw, vol, c), p[prefix + "proj.weight"], p[prefix + "proj.bias"])
    out = R._unpartition(out, b, (t, h, w), window, shift)
    return out, dict(P=attn, v=v, o=o, tok=R.window_tokens((t, h, w), window, shift), b=b, nw=nw, vol=vol)


def oracle_grads(sd, cfg, video, target=None, dtype=torch.float32, round16=False):
    """(logits [B, classes], target list, grids, mats[stage][block] = dict(A = dense head-mean of max(P * dO.v^T, 0)
    fp64 [B, N_s, N_s], P, dP_rule = dO . v^T, dP_autograd = dlogit/dP as autograd gives it)).  target None: per clip
    the argmax.  round16: the bf16 yardstick (see the module docstring)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    eps = cfg.get("layer_norm_eps", 1e-5)
    pt, ph, pw = cfg["patch_size"]
    x = F.conv3d(video.to(dtype), sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=(pt, ph, pw))
    x = x.permute(0, 2, 3, 4, 1)
    x = F.layer_norm(x, (x.shape[-1],), sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"], eps)
    x = x.detach().requires_grad_()
    win = tuple(cfg["window_size"])
    grids, kept = [], []
    with torch.enable_grad():
        for s, depth in enumerate(cfg["depths"]):
            heads = cfg["num_heads"][s]
            grids.append(tuple(x.shape[1:4]))
            kept.append([])
            for i in range(depth):
                pre = f"features.{2 * s}.{i}."
                shift = [0 if i % 2 == 0 else k // 2 for k in win]
                y = F.layer_norm(x, (x.shape[-1],), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
                y, kd = _window_attention_kept(y, sd, pre + "attn.", heads, win, shift, round16)
                kept[-1].append(kd)
                x = x + y
                y = F.layer_norm(x, (x.shape[-1],), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], eps)
                y = F.gelu(F.linear(y, sd[pre + "mlp.0.weight"], sd[pre + "mlp.0.bias"]))
                x = x + F.linear(y, sd[pre + "mlp.3.weight"], sd[pre + "mlp.3.bias"])
            if s < len(cfg["depths"]) - 1:
                x = O.patch_merging(x, sd, f"features.{2 * s + 1}.", eps)
        x = F.layer_norm(x, (x.shape[-1],), sd["norm.weight"], sd["norm.bias"], eps)
        logits = F.linear(x.mean(dim=(1, 2, 3)), sd["head.weight"], sd["head.bias"])
        B = logits.shape[0]
        if target is None:
            target = logits.detach().argmax(dim=1).tolist()
        elif isinstance(target, int):
            target = [target] * B
        logits.gather(1, torch.tensor(target).reshape(-1, 1)).sum().backward()
    mats = []
    for s, st in enumerate(kept):
        mats.append([])
        n = grids[s][0] * grids[s][1] * grids[s][2]
        for kd in st:
            P, v, do = kd["P"].detach(), kd["v"].detach(), kd["o"].grad
            if round16:
                v, do = bf16(v), bf16(do)
            dP = do.matmul(v.transpose(-2, -1))
            A = (P.double() * dP.double().clamp_min(0)).mean(1).view(kd["b"], kd["nw"], kd["vol"], kd["vol"])
            mats[-1].append(dict(A=R.scatter_dense(A, kd["tok"], n), P=P, dP_rule=dP, dP_autograd=kd["P"].grad))
    return logits.detach(), target, grids, mats


def _seed(B, grids):
    t, h, w = grids[-1]
    return torch.full((B, t * h * w), 1.0 / (t * h * w), dtype=torch.float64)


def rollout_dense(mats, grids):
    """(a, base) fp64 [B, N_0] with the matrix products formed first: with total = Bm + Am (Bm the hops alone, Am the
    part through at least one attention), a step is Am <- Am + (Bm + Am) A and a hop multiplies both; then the uniform
    row times each."""
    B = mats[0][0]["A"].shape[0]
    n = grids[-1][0] * grids[-1][1] * grids[-1][2]
    Bm = torch.eye(n, dtype=torch.float64).expand(B, n, n).clone()
    Am = torch.zeros(B, n, n, dtype=torch.float64)
    for s in reversed(range(len(grids))):
        for d in reversed(mats[s]):
            Am = Am + (Bm + Am) @ d["A"]
        if s > 0:
            Hm = R.hop_matrix(grids[s - 1])
            Bm, Am = Bm @ Hm, Am @ Hm
    seed = _seed(B, grids).unsqueeze(1)
    return seed.matmul(Am)[:, 0], seed.matmul(Bm)[:, 0]


def rollout_stepwise(mats, grids, dtype=torch.float64):
    """(a, base) [B, N_0] as vector steps and index hops, last block first: a <- a + (base + a) A per block, spread(a)
    and spread(base) per hop"""
    B = mats[0][0]["A"].shape[0]
    base = _seed(B, grids).to(dtype)
    a = torch.zeros_like(base)
    for s in reversed(range(len(grids))):
        for d in reversed(mats[s]):
            a = a + torch.einsum("bi,bij->bj", base + a, d["A"].to(dtype))
        if s > 0:
            a = R.spread_ref(a.reshape(-1), B, grids[s - 1]).reshape(B, -1)
            base = R.spread_ref(base.reshape(-1), B, grids[s - 1]).reshape(B, -1)
    return a, base


def saliency(a):
    """a / sum a per clip in fp64 (all zero where the sum is exactly 0): [B, N_0]"""
    a = a.double()
    total = a.sum(dim=1, keepdim=True)
    return torch.where(total > 0, a / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(a))


def E(x, ref):
    return float((x.double() - ref.double()).abs().max() / ref.double().abs().max())
