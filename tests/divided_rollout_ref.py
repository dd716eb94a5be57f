"""Reference side of the TimeSformer saliency tests (test_divided_rollout_{cpu,gpu}.py), plain torch on the CPU.

  oracle_probs        the per-layer loop of oracle/timesformer_ref.timesformer_forward restated to keep every layer's
                      temporal [B, P, H, T, T] and spatial [B, T, H, 1+P, 1+P] probabilities, optionally with q and k
                      rounded to bf16 before each softmax (the yardstick of the model bound)
  layer_matrices      the dense S x S matrices A_t and A_s of one layer (fp64)
  rollout_dense       the CLS row of prod_l (A_s A_t), from the dense matrices
  rollout_stepwise    the same as L vector-times-matrix steps in the frame layout, the way the GPU runs it
  cls_attention_row   the head-mean CLS attention row of the last layer's spatial attention
  temporal_step_ref   the temporal step's formula on bf16 q'|k|v rows, in a chosen dtype

Clip layout: S = 1 + P*T tokens, CLS then patch-major / time-minor, token (p, t) at 1 + p*T + t.
"""
import torch

from oracle.vivit_ref import layer_norm


def _attn_probs(x, wqkv, bqkv, H, round_qk):
    """oracle/timesformer_ref._attn keeping the probabilities: x [N, L, D] -> (context [N, L, D], a [N, H, L, L])"""
    N, L, D = x.shape
    qkv = (x @ wqkv.T + bqkv).reshape(N, L, 3, H, D // H).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    if round_qk:
        q, k = q.bfloat16().float(), k.bfloat16().float()
    a = torch.softmax((q @ k.transpose(-2, -1)) * (D // H) ** -0.5, dim=-1)
    return (a @ v).transpose(1, 2).reshape(N, L, D), a


def oracle_probs(sd, cfg, pixel_values, round_qk=False):
    """(logits [B, labels], [L] of (temporal [B, P, H, T, T], spatial [B, T, H, 1+P, 1+P]))"""
    D, H, ps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"]
    eps = cfg.get("layer_norm_eps", 1e-6)
    B, T, C, Hh, Ww = pixel_values.shape
    n = (Hh // ps) * (Ww // ps)
    e = "timesformer.embeddings."
    x = torch.nn.functional.conv2d(pixel_values.reshape(B * T, C, Hh, Ww), sd[e + "patch_embeddings.projection.weight"],
                                   sd[e + "patch_embeddings.projection.bias"], stride=ps)
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([sd[e + "cls_token"].expand(B * T, -1, -1), x], 1) + sd[e + "position_embeddings"]
    cls = x[:B, 0:1]
    x = x[:, 1:].reshape(B, T, n, D).permute(0, 2, 1, 3).reshape(B * n, T, D) + sd[e + "time_embeddings"]
    h = torch.cat([cls, x.reshape(B, n * T, D)], 1)
    probs = []
    for i in range(cfg["num_hidden_layers"]):
        p = f"timesformer.encoder.layer.{i}."
        te = h[:, 1:].reshape(B * n, T, D)
        y = layer_norm(te, sd[p + "temporal_layernorm.weight"], sd[p + "temporal_layernorm.bias"], eps)
        y, at = _attn_probs(y, sd[p + "temporal_attention.attention.qkv.weight"],
                            sd[p + "temporal_attention.attention.qkv.bias"], H, round_qk)
        y = y @ sd[p + "temporal_attention.output.dense.weight"].T + sd[p + "temporal_attention.output.dense.bias"]
        y = y.reshape(B, n * T, D) @ sd[p + "temporal_dense.weight"].T + sd[p + "temporal_dense.bias"]
        te = h[:, 1:] + y
        init_cls = h[:, 0:1]
        sp = te.reshape(B, n, T, D).permute(0, 2, 1, 3).reshape(B * T, n, D)
        sp = torch.cat([init_cls.repeat(1, T, 1).reshape(B * T, 1, D), sp], 1)
        y = layer_norm(sp, sd[p + "layernorm_before.weight"], sd[p + "layernorm_before.bias"], eps)
        y, as_ = _attn_probs(y, sd[p + "attention.attention.qkv.weight"], sd[p + "attention.attention.qkv.bias"], H,
                             round_qk)
        y = y @ sd[p + "attention.output.dense.weight"].T + sd[p + "attention.output.dense.bias"]
        cls_res = y[:, 0].reshape(B, T, D).mean(1, keepdim=True)
        res = y[:, 1:].reshape(B, T, n, D).permute(0, 2, 1, 3).reshape(B, n * T, D)
        h = torch.cat([init_cls, te], 1) + torch.cat([cls_res, res], 1)
        y = layer_norm(h, sd[p + "layernorm_after.weight"], sd[p + "layernorm_after.bias"], eps)
        y = torch.nn.functional.gelu(y @ sd[p + "intermediate.dense.weight"].T + sd[p + "intermediate.dense.bias"])
        h = h + y @ sd[p + "output.dense.weight"].T + sd[p + "output.dense.bias"]
        probs.append((at.reshape(B, n, H, T, T), as_.reshape(B, T, H, 1 + n, 1 + n)))
    seq = layer_norm(h, sd["timesformer.layernorm.weight"], sd["timesformer.layernorm.bias"], eps)
    return seq[:, 0] @ sd["classifier.weight"].T + sd["classifier.bias"], probs


def sharpen(sd, cfg, factor=4.0):
    """a copy of the state dict with the q and k rows of every ...attention.qkv.weight multiplied by `factor`:
    the synthetic weights give almost uniform attention, under which a wrong rule is hard to tell from the right one"""
    D = cfg["hidden_size"]
    out = {k: v.clone() for k, v in sd.items()}
    for k, v in out.items():
        if k.endswith("attention.qkv.weight"):
            v[:2 * D] *= factor
    return out


def layer_matrices(at, as_, alpha):
    """(A_t, A_s) fp64 [B, S, S] of one layer from its probabilities; every row sums to 1"""
    B, P, _, T, _ = at.shape
    S = 1 + P * T
    At, As = at.double().mean(2), as_.double().mean(2)  # [B, P, T, T], [B, T, 1+P, 1+P]
    eye = torch.eye(S, dtype=torch.float64)
    Mt = torch.zeros(B, S, S, dtype=torch.float64)
    Mt[:, 0, 0] = 1.0  # the temporal branch never updates CLS
    for p in range(P):
        lo = 1 + p * T
        Mt[:, lo:lo + T, lo:lo + T] = alpha * At[:, p] + (1 - alpha) * torch.eye(T, dtype=torch.float64)
    Ms = (1 - alpha) * eye.repeat(B, 1, 1)
    for t in range(T):
        cols = 1 + torch.arange(P) * T + t  # frame t's patch tokens in the clip layout
        A = As[:, t]
        Ms[:, cols[:, None], cols[None, :]] += alpha * A[:, 1:, 1:]
        Ms[:, cols, 0] += alpha * A[:, 1:, 0]
        Ms[:, 0, cols] += alpha / T * A[:, 0, 1:]  # the per-frame CLS outputs are averaged
        Ms[:, 0, 0] += alpha / T * A[:, 0, 0]
    return Mt, Ms


def rollout_dense(probs, alpha=0.5):
    """the CLS row of prod_l (A_s A_t), last layer leftmost: fp64 [B, S]"""
    r = None
    for at, as_ in reversed(probs):
        Mt, Ms = layer_matrices(at, as_, alpha)
        M = Ms @ Mt
        r = M[:, 0, :] if r is None else torch.einsum("bi,bij->bj", r, M)
    return r


def rollout_stepwise(probs, alpha=0.5):
    """the same row as L times (spatial step, temporal step) on the frame layout [B, T, 1+P]: fp64 [B, S]"""
    B, P, _, T, _ = probs[0][0].shape
    rf = torch.zeros(B, T, 1 + P, dtype=torch.float64)
    rf[:, :, 0] = 1.0 / T
    clip = None
    for at, as_ in reversed(probs):
        At, As = at.double().mean(2), as_.double().mean(2)
        rf = alpha * torch.einsum("bti,btij->btj", rf, As) + (1 - alpha) * rf
        x = rf[:, :, 1:]  # [B, T, P]
        y = alpha * torch.einsum("btp,bptk->bpk", x, At) + (1 - alpha) * x.transpose(1, 2)  # [B, P, T']
        c = rf[:, :, 0].sum(1)
        clip = torch.cat([c[:, None], y.reshape(B, P * T)], 1)
        rf = torch.cat([(c / T)[:, None, None].expand(B, T, 1), y.transpose(1, 2)], 2)
    return clip


def cls_attention_row(probs):
    """CLS: (1/T) sum_t A_s^t[0, 0]; patch (p, t): A_s^t[0, 1+p] / T, of the last layer: fp64 [B, S]"""
    As = probs[-1][1].double().mean(2)  # [B, T, 1+P, 1+P]
    B, T = As.shape[:2]
    row = As[:, :, 0, :] / T  # [B, T, 1+P]
    return torch.cat([row[:, :, 0].sum(1, keepdim=True), row[:, :, 1:].transpose(1, 2).reshape(B, -1)], 1)


def temporal_step_ref(qkv, r_frame, B, P, T, H, alpha, dtype):
    """vc_temporal_rollout_step's formula in `dtype` from bf16 q'|k|v rows in the clip layout and r_frame [B*T, 1+P]:
    (r_clip [B, 1+P*T], r_frame_out [B*T, 1+P]).  The CLS rows and the rows past B*S are not touched."""
    S = 1 + P * T
    rows = torch.stack([qkv[b * S + 1:(b + 1) * S] for b in range(B)]).to(dtype)  # [B, P*T, 3*H*64]
    x = rows.reshape(B, P, T, 3, H, 64)
    q, k = x[:, :, :, 0].transpose(2, 3), x[:, :, :, 1].transpose(2, 3)  # [B, P, H, T, 64]
    s = q @ k.transpose(-1, -2)
    e = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    p = e / e.sum(dim=-1, keepdim=True)  # [B, P, H, T, T']
    rf = r_frame.to(dtype).reshape(B, T, 1 + P)
    xr = rf[:, :, 1:]  # [B, T, P]
    y = alpha * torch.einsum("btp,bphtk->bpk", xr, p) / H + (1 - alpha) * xr.transpose(1, 2)
    c = rf[:, 0, 0].clone()
    for t in range(1, T):  # in t order
        c = c + rf[:, t, 0]
    clip = torch.cat([c[:, None], y.reshape(B, P * T)], 1)
    frame = torch.cat([(c / T)[:, None, None].expand(B, T, 1), y.transpose(1, 2)], 2).reshape(B * T, 1 + P)
    return clip, frame
