"""ViViT saliency on the GPU: the rollout-step kernel (csrc/attention_rollout.hip) against a materialised fp64
evaluation of the same formula, and VivitForVideoClassification.explain against attention rollout computed from
the fp32 oracle's materialised attentions (the per-layer loop of oracle/vivit_ref.vivit_forward, keeping `a`).

Bounds (measured figures: DESIGN.md section 4):
  kernel  max|r_out - ref64| / max|ref64| <= 8 x the same formula in fp32 torch on the CPU against ref64, per
          shape: the inputs are identical, so only the exp2 rounding and the summation order differ;
  model   max|token_relevance - ref| / max|ref| <= 4 x the oracle with q and k rounded to bf16 before every
          softmax against the unrounded oracle: the GPU's hidden states also carry the bf16 GEMM rounding.
"""
import json
import os

import numpy as np
import pytest
import torch

from vclip_amd import ops
from vclip_amd.weights import make_synthetic_clips, make_vivit_weights

pytestmark = pytest.mark.gpu
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN16 = 0x7FC0  # a bf16 quiet NaN


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# ------------------------------------------------------------------ kernel: reference and inputs
def make_qkv(B, S, H, seed, pad_nan=True):
    """bf16 q'|k|v rows b*S + i (scores q'.k of about +-15) plus padding rows (NaN or zero)"""
    g = torch.Generator().manual_seed(seed)
    rows = (B * S + 63) // 64 * 64 + 64
    x = torch.randn(rows, 3 * H * 64, generator=g)
    x[:, :H * 64] *= 0.45  # q': the dot product over 64 dims then has a standard deviation of 3.6, extremes +-15..20
    x = x.to(torch.bfloat16)
    if pad_nan:
        x.view(torch.int16)[B * S:] = torch.tensor(NAN16, dtype=torch.int16)
    else:
        x[B * S:] = 0
    return x


def scores(qkv, B, S, H, dtype):
    """q'.k per (clip, head): [B, H, S, S] in `dtype` from the bf16 values"""
    x = qkv[:B * S].to(dtype).reshape(B, S, 3, H, 64)
    q, k = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2)
    return q @ k.transpose(2, 3)


def lse2_of(qkv, B, S, H):
    """the base-2 log-sum-exp in fp64, rounded to the f32 the kernel reads: [B*H*S]"""
    s = scores(qkv, B, S, H, torch.float64)
    m = s.max(dim=-1, keepdim=True).values
    return (m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))).reshape(-1).float()


def step_ref(qkv, lse, r_in, B, S, H, alpha, dtype):
    """the rollout step's formula, materialised, in `dtype` on the CPU"""
    p = torch.exp2(scores(qkv, B, S, H, dtype) - lse.to(dtype).reshape(B, H, S, 1))
    u = torch.einsum("bi,bhij->bj", r_in.to(dtype), p) / H
    return alpha * u + (1 - alpha) * r_in.to(dtype)


def r_inputs(B, S, seed):
    e = torch.zeros(B, S)
    e[:, 0] = 1.0
    g = torch.Generator().manual_seed(seed)
    return {"e_cls": e, "random": torch.rand(B, S, generator=g) + 0.05}


def run_step(qkv_d, lse_d, r_in, B, S, H, alpha):
    work = ops.attention_rollout_work(B, S, H, "cuda")
    out = torch.full((B, S), float("nan"), device="cuda")
    ops.attention_rollout_step(qkv_d, lse_d, r_in.cuda(), B, S, H, alpha, work, out)
    return out.cpu()


def check_against_fp64(qkv, lse, B, S, H, what):
    """every (r_in, alpha) case of one shape: finite, and within 8 x the shape's fp32 yardstick of fp64"""
    qkv_d, lse_d = qkv.cuda(), lse.cuda()
    errs, yard = {}, 0.0
    for name, r in r_inputs(B, S, seed=S).items():
        for alpha in (1.0, 0.5):
            ref = step_ref(qkv, lse, r, B, S, H, alpha, torch.float64)
            yard = max(yard, rel_err(step_ref(qkv, lse, r, B, S, H, alpha, torch.float32), ref))
            got = run_step(qkv_d, lse_d, r, B, S, H, alpha)
            assert torch.isfinite(got).all(), (what, name, alpha)
            errs[(name, alpha)] = rel_err(got, ref)
    print(f"rollout step {what} (B, S, H) = {(B, S, H)}: fp32 yardstick {yard:.3e}, kernel "
          + ", ".join(f"{k[0]}/a={k[1]}: {v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) <= 8 * yard, (errs, yard)


# ------------------------------------------------------------------ 1. kernel against materialised fp64
@pytest.mark.parametrize("B,S,H", [(1, 33, 2), (3, 65, 1), (1, 197, 3), (2, 321, 12)])
def test_rollout_step_matches_fp64(B, S, H):
    """partial 64-row tiles at every S (65 and 321 leave one row), another clip's rows in the overhang at
    B > 1, NaN in the padding rows past B*S"""
    qkv = make_qkv(B, S, H, seed=B * 1000 + S)
    check_against_fp64(qkv, lse2_of(qkv, B, S, H), B, S, H, "fp64 lse")


# ------------------------------------------------------------------ 2. pairing with the real forward
def test_rollout_step_pairs_with_attention_fwd_lse():
    B, S, H = 2, 197, 3
    qkv = make_qkv(B, S, H, seed=7, pad_nan=False)
    qkv_d = qkv.cuda()
    o = torch.zeros(qkv.shape[0], H * 64, dtype=torch.bfloat16, device="cuda")
    lse_d = torch.zeros(B * H * S, device="cuda")
    ops.attention_fwd_lse(qkv_d, B, S, H, o, lse_d)
    for name, r in r_inputs(B, S, seed=3).items():
        u = run_step(qkv_d, lse_d, r, B, S, H, 1.0)  # alpha = 1: r_out = u
        got, want = u.double().sum(1), r.double().sum(1)
        print(f"rollout step with the forward's lse, {name}: sum_j u {got.tolist()} sum_i r_in {want.tolist()}")
        # rows of the recomputed P sum to one up to exp2 rounding and order
        assert ((got - want).abs() <= 1e-3 * want).all(), (name, got, want)
    check_against_fp64(qkv, lse_d.cpu(), B, S, H, "forward's lse")


# ------------------------------------------------------------------ 3. determinism, batch invariance
def test_rollout_step_deterministic_and_batch_invariant():
    B, S, H = 3, 197, 3
    qkv = make_qkv(B, S, H, seed=11)
    lse = lse2_of(qkv, B, S, H)
    r = r_inputs(B, S, seed=5)["random"]
    a = run_step(qkv.cuda(), lse.cuda(), r, B, S, H, 0.5)
    b = run_step(qkv.cuda(), lse.cuda(), r, B, S, H, 0.5)
    assert torch.equal(a, b)
    one = make_qkv(1, S, H, seed=0)
    one[:S] = qkv[S:2 * S]
    c = run_step(one.cuda(), lse.reshape(B, H * S)[1].contiguous().cuda(), r[1:2].contiguous(), 1, S, H, 0.5)
    assert torch.equal(a[1:2], c)


# ------------------------------------------------------------------ 4. model against the fp32 oracle
def oracle_attentions(sd, cfg, pix, round_qk=False):
    """oracle/vivit_ref.vivit_forward's per-layer loop, keeping every layer's `a`: (logits, [L] of [B, H, S, S]).
    round_qk: q and k rounded to bf16 before the softmax (the yardstick of the model bound)."""
    from oracle.vivit_ref import gelu_fast, layer_norm
    D, H = cfg["hidden_size"], cfg["num_attention_heads"]
    hd = D // H
    eps = cfg.get("layer_norm_eps", 1e-6)
    kt, kh, kw = cfg["tubelet_size"]
    B = pix.shape[0]
    emb = torch.nn.functional.conv3d(pix.transpose(1, 2), sd["vivit.embeddings.patch_embeddings.projection.weight"],
                                     sd["vivit.embeddings.patch_embeddings.projection.bias"], stride=(kt, kh, kw))
    emb = emb.flatten(2).transpose(1, 2)
    h = torch.cat([sd["vivit.embeddings.cls_token"].expand(B, -1, -1), emb], dim=1) + sd["vivit.embeddings.position_embeddings"]
    S = h.shape[1]
    scale = hd ** -0.5
    attn = []
    for i in range(cfg["num_hidden_layers"]):
        p = f"vivit.layers.{i}."
        r = h
        y = layer_norm(h, sd[p + "layernorm_before.weight"], sd[p + "layernorm_before.bias"], eps)

        def proj(nm, t):
            return t @ sd[p + f"attention.{nm}.weight"].T + sd[p + f"attention.{nm}.bias"]

        q = proj("q_proj", y).view(B, S, H, hd).transpose(1, 2)
        k = proj("k_proj", y).view(B, S, H, hd).transpose(1, 2)
        v = proj("v_proj", y).view(B, S, H, hd).transpose(1, 2)
        if round_qk:
            q, k = q.bfloat16().float(), k.bfloat16().float()
        a = torch.softmax((q @ k.transpose(2, 3)) * scale, dim=-1, dtype=torch.float32)
        attn.append(a)
        o = (a @ v).transpose(1, 2).reshape(B, S, D)
        h = proj("o_proj", o) + r
        r = h
        y = layer_norm(h, sd[p + "layernorm_after.weight"], sd[p + "layernorm_after.bias"], eps)
        y = gelu_fast(y @ sd[p + "mlp.fc1.weight"].T + sd[p + "mlp.fc1.bias"])
        h = y @ sd[p + "mlp.fc2.weight"].T + sd[p + "mlp.fc2.bias"] + r
    seq = layer_norm(h, sd["vivit.layernorm.weight"], sd["vivit.layernorm.bias"], eps)
    return seq[:, 0, :] @ sd["classifier.weight"].T + sd["classifier.bias"], attn


def relevance_ref(attn, method, residual=0.5):
    """the CLS row of prod_l (residual A_l + (1 - residual) I), A_l the head mean, last layer first (fp64)"""
    mean = [a.double().mean(1) for a in attn]
    if method == "cls_attention":
        return mean[-1][:, 0, :]
    r = torch.zeros_like(mean[0][:, 0, :])
    r[:, 0] = 1.0
    for A in reversed(mean):
        r = residual * torch.einsum("bi,bij->bj", r, A) + (1 - residual) * r
    return r


def _tiny():
    g = np.load(os.path.join(GD, "vivit_tiny.npz"))
    return json.loads(str(g["config"])), torch.from_numpy(g["pixel_values"]), torch.from_numpy(g["logits"])


def _multi_tile():
    cfg = dict(image_size=96, num_frames=8, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=128,
               num_hidden_layers=3, num_attention_heads=2, intermediate_size=256, hidden_act="gelu_fast",
               layer_norm_eps=1e-6, qkv_bias=True)
    return cfg, torch.from_numpy(make_synthetic_clips(2, 8, 96, seed=1)), None


def _model(cfg):
    from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
    m = VivitForVideoClassification(VivitConfig(**cfg, id2label={0: "non-referral", 1: "referral"}))
    m.load_state_dict(make_vivit_weights(cfg, seed=0))
    return m.cuda().eval()


@pytest.fixture(scope="module", params=["tiny", "multi_tile"])
def case(request):
    """(cfg, pix, logits to match, model, the oracle's attentions unrounded and with bf16 q / k), made once"""
    cfg, pix, want = _tiny() if request.param == "tiny" else _multi_tile()
    sd = {k: torch.from_numpy(v) for k, v in make_vivit_weights(cfg, seed=0).items()}
    with torch.no_grad():
        logits, attn = oracle_attentions(sd, cfg, pix)
        _, attn16 = oracle_attentions(sd, cfg, pix, round_qk=True)
    return cfg, pix, logits if want is None else want, _model(cfg), attn, attn16


@pytest.mark.parametrize("method", ["rollout", "cls_attention"])
def test_explain_matches_oracle_rollout(case, method):
    cfg, pix, want_logits, m, attn, attn16 = case
    ex = m.explain(pix.cuda(), method=method, residual=0.5)
    B = pix.shape[0]
    kt, kh, kw = cfg["tubelet_size"]
    grid = (cfg["num_frames"] // kt, cfg["image_size"] // kh, cfg["image_size"] // kw)
    S = 1 + grid[0] * grid[1] * grid[2]
    assert tuple(ex.token_relevance.shape) == (B, S) and tuple(ex.saliency.shape) == (B, *grid)
    assert tuple(ex.temporal.shape) == (B, grid[0]) and tuple(ex.logits.shape) == (B, 2)
    assert all(t.dtype == torch.float32 for t in (ex.logits, ex.token_relevance, ex.saliency, ex.temporal))
    assert float((ex.logits.cpu() - want_logits).abs().max()) < 1e-2
    assert torch.isfinite(ex.token_relevance).all() and (ex.saliency >= 0).all()
    assert ((ex.saliency.double().sum(dim=(1, 2, 3)) - 1).abs() < 1e-5).all()
    if method == "rollout":
        assert ((ex.token_relevance.double().sum(1) - 1).abs() < 5e-3).all()  # the compounded row-sum error
    assert torch.equal(ex.temporal, ex.saliency.sum(dim=(2, 3)))
    patch = ex.token_relevance[:, 1:].double()
    assert torch.allclose(ex.saliency.double().reshape(B, -1), patch / patch.sum(1, keepdim=True), rtol=1e-6, atol=0)
    ref = relevance_ref(attn, method)
    yard = rel_err(relevance_ref(attn16, method), ref)
    err = rel_err(ex.token_relevance, ref)
    print(f"explain {method} S = {S} L = {cfg['num_hidden_layers']}: bf16 q/k oracle yardstick {yard:.3e}, GPU {err:.3e}")
    assert err <= 4 * yard, (err, yard)


# ------------------------------------------------------------------ 5. refusals, the forward untouched
def test_explain_refusals_and_forward_untouched():
    cfg, pix, _ = _tiny()
    m = _model(cfg)
    pix = pix.cuda()
    before = m(pixel_values=pix).logits.clone()
    m.explain(pix)
    assert torch.equal(m(pixel_values=pix).logits, before)
    m.graph_replay = True
    assert torch.equal(m(pixel_values=pix).logits, before)
    captures = m._graphs.captures
    m.explain(pix, method="cls_attention")
    assert torch.equal(m(pixel_values=pix).logits, before)
    assert m._graphs.captures == captures  # explain invalidated nothing
    m.graph_replay = False
    m.compute_dtype = torch.float16
    with pytest.raises(RuntimeError, match="bfloat16"):
        m.explain(pix)
    m.compute_dtype = torch.bfloat16
    m.precise_layers = 1
    with pytest.raises(RuntimeError, match="precise_layers"):
        m.explain(pix)
    m.precise_layers = 0
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.explain(pix)
    m.eval()
    with pytest.raises(ValueError, match="method"):
        m.explain(pix, method="gradcam")
    assert torch.equal(m(pixel_values=pix).logits, before)


# ------------------------------------------------------------------ 6. full size once
def test_explain_vivit_b_full_size_memory():
    """ViViT-B/16x2 at B = 1: finite, the sums hold, and the call's extra device memory stays under 400 MB
    (184 MB of kept q|k|v, the lse, the partials): an S x S or H x S x S buffer would blow through it."""
    with open(os.path.join(GD, "vivit_full.json")) as f:
        cfg = json.load(f)["config"]
    m = _model(cfg)
    pix = torch.from_numpy(make_synthetic_clips(1, cfg["num_frames"], cfg["image_size"], seed=3)).cuda()
    m(pixel_values=pix)  # the packed weights and the forward's workspace exist before the measurement
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ex = m.explain(pix, method="rollout")
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"explain ViViT-B B = 1: peak extra device memory {extra / 1e6:.1f} MB")
    assert extra < 400e6, extra
    assert tuple(ex.saliency.shape) == (1, 16, 14, 14)
    assert torch.isfinite(ex.token_relevance).all() and torch.isfinite(ex.logits).all()
    assert (ex.saliency >= 0).all()
    assert abs(float(ex.saliency.double().sum()) - 1) < 1e-5
    assert abs(float(ex.token_relevance.double().sum()) - 1) < 5e-3
    assert torch.equal(ex.temporal, ex.saliency.sum(dim=(2, 3)))
