"""The class-specific ViViT saliency on the GPU: the gradient-weighted rollout step (csrc/attention_rollout.hip)
against a materialised fp64 evaluation of its formula, and explain(method="grad_rollout") against the rule of
Chefer, Gur & Wolf (2021) evaluated with autograd over the fp32 oracle's per-layer loop
(oracle/vivit_ref.vivit_forward), which materialises every attention matrix.

Bounds (measured figures: DESIGN.md section 4):
  kernel  max|r_out - ref64| / max|ref64| <= 8 x the same formula in fp32 torch on the CPU against ref64, per
          shape (the sibling rollout step's bound): the inputs are identical in all three;
  model   on the patch entries (the CLS entry is about 1 and would hide them), max|rel - ref| / max|ref| <=
          MODEL_FACTOR x the same oracle with q, k, v and dO rounded to bf16 before the layer matrices are formed.
          The GPU also carries the bf16 GEMM rounding of the forward and of the whole gradient chain, so the
          factor is not derivable: it is the smallest power of two at least twice the largest ratio measured over
          the four (fixture, target) cases: 1.72, 2.13 (S = 33, L = 2, targets 0, 1) and 3.28, 1.67 (S = 145,
          L = 3), so 8.  The forward-only rollout uses 4.
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
MODEL_FACTOR = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# ------------------------------------------------------------------ kernel: reference and inputs
def make_qkv(B, S, H, seed, pad_nan=True):
    """bf16 q'|k|v rows b*S + i (scores q'.k of about +-15) plus padding rows (NaN or zero): the generator of
    tests/test_rollout_gpu.py"""
    g = torch.Generator().manual_seed(seed)
    rows = (B * S + 63) // 64 * 64 + 64
    x = torch.randn(rows, 3 * H * 64, generator=g)
    x[:, :H * 64] *= 0.45
    x = x.to(torch.bfloat16)
    if pad_nan:
        x.view(torch.int16)[B * S:] = torch.tensor(NAN16, dtype=torch.int16)
    else:
        x[B * S:] = 0
    return x


def make_dout(B, S, H, seed):
    """bf16 randn dO rows b*S + i, head h at columns 64h, NaN in the padding rows"""
    g = torch.Generator().manual_seed(seed + 77)
    x = torch.randn((B * S + 63) // 64 * 64 + 64, H * 64, generator=g).to(torch.bfloat16)
    x.view(torch.int16)[B * S:] = torch.tensor(NAN16, dtype=torch.int16)
    return x


def heads(x, B, S, H, part, dtype):
    """[B, H, S, 64] in `dtype`: part 0 / 1 / 2 of q'|k|v rows, or the heads of dO rows (part None)"""
    if part is None:
        return x[:B * S, :H * 64].to(dtype).reshape(B, S, H, 64).transpose(1, 2)
    return x[:B * S].to(dtype).reshape(B, S, 3, H, 64)[:, :, part].transpose(1, 2)


def lse2_of(qkv, B, S, H):
    """the base-2 log-sum-exp in fp64, rounded to the f32 the kernel reads: [B*H*S]"""
    s = heads(qkv, B, S, H, 0, torch.float64) @ heads(qkv, B, S, H, 1, torch.float64).transpose(2, 3)
    m = s.max(dim=-1, keepdim=True).values
    return (m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))).reshape(-1).float()


def step_ref(qkv, dout, lse, r_in, B, S, H, alpha, beta, dtype):
    """the gradient-weighted step's formula, materialised, in `dtype` on the CPU"""
    q, k, v = (heads(qkv, B, S, H, i, dtype) for i in range(3))
    p = torch.exp2(q @ k.transpose(2, 3) - lse.to(dtype).reshape(B, H, S, 1))
    dp = heads(dout, B, S, H, None, dtype) @ v.transpose(2, 3)
    u = torch.einsum("bi,bhij->bj", r_in.to(dtype), (p * dp).clamp(min=0)) / H
    return alpha * u + beta * r_in.to(dtype)


def r_inputs(B, S, seed):
    e = torch.zeros(B, S)
    e[:, 0] = 1.0
    g = torch.Generator().manual_seed(seed)
    return {"e_cls": e, "random": torch.rand(B, S, generator=g) + 0.05}


def run_step(qkv_d, dout_d, lse_d, r_in, B, S, H, alpha, beta):
    work = ops.attention_rollout_work(B, S, H, "cuda")
    out = torch.full((B, S), float("nan"), device="cuda")
    ops.attention_grad_rollout_step(qkv_d, dout_d, lse_d, r_in.cuda(), B, S, H, alpha, beta, work, out)
    return out.cpu()


def check_against_fp64(qkv, dout, lse, B, S, H, what):
    """every (r_in, alpha, beta) case of one shape: finite, and within 8 x the shape's fp32 yardstick of fp64"""
    qkv_d, dout_d, lse_d = qkv.cuda(), dout.cuda(), lse.cuda()
    errs, yard = {}, 0.0
    for name, r in r_inputs(B, S, seed=S).items():
        for alpha, beta in ((1.0, 0.0), (1.0, 1.0)):  # beta = 0: u is not swamped by r_in
            ref = step_ref(qkv, dout, lse, r, B, S, H, alpha, beta, torch.float64)
            yard = max(yard, rel_err(step_ref(qkv, dout, lse, r, B, S, H, alpha, beta, torch.float32), ref))
            got = run_step(qkv_d, dout_d, lse_d, r, B, S, H, alpha, beta)
            assert torch.isfinite(got).all(), (what, name, alpha, beta)
            errs[(name, beta)] = rel_err(got, ref)
    print(f"grad rollout step {what} (B, S, H) = {(B, S, H)}: fp32 yardstick {yard:.3e}, kernel "
          + ", ".join(f"{k[0]}/b={k[1]}: {v:.3e} ({v / yard:.2f}x)" for k, v in errs.items()))
    assert max(errs.values()) <= 8 * yard, (errs, yard)


# ------------------------------------------------------------------ 1. kernel against materialised fp64
@pytest.mark.parametrize("B,S,H", [(1, 33, 2), (3, 65, 1), (1, 197, 3), (2, 321, 12)])
def test_grad_rollout_step_matches_fp64(B, S, H):
    """partial 64-row tiles at every S (65 and 321 leave one row), another clip's rows in the overhang at
    B > 1, twelve heads, NaN in the padding rows past B*S of q|k|v and of dO"""
    qkv = make_qkv(B, S, H, seed=B * 1000 + S)
    check_against_fp64(qkv, make_dout(B, S, H, seed=S), lse2_of(qkv, B, S, H), B, S, H, "fp64 lse")


# ------------------------------------------------------------------ 2. exact cases
def test_grad_rollout_step_zero_gradient_deterministic_and_batch_invariant():
    B, S, H = 3, 197, 3
    qkv = make_qkv(B, S, H, seed=11)
    dout = make_dout(B, S, H, seed=11)
    lse = lse2_of(qkv, B, S, H)
    r = r_inputs(B, S, seed=5)["random"]
    qkv_d, lse_d = qkv.cuda(), lse.cuda()
    zero = torch.zeros_like(dout)
    zero.view(torch.int16)[B * S:] = torch.tensor(NAN16, dtype=torch.int16)
    for beta in (1.0, 0.5, 0.0):  # dO = 0: every product is 0, r_out = beta * r_in exactly
        assert torch.equal(run_step(qkv_d, zero.cuda(), lse_d, r, B, S, H, 1.0, beta), beta * r)
    a = run_step(qkv_d, dout.cuda(), lse_d, r, B, S, H, 1.0, 1.0)
    b = run_step(qkv_d, dout.cuda(), lse_d, r, B, S, H, 1.0, 1.0)
    assert torch.equal(a, b)
    assert not torch.equal(a, r)  # ... and the gradient did something
    one, one_do = make_qkv(1, S, H, seed=0), make_dout(1, S, H, seed=0)
    one[:S], one_do[:S] = qkv[S:2 * S], dout[S:2 * S]
    c = run_step(one.cuda(), one_do.cuda(), lse.reshape(B, H * S)[1].contiguous().cuda(), r[1:2].contiguous(), 1, S, H,
                 1.0, 1.0)
    assert torch.equal(a[1:2], c)


# ------------------------------------------------------------------ 3. pairing with the real forward
def test_grad_rollout_step_pairs_with_attention_fwd_lse():
    B, S, H = 2, 197, 3
    qkv = make_qkv(B, S, H, seed=7, pad_nan=False)  # the forward reads a 64-key tile past each clip's end
    qkv_d = qkv.cuda()
    o = torch.zeros(qkv.shape[0], H * 64, dtype=torch.bfloat16, device="cuda")
    lse_d = torch.zeros(B * H * S, device="cuda")
    ops.attention_fwd_lse(qkv_d, B, S, H, o, lse_d)
    check_against_fp64(qkv, make_dout(B, S, H, seed=7), lse_d.cpu(), B, S, H, "forward's lse")


# ------------------------------------------------------------------ 4. model against the fp32 oracle with autograd
def oracle_grad_rollout(sd, cfg, pix, target):
    """oracle/vivit_ref.vivit_forward's per-layer loop under autograd for y = sum_b logits[b, target[b]]:
    (logits, relevance [B, S] fp64, the same with q, k, v and dO rounded to bf16 before each layer's matrix).
    relevance: r = e_CLS, for l = L .. 1  r <- r + mean_h(max(dy/dA_l[h] * A_l[h], 0))^T r."""
    from oracle.vivit_ref import gelu_fast, layer_norm
    D, H = cfg["hidden_size"], cfg["num_attention_heads"]
    hd = D // H
    eps = cfg.get("layer_norm_eps", 1e-6)
    kt, kh, kw = cfg["tubelet_size"]
    B = pix.shape[0]
    pix = pix.clone().requires_grad_(True)  # the weights need no gradient: the clip carries the graph
    emb = torch.nn.functional.conv3d(pix.transpose(1, 2), sd["vivit.embeddings.patch_embeddings.projection.weight"],
                                     sd["vivit.embeddings.patch_embeddings.projection.bias"], stride=(kt, kh, kw))
    emb = emb.flatten(2).transpose(1, 2)
    h = torch.cat([sd["vivit.embeddings.cls_token"].expand(B, -1, -1), emb], dim=1) + sd["vivit.embeddings.position_embeddings"]
    S = h.shape[1]
    scale = hd ** -0.5
    kept = []
    for i in range(cfg["num_hidden_layers"]):
        p = f"vivit.layers.{i}."
        r = h
        y = layer_norm(h, sd[p + "layernorm_before.weight"], sd[p + "layernorm_before.bias"], eps)

        def proj(nm, t):
            return t @ sd[p + f"attention.{nm}.weight"].T + sd[p + f"attention.{nm}.bias"]

        q = proj("q_proj", y).view(B, S, H, hd).transpose(1, 2)
        k = proj("k_proj", y).view(B, S, H, hd).transpose(1, 2)
        v = proj("v_proj", y).view(B, S, H, hd).transpose(1, 2)
        a = torch.softmax((q @ k.transpose(2, 3)) * scale, dim=-1, dtype=torch.float32)
        av = a @ v
        a.retain_grad()
        av.retain_grad()
        kept.append((q, k, v, a, av))
        o = av.transpose(1, 2).reshape(B, S, D)
        h = proj("o_proj", o) + r
        r = h
        y = layer_norm(h, sd[p + "layernorm_after.weight"], sd[p + "layernorm_after.bias"], eps)
        y = gelu_fast(y @ sd[p + "mlp.fc1.weight"].T + sd[p + "mlp.fc1.bias"])
        h = y @ sd[p + "mlp.fc2.weight"].T + sd[p + "mlp.fc2.bias"] + r
    seq = layer_norm(h, sd["vivit.layernorm.weight"], sd["vivit.layernorm.bias"], eps)
    logits = seq[:, 0, :] @ sd["classifier.weight"].T + sd["classifier.bias"]
    logits[torch.arange(B), torch.as_tensor(target)].sum().backward()

    def roll(mats):
        r = torch.zeros(B, S, dtype=torch.float64)
        r[:, 0] = 1.0
        for A in reversed(mats):
            r = r + torch.einsum("bi,bij->bj", r, A)
        return r

    exact, rounded = [], []
    b16 = lambda t: t.detach().bfloat16().double()  # noqa: E731
    for q, k, v, a, av in kept:
        exact.append((a.grad.double() * a.detach().double()).clamp(min=0).mean(1))
        a16 = torch.softmax((b16(q) @ b16(k).transpose(2, 3)) * scale, dim=-1)
        rounded.append(((b16(av.grad) @ b16(v).transpose(2, 3)) * a16).clamp(min=0).mean(1))
    return logits.detach(), roll(exact), roll(rounded)


def _tiny():
    g = np.load(os.path.join(GD, "vivit_tiny.npz"))
    return json.loads(str(g["config"])), torch.from_numpy(g["pixel_values"])


def _multi_tile():
    cfg = dict(image_size=96, num_frames=8, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=128,
               num_hidden_layers=3, num_attention_heads=2, intermediate_size=256, hidden_act="gelu_fast",
               layer_norm_eps=1e-6, qkv_bias=True)
    return cfg, torch.from_numpy(make_synthetic_clips(2, 8, 96, seed=1))


def _model(cfg):
    from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
    m = VivitForVideoClassification(VivitConfig(**cfg, id2label={0: "non-referral", 1: "referral"}))
    m.load_state_dict(make_vivit_weights(cfg, seed=0))
    return m.cuda().eval()


@pytest.fixture(scope="module", params=["tiny", "multi_tile"])
def case(request):
    """(cfg, pix, model, {target: the oracle's (logits, relevance, bf16-rounded relevance)}), made once"""
    cfg, pix = _tiny() if request.param == "tiny" else _multi_tile()
    sd = {k: torch.from_numpy(v) for k, v in make_vivit_weights(cfg, seed=0).items()}
    return cfg, pix, _model(cfg), {t: oracle_grad_rollout(sd, cfg, pix, [t] * pix.shape[0]) for t in (0, 1)}


def test_explain_grad_rollout_matches_oracle(case):
    """the target is passed explicitly: the fixtures' logit margins (0.014 - 0.056) are within the logit tolerance,
    so an argmax target could differ between the GPU and the oracle"""
    cfg, pix, m, oracle = case
    B = pix.shape[0]
    kt, kh, kw = cfg["tubelet_size"]
    grid = (cfg["num_frames"] // kt, cfg["image_size"] // kh, cfg["image_size"] // kw)
    S = 1 + grid[0] * grid[1] * grid[2]
    maps, ratios = {}, {}
    for t in (0, 1):
        want_logits, ref, ref16 = oracle[t]
        assert (ref[:, 1:].sum(1) > 0).all()  # the fixture does not meet the zero-sum refusal
        ex = m.explain(pix.cuda(), method="grad_rollout", target=t)
        assert ex.method == "grad_rollout" and ex.target == [t] * B
        assert tuple(ex.token_relevance.shape) == (B, S) and tuple(ex.saliency.shape) == (B, *grid)
        assert tuple(ex.temporal.shape) == (B, grid[0]) and tuple(ex.logits.shape) == (B, 2)
        assert all(x.dtype == torch.float32 for x in (ex.logits, ex.token_relevance, ex.saliency, ex.temporal))
        assert float((ex.logits.cpu() - want_logits).abs().max()) < 1e-2
        assert torch.isfinite(ex.token_relevance).all() and (ex.saliency >= 0).all()
        assert ((ex.saliency.double().sum(dim=(1, 2, 3)) - 1).abs() < 1e-5).all()
        assert torch.equal(ex.temporal, ex.saliency.sum(dim=(2, 3)))
        patch = ex.token_relevance[:, 1:].double()
        assert torch.allclose(ex.saliency.double().reshape(B, -1), patch / patch.sum(1, keepdim=True), rtol=1e-6, atol=0)
        yard = rel_err(ref16[:, 1:], ref[:, 1:])
        err = rel_err(ex.token_relevance[:, 1:], ref[:, 1:])
        ratios[t] = err / yard
        print(f"explain grad_rollout S = {S} L = {cfg['num_hidden_layers']} target {t}: patch sums "
              f"{[round(float(v), 4) for v in ref[:, 1:].sum(1)]}, bf16 q/k/v/dO oracle yardstick {yard:.3e}, GPU "
              f"{err:.3e} ({err / yard:.2f}x)")
        maps[t] = ex.saliency
    assert not torch.equal(maps[0], maps[1])  # class-specific
    assert max(ratios.values()) <= MODEL_FACTOR, ratios


# ------------------------------------------------------------------ 5. target=None
def test_explain_grad_rollout_default_target_is_the_argmax(case):
    cfg, pix, m, _ = case
    ex = m.explain(pix.cuda(), method="grad_rollout")
    assert ex.target == ex.logits.argmax(dim=1).tolist()
    same = m.explain(pix.cuda(), method="grad_rollout", target=ex.target)
    assert same.target == ex.target and torch.equal(same.logits, ex.logits)
    assert torch.equal(same.token_relevance, ex.token_relevance) and torch.equal(same.saliency, ex.saliency)
    as_tensor = m.explain(pix.cuda(), method="grad_rollout", target=torch.tensor(ex.target))
    assert torch.equal(as_tensor.token_relevance, ex.token_relevance)
    with pytest.raises(ValueError, match="entries"):
        m.explain(pix.cuda(), method="grad_rollout", target=[0] * (pix.shape[0] + 1))


# ------------------------------------------------------------------ 6. nothing else moved
def test_explain_grad_rollout_leaves_the_model_alone():
    cfg, pix = _tiny()
    m = _model(cfg)
    pix = pix.cuda()
    m.graph_replay = True
    before = m(pixel_values=pix).logits.clone()
    roll = m.explain(pix, method="rollout")
    captures, packed, ws = m._graphs.captures, m._packed, dict(m._ws)
    m.explain(pix, method="grad_rollout", target=1)
    assert torch.equal(m(pixel_values=pix).logits, before)
    assert m._graphs.captures == captures and m._packed is packed
    assert m._ws.keys() == ws.keys() and all(m._ws[k] is ws[k] for k in ws)
    assert m._flat is None and m._gflat is None and m._engine is None
    assert all(p.grad is None for p in m.parameters())
    again = m.explain(pix, method="rollout")
    assert again.target is None
    assert torch.equal(again.token_relevance, roll.token_relevance) and torch.equal(again.logits, roll.logits)
    m.config.hidden_act = "gelu"  # no backward for the erf GELU in the data-gradient chain
    m._explain_grad = {}
    with pytest.raises(RuntimeError, match="hidden_act"):
        m.explain(pix, method="grad_rollout")


def test_explain_grad_rollout_refuses_a_zero_map():
    """a classifier whose weights are zero has no gradient to weight the attention by: every product is 0, the
    relevance stays e_CLS, and there is nothing to normalise"""
    cfg, pix = _tiny()
    m = _model(cfg)
    with torch.no_grad():
        m.P("classifier.weight").zero_()
    with pytest.raises(RuntimeError, match="sum to 0"):
        m.explain(pix.cuda(), method="grad_rollout", target=0)


# ------------------------------------------------------------------ 7. full size once
def test_explain_grad_rollout_vivit_b_full_size():
    """ViViT-B/16x2 at B = 1: runs, finite, the sums hold; prints the peak extra device memory (the kept
    activations of a backward: DESIGN.md section 5.13)"""
    with open(os.path.join(GD, "vivit_full.json")) as f:
        cfg = json.load(f)["config"]
    m = _model(cfg)
    pix = torch.from_numpy(make_synthetic_clips(1, cfg["num_frames"], cfg["image_size"], seed=3)).cuda()
    m(pixel_values=pix)  # the packed weights and the forward's workspace exist before the measurement
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ex = m.explain(pix, method="grad_rollout")
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"explain grad_rollout ViViT-B B = 1: peak extra device memory {extra / 1e6:.1f} MB, target {ex.target}")
    assert tuple(ex.saliency.shape) == (1, 16, 14, 14)
    assert torch.isfinite(ex.token_relevance).all() and torch.isfinite(ex.logits).all()
    assert (ex.saliency >= 0).all()
    assert abs(float(ex.saliency.double().sum()) - 1) < 1e-5
    assert torch.equal(ex.temporal, ex.saliency.sum(dim=(2, 3)))
