"""The last ViViT layer for the CLS rows only (csrc/cls_tail.hip): the CLS-query attention and the
skinny GEMM against torch references on the same 16-bit operands, and the pruned forward against
the full one.

u(dtype) below is the unit roundoff of the 16-bit type (half the spacing of neighbours, relative):
2^-8 for bf16 (8 significand bits), 2^-11 for fp16."""
import json
import math
import os

import numpy as np
import pytest
import torch

from vclip_amd.weights import make_synthetic_clips, make_vivit_weights

pytestmark = pytest.mark.gpu
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = [torch.bfloat16, torch.float16]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---- CLS attention -------------------------------------------------------------------------------

def _attn_ref(qkv, B, S, H):
    """fp32 torch reference on the upcast 16-bit operands: exp2 of the pre-scaled scores"""
    D = H * 64
    x = qkv[:B * S].float().reshape(B, S, 3, H, 64)
    q, k, v = x[:, 0, 0], x[:, :, 1], x[:, :, 2]  # [B,H,64], [B,S,H,64]
    s = torch.einsum("bhd,bshd->bhs", q, k)
    p = torch.exp2(s - s.max(dim=2, keepdim=True).values)
    return torch.einsum("bhs,bshd->bhd", p, v) / p.sum(dim=2, keepdim=True)


def _run_attn(qkv, B, S, H, pad_rows=64):
    """cls_attention on qkv [B*S, 3*H*64] laid into a buffer with NaN rows past B*S; returns o [B,H,64] and
    checks that nothing but the rows b*S of out was written"""
    from vclip_amd import ops
    D = H * 64
    buf = torch.full((B * S + pad_rows, 3 * D), float("nan"), dtype=qkv.dtype, device="cuda")
    buf[:B * S] = qkv
    out = torch.full((B * S, D), 3.0, dtype=qkv.dtype, device="cuda")
    ops.cls_attention(buf, B, S, H, ops.cls_attention_work(B, S, H, "cuda"), out)
    o = out[::S].clone()
    out[::S] = 3.0
    assert bool((out == 3.0).all()), "cls_attention wrote a row other than b*S"
    return o.float().reshape(B, H, 64)


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 197, 3137])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_cls_attention_matches_fp32_reference(dtype, S):
    """S below one key split (256 keys), not a multiple of it, one past a 64-key tile; NaN rows past
    B*S must not reach the result (keys are masked by index).  Bar per (clip, head): one rounding of
    the output to the 16-bit type, 2^-8 max|ref| (the fp32 accumulation error is orders below)."""
    for B in (1, 3):
        for H in (1, 4, 12):
            g = _gen(1000 * S + 10 * H + B)
            qkv = torch.randn(B * S, 3 * H * 64, generator=g, device="cuda")
            qkv[:, :H * 64] *= 0.125 * math.log2(math.e) * 4  # q pre-scaled; scores of a few units
            qkv = qkv.to(dtype)
            ref = _attn_ref(qkv, B, S, H)
            o = _run_attn(qkv, B, S, H)
            assert bool(torch.isfinite(o).all())
            err = (o - ref).abs().amax(dim=2)
            bar = 2.0 ** -8 * ref.abs().amax(dim=2)
            assert bool((err <= bar).all()), (S, B, H, float((err / bar).max()))


@pytest.mark.parametrize("where", ["last", "first", "middle"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_cls_attention_wide_score_range(dtype, where):
    """Scores spread over 400 in the log2 domain, the maximum in the last key (of a partial split), the
    first, or inside: with an inexact max exp2 would overflow or flush every term."""
    B, S, H = 2, 300, 2
    g = _gen(7)
    qkv = torch.randn(B * S, 3 * H * 64, generator=g, device="cuda")
    score = torch.linspace(-200.0, 200.0, S, device="cuda")
    if where == "first":
        score = score.flip(0)
    elif where == "middle":
        score = torch.roll(score, 130)
    qkv[:, :H * 64] = 4.0
    qkv[:, H * 64:2 * H * 64] = (score / 256.0).repeat(B)[:, None]  # q.k = 64 * 4 * score / 256
    qkv = qkv.to(dtype)
    ref = _attn_ref(qkv, B, S, H)
    o = _run_attn(qkv, B, S, H)
    assert bool(torch.isfinite(o).all())
    assert bool(((o - ref).abs().amax(dim=2) <= 2.0 ** -8 * ref.abs().amax(dim=2)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_cls_attention_batch_invariant(dtype):
    B, S, H = 3, 517, 4
    qkv = (torch.randn(B * S, 3 * H * 64, generator=_gen(3), device="cuda") * 0.7).to(dtype)
    full = _run_attn(qkv, B, S, H)
    one = _run_attn(qkv[S:2 * S].contiguous(), 1, S, H)
    assert torch.equal(full[1:2], one)


# ---- skinny GEMM -----------------------------------------------------------------------------------

EPIS = ["bias", "bias_gelu_tanh", "bias_gelu_erf", "bias_resid_f32"]


def _strided_rows(rows, stride_rows, fill):
    """`rows` [M, C] placed at row stride `stride_rows` of a buffer filled with `fill`: (buffer, view)"""
    M, C = rows.shape
    buf = torch.full(((M - 1) * stride_rows + 1, C), fill, dtype=rows.dtype, device="cuda")
    view = buf[::stride_rows]
    view.copy_(rows)
    return buf, view


def _gelu64(x, kind):
    if kind == "bias_gelu_tanh":
        return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _ln_operand(x, g, b, eps, dtype, stride):
    """The 16-bit rows the LayerNorm prologue feeds the product, read back through an identity weight
    (exact: one non-zero product per output), and checked against an fp64 LayerNorm to one 16-bit
    rounding plus one flipped rounding (2 u |y|; 1e-6: fp16 subnormals)."""
    from vclip_amd import ops
    M, K = x.shape
    eye = torch.eye(K, dtype=dtype, device="cuda")
    _, xv = _strided_rows(x, stride, 0.0)
    a16 = ops.skinny_gemm(xv, eye, torch.zeros(K, device="cuda"), "bias", torch.empty(M, K, dtype=dtype, device="cuda"),
                          ln=(g, b, eps))
    xd = x.double()
    mu = xd.mean(dim=1, keepdim=True)
    y = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(dim=1, keepdim=True) + eps) * g.double() + b.double()
    assert bool(((a16.double() - y).abs() <= 2 * U[dtype] * y.abs() + 1e-6).all())
    return a16


@pytest.mark.parametrize("N,K", [(768, 768), (3072, 768), (768, 3072), (128, 64), (256, 192)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_skinny_gemm_matches_fp64_reference(dtype, N, K):
    """Every epilogue, with and without the LayerNorm prologue, M in {1, 3, 8, 11} (one row, a partial
    chunk, a whole chunk, two chunks), rows contiguous and at strides 17 and 3137 (A, out and the
    residual), against fp64 on the same 16-bit operands.  Bars per element, E = K 2^-24 sum|a||w| (fp32
    accumulation): fp32 outputs E; 16-bit outputs E' + u |ref| (one more rounding), where for the GELU
    epilogues E' = 1.13 E + 1e-6 (max |gelu'| = 1.13; the kernels' GELU approximations are within 5e-7,
    common.hpp).  The buffers are compared whole: no row but the addressed ones may change."""
    from vclip_amd import ops
    u = U[dtype]
    eps = 1e-6
    g = _gen(N * 7 + K)
    w = (torch.randn(N, K, generator=g, device="cuda") / math.sqrt(K)).to(dtype)
    bias = torch.randn(N, generator=g, device="cuda") * 0.5
    lng = 1.0 + 0.2 * torch.randn(K, generator=g, device="cuda")
    lnb = 0.1 * torch.randn(K, generator=g, device="cuda")
    worst = 0.0
    for M in (1, 3, 8, 11):
        x32 = torch.randn(M, K, generator=g, device="cuda") * 1.5 + 0.3
        resid = torch.randn(M, N, generator=g, device="cuda")
        for stride in (1, 17, 3137):
            for ln in (False, True):
                if ln:
                    a16 = _ln_operand(x32, lng, lnb, eps, dtype, stride)
                    _, av = _strided_rows(x32, stride, float("nan"))
                else:
                    a16 = x32.to(dtype)
                    _, av = _strided_rows(a16, stride, float("nan"))
                acc = a16.double() @ w.double().T + bias.double()
                E = K * 2.0 ** -24 * (a16.double().abs() @ w.double().abs().T)
                for epi in EPIS:
                    if epi == "bias_resid_f32":
                        buf, ov = _strided_rows(resid, stride, 5.0)
                        ref, tol = resid.double() + acc, E
                    else:
                        buf, ov = _strided_rows(torch.full((M, N), 9.0, dtype=dtype, device="cuda"), stride, 5.0)
                        if epi == "bias":
                            ref, tol = acc, E + u * acc.abs()
                        else:
                            ref = _gelu64(acc, epi)
                            tol = 1.13 * E + 1e-6 + u * ref.abs()
                    ops.skinny_gemm(av, w, bias, epi, ov, ln=(lng, lnb, eps) if ln else None)
                    got = ov.double().clone()
                    ov.fill_(5.0)
                    assert bool((buf == 5.0).all()), (epi, M, stride, ln, "a row that was not addressed changed")
                    ratio = float(((got - ref).abs() / tol).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (epi, M, stride, ln, ratio)
    print(f"skinny_gemm N={N} K={K} {dtype}: worst |err| / bar = {worst:.3f}")


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_skinny_gemm_row_invariant(dtype, ln):
    """Row i of an M = 8 call equals the M = 1 call on that row, and row 9 of an M = 11 call (second
    chunk, slot 1) too, bit for bit."""
    from vclip_amd import ops
    N, K = 256, 768
    g = _gen(11)
    w = (torch.randn(N, K, generator=g, device="cuda") / math.sqrt(K)).to(dtype)
    bias = torch.randn(N, generator=g, device="cuda")
    x = torch.randn(11, K, generator=g, device="cuda")
    a = x if ln else x.to(dtype)
    lnp = (torch.rand(K, generator=g, device="cuda") + 0.5, torch.randn(K, generator=g, device="cuda"), 1e-6) if ln else None
    for epi in ("bias_gelu_tanh", "bias_resid_f32"):
        def call(rows):
            out = torch.ones(rows.shape[0], N, dtype=torch.float32 if epi == "bias_resid_f32" else dtype, device="cuda")
            return ops.skinny_gemm(rows.contiguous(), w, bias, epi, out, ln=lnp)
        all11, first8 = call(a), call(a[:8])
        for i in (0, 5, 7):
            assert torch.equal(first8[i:i + 1], call(a[i:i + 1])), (epi, i)
        assert torch.equal(all11[:8], first8)
        assert torch.equal(all11[9:10], call(a[9:10]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_skinny_gemm_ln_prologue_equals_layernorm_kernel(dtype):
    """At the ViViT width the prologue's normalised rows are the LayerNorm kernel's, bit for bit (same
    statistics, same order, same rounding): LN2 of the CLS rows is what the full layer computes."""
    from vclip_amd import ops
    K, M = 768, 5
    g = _gen(5)
    x = torch.randn(M, K, generator=g, device="cuda") * 2.0 - 0.4
    lng, lnb = torch.rand(K, generator=g, device="cuda") + 0.5, torch.randn(K, generator=g, device="cuda")
    want = ops.layernorm(x, lng, lnb, 1e-6, torch.empty(M, K, dtype=dtype, device="cuda"))
    assert torch.equal(_ln_operand(x, lng, lnb, 1e-6, dtype, 1), want)


def test_cls_tail_refuses_what_it_does_not_take():
    from vclip_amd import _lib, ops
    w = torch.zeros(8, 4104, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.VclipError):  # K past the LDS staging
        ops.skinny_gemm(torch.zeros(1, 4104, dtype=torch.bfloat16, device="cuda"), w, torch.zeros(8, device="cuda"), "bias",
                        torch.zeros(1, 8, dtype=torch.bfloat16, device="cuda"))
    assert not ops.skinny_gemm_takes(4104) and not ops.skinny_gemm_takes(100) and ops.skinny_gemm_takes(3072)
    with pytest.raises(_lib.VclipError):  # a work buffer of another shape
        ops.cls_attention(torch.zeros(600, 192, dtype=torch.bfloat16, device="cuda"), 1, 600, 1,
                          ops.cls_attention_work(1, 256, 1, "cuda"), torch.zeros(1, 64, dtype=torch.bfloat16, device="cuda"))


# ---- the model -------------------------------------------------------------------------------------

def _model(cfg):
    from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
    c = VivitConfig(**cfg, id2label={0: "non-referral", 1: "referral"})
    m = VivitForVideoClassification(c)
    m.load_state_dict(make_vivit_weights(cfg, seed=0))
    return m.cuda().eval()


@pytest.fixture(scope="module", params=["tiny", "vivit_b"])
def case(request):
    """(model, clips, HF golden logits): the tiny golden config (B = 3) and ViViT-B at B = 2"""
    if request.param == "tiny":
        g = np.load(os.path.join(GD, "vivit_tiny.npz"))
        cfg = json.loads(str(g["config"]))
        return _model(cfg), torch.from_numpy(g["pixel_values"]).cuda(), np.asarray(g["logits"])
    with open(os.path.join(GD, "vivit_full.json")) as f:
        g = json.load(f)
    cfg = g["config"]
    pix = torch.from_numpy(make_synthetic_clips(g["batch"], cfg["num_frames"], cfg["image_size"], seed=g["input_seed"]))
    return _model(cfg), pix.cuda(), np.array(g["logits"])


def _logits(m, pix, cls_only, **attrs):
    keep = {k: getattr(m, k) for k in attrs}
    m.cls_only_last_layer = cls_only
    for k, v in attrs.items():
        setattr(m, k, v)
    try:
        return m.forward_logits(pix).clone()
    finally:
        m.cls_only_last_layer = True
        for k, v in keep.items():
            setattr(m, k, v)


def test_pruned_logits_within_a_tenth_of_the_bf16_error(case):
    """max |logit(CLS-only last layer) - logit(full last layer)| is at most a tenth of the full forward's
    own error against the HF golden on the same clips: only fp32 summation order and isolated single-ulp
    16-bit flips may differ between the two.

    Measured (MI355X): ViViT-B B = 2 bf16 2.37e-4 against a full-forward error of 4.67e-3 (0.05; fp16 1.5e-5
    against 7.6e-4), and on the bench's 8 clips 3.80e-4 against 4.77e-3 (0.08).  That difference is the MFMA
    attention kernel's 16-bit P, which the CLS kernel keeps in fp32: with the full kernel feeding the CLS-only
    GEMMs the logits agree to 1.8e-7.  At S <= 256 (the tiny config: S = 33) the library's attention is the
    short-sequence kernel, and the model keeps it in the last layer too (vivit.py), so there only the fp32
    summation order of the CLS-only GEMMs differs (6e-8)."""
    m, pix, golden = case
    full = _logits(m, pix, False).cpu().numpy()
    pruned = _logits(m, pix, True).cpu().numpy()
    own = float(np.abs(full - golden).max())
    delta = float(np.abs(pruned - full).max())
    print(f"max |pruned - full| = {delta:.3e}; full forward vs HF golden = {own:.3e}; pruned vs golden = "
          f"{float(np.abs(pruned - golden).max()):.3e}")
    assert delta <= 0.1 * own, (delta, own)


def test_last_layer_launches(case):
    """What the pruned forward launches: full-size o_proj / fc1 / fc2 in all layers but the last, the CLS-only
    GEMMs once, and for the last layer's attention the CLS kernel, or the short-sequence kernel at S <= 256."""
    m, pix, _ = case
    n = m.config.num_hidden_layers
    _, S, _, _ = m.geometry(pix.shape[0])
    m.kernel_events = ev = {}
    try:
        _logits(m, pix, True, concurrent_streams=1)
    finally:
        m.kernel_events = None
    torch.cuda.synchronize()
    count = {k: len(v) for k, v in ev.items()}
    assert count["o_proj"] == count["fc1"] == count["fc2"] == n - 1 and count["layernorm"] == 2 * n - 1
    assert count["cls_o_proj"] == count["cls_fc1"] == count["cls_fc2"] == 1 and count["qkv"] == n
    if S <= 256:
        assert count["attention"] == n and "cls_attention" not in count
    else:
        assert count["attention"] == n - 1 and count["cls_attention"] == 1


def test_pruned_path_bit_identical_across_streams_and_graph_replay(case):
    m, pix, _ = case
    one = _logits(m, pix, True, concurrent_streams=1)
    assert torch.equal(_logits(m, pix, True, concurrent_streams=2), one)
    for ns in (1, 2):
        assert torch.equal(_logits(m, pix, True, concurrent_streams=ns, graph_replay=True), one)
        assert torch.equal(_logits(m, pix, True, concurrent_streams=ns, graph_replay=True), one)  # the replay
    # the attribute is part of the replay key: toggling it re-captures
    full = _logits(m, pix, False, concurrent_streams=2)
    assert torch.equal(_logits(m, pix, False, concurrent_streams=2, graph_replay=True), full)
    assert torch.equal(_logits(m, pix, True, concurrent_streams=2, graph_replay=True), one)


def test_forward_part_default_runs_every_layer_over_every_row(case):
    """_forward_part(pix, 0) leaves the full last hidden state in X (per-layer drift test, timeline tool):
    the same bits as cls_only=False passed explicitly, and the full forward's logits."""
    m, pix, _ = case
    B = pix.shape[0]
    _, S, _, _ = m.geometry(B)
    lg0 = m._forward_part(pix, 0).clone()
    x0 = m._workspace(B, pix.device, 0)["X"][:B * S].clone()
    lg1 = m._forward_part(pix, 0, cls_only=False).clone()
    x1 = m._workspace(B, pix.device, 0)["X"][:B * S].clone()
    assert torch.equal(x0, x1) and torch.equal(lg0, lg1)
    assert torch.equal(lg0, _logits(m, pix, False, concurrent_streams=1))
    # the pruned call changes the CLS rows only past the last layer's q|k|v: patch rows keep layer L-1's state
    m._forward_part(pix, 0, cls_only=True)
    x2 = m._workspace(B, pix.device, 0)["X"][:B * S]
    assert not torch.equal(x2[1:S], x0[1:S])


def test_fallbacks_run_the_full_layer(case):
    """Train mode, and an fp16 build whose split-operand layers include the last one: the full layer's logits
    bit for bit."""
    m, pix, _ = case
    full = _logits(m, pix, False)
    m.train()
    try:
        with torch.no_grad():
            assert torch.equal(_logits(m, pix, True), full)
    finally:
        m.eval()
    if m.config.hidden_size % 256 == 0:  # the split-operand GEMM runs whole 256-column tiles: not the tiny widths
        fp16 = dict(compute_dtype=torch.float16, precise_layers=m.config.num_hidden_layers)
        assert torch.equal(_logits(m, pix, True, **fp16), _logits(m, pix, False, **fp16))
    # and fp16 without split operands in the last layer takes the pruned path, close to its full one
    a, b = _logits(m, pix, True, compute_dtype=torch.float16), _logits(m, pix, False, compute_dtype=torch.float16)
    assert float((a - b).abs().max()) < 1e-3
