"""LoRA fine-tuning of ViViT on the GPU (vclip_amd/lora.py, csrc/lora.hip, vivit_train.TrainEngine's LoRA mode):
the merge kernel and the adapter-gradient kernels against fp64 on the same operands, the model's adapter gradients
and a three-step AdamW loop against autograd on the fp32 oracle (tests/lora_ref.py), the early stop of the backward,
the zero-adapter identity, merging, and the combinations that are refused.

Tolerances.  vc_lora_merge's fp32 output: r fused multiply-adds and one more for W + s*acc, each within 2^-24 of
its result, so |err| <= (r + 1) 2^-24 (|W| + s |B||A|) <= r 2^-23 (...).  Adapter gradients: the r-wide intermediate
(x A^T or dy B) is rounded to bf16 once, 2^-9 relative per element, and the fp32 sums over M <= 2080 rows add far
less, so relative L2 <= 2^-7 leaves a fourfold margin (the kernel also reads A / B rounded to bf16, the MFMA's
operand type: the same 2^-9 per element once more, inside that margin; the fp64 reference keeps them fp32).  Model
gradients, losses and AdamW updates: the bars of tests/test_vivit_train_gpu.py (relative L2 < 5e-2 and cosine > 0.998
per tensor, logits 1e-2, losses 2e-2, accumulated update within 0.1)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

SMALL = dict(image_size=32, num_frames=4, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=256,
             num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, hidden_act="gelu_fast",
             layer_norm_eps=1e-6, qkv_bias=True)
ALL6 = ("q", "k", "v", "o", "fc1", "fc2")
SHAPES = [(256, 256), (512, 256), (256, 512)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd import _lib as L
    L.load()


def _randn(*shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


# ---- 1. vc_lora_merge -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [3, 8, 16, 64])
@pytest.mark.parametrize("N,K", SHAPES)
def test_merge_against_fp64_and_its_own_roundings(N, K, r):
    from vclip_amd import ops
    W, A, B = _randn(N, K, seed=1, scale=0.05), _randn(r, K, seed=2, scale=0.1), _randn(N, r, seed=3, scale=0.1)
    s, ns, scale = 2.0, N // 2, 0.18033688
    out = torch.full((N, K), float("nan"), device=DEV)
    dst = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    dst_t = torch.zeros(K, N, dtype=torch.bfloat16, device=DEV)
    ops.lora_merge(W, A, B, s, dst, dst_t, out, nscaled=ns, scale=scale)
    ref = W.double() + s * (B.double() @ A.double())
    bound = r * 2.0 ** -23 * (W.double().abs() + s * (B.double().abs() @ A.double().abs()))
    err = (out.double() - ref).abs()
    print("merge fp32: max err / bound", float((err / bound).max()))
    assert bool((err <= bound).all())
    scaled = out.clone()
    scaled[:ns] *= scale
    assert torch.equal(dst, scaled.to(torch.bfloat16))      # one rounding of the kernel's own fp32 value
    assert torch.equal(dst_t, dst.t().contiguous())
    # each output alone gives the same bits
    d2, t2, o2 = torch.zeros_like(dst), torch.zeros_like(dst_t), torch.zeros_like(out)
    ops.lora_merge(W, A, B, s, dst=d2, nscaled=ns, scale=scale)
    ops.lora_merge(W, A, B, s, dst_t=t2, nscaled=ns, scale=scale)
    ops.lora_merge(W, A, B, s, out=o2)
    assert torch.equal(d2, dst) and torch.equal(t2, dst_t) and torch.equal(o2, out)


@pytest.mark.parametrize("r", [3, 8])
def test_merge_row_range_leaves_other_rows(r):
    """the v rows [512, 768) of a fused [768, 256] q|k|v pack and of its [256, 768] transpose, in place"""
    from vclip_amd import ops
    D = 256
    W = _randn(3 * D, D, seed=4, scale=0.05)
    A, B = _randn(r, D, seed=5, scale=0.1), _randn(D, r, seed=6, scale=0.1)
    qs = 0.125 * ops.LOG2E
    dst = torch.full((3 * D, D), 7.0, dtype=torch.bfloat16, device=DEV)
    dst_t = torch.full((D, 3 * D), 7.0, dtype=torch.bfloat16, device=DEV)
    out = torch.full((3 * D, D), 7.0, device=DEV)
    ops.lora_merge(W, A, B, 1.5, dst, dst_t, out, row0=2 * D, nscaled=D, scale=qs)
    assert bool((dst[:2 * D] == 7).all()) and bool((dst_t[:, :2 * D] == 7).all()) and bool((out[:2 * D] == 7).all())
    alone = torch.zeros(D, D, device=DEV)
    ops.lora_merge(W[2 * D:].contiguous(), A, B, 1.5, out=alone)
    assert torch.equal(out[2 * D:], alone)
    assert torch.equal(dst[2 * D:], alone.to(torch.bfloat16)) and torch.equal(dst_t[:, 2 * D:], dst[2 * D:].t())
    # the q rows [0, 256) carry the q scale
    ops.lora_merge(W, A, B, 1.5, dst, dst_t, out, row0=0, nscaled=D, scale=qs)
    assert torch.equal(dst[:D], (out[:D] * qs).to(torch.bfloat16)) and torch.equal(dst_t[:, :D], dst[:D].t())
    assert bool((dst[D:2 * D] == 7).all()) and torch.equal(dst[2 * D:], alone.to(torch.bfloat16))


@pytest.mark.parametrize("N,K", SHAPES + [(768, 256)])
def test_merge_with_zero_b_is_pack_weight(N, K):
    from vclip_amd import ops
    W, A = _randn(N, K, seed=7, scale=0.05), _randn(8, K, seed=8)
    B = torch.zeros(N, 8, device=DEV)
    ns, scale = (256, 0.18033688) if N == 768 else (0, 1.0)
    got, got_t = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV), torch.zeros(K, N, dtype=torch.bfloat16, device=DEV)
    ref, ref_t = torch.ones_like(got), torch.ones_like(got_t)
    ops.lora_merge(W, A, B, 2.0, got, got_t, nscaled=ns, scale=scale)
    ops.pack_weight(W, ref, ref_t, nscaled=ns, scale=scale)
    assert torch.equal(got, ref) and torch.equal(got_t, ref_t)


# ---- 2. adapter gradients ---------------------------------------------------------------------------------------
def _grad_case(M, N, K, r, real_rows=None):
    """x bf16 [M, K]; dy bf16 = columns [2N, 3N) of a [M, 3N] buffer (row stride 3N, as the v slice of dQKV)"""
    x = _randn(M, K, seed=11, dtype=torch.bfloat16)
    buf = _randn(M, 3 * N, seed=12, scale=0.01, dtype=torch.bfloat16)
    if real_rows is not None:
        x[real_rows:] = 0
        buf[real_rows:] = 0
    dy = buf[:, 2 * N:]
    A, B = _randn(r, K, seed=13, scale=K ** -0.5), _randn(N, r, seed=14, scale=0.02)
    return x, dy, A, B


def _run_grads(x, dy, A, B, c):
    from vclip_amd import ops
    M, (N, r), K = x.shape[0], B.shape, x.shape[1]
    dA, dB = torch.full((r, K), float("nan"), device=DEV), torch.full((N, r), float("nan"), device=DEV)
    uv = torch.zeros(M * r, dtype=torch.bfloat16, device=DEV)
    work = ops.lora_wgrad_work(max(N, K), r, DEV, splits=64)
    ops.lora_grads(x, dy, A, B, c, dA, dB, uv, work)
    return dA, dB


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("r", [3, 8, 64])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [64, 2080])  # one split; 33 splits of 64 rows with a 32-row last one
def test_adapter_gradients_against_fp64(M, N, K, r):
    x, dy, A, B = _grad_case(M, N, K, r)
    c = 0.37
    dA, dB = _run_grads(x, dy, A, B, c)
    xd, dyd = x.double(), dy.double()
    rB = c * dyd.t() @ (xd @ A.double().t())
    rA = c * (dyd @ B.double()).t() @ xd
    eA, eB = _rel(dA, rA), _rel(dB, rB)
    print(f"M={M} N={N} K={K} r={r}: rel L2 dA {eA:.2e} dB {eB:.2e} (bar {2.0 ** -7:.2e})")
    assert eA <= 2.0 ** -7 and eB <= 2.0 ** -7
    dA2, dB2 = _run_grads(x, dy, A, B, c)
    assert torch.equal(dA, dA2) and torch.equal(dB, dB2)


def test_adapter_gradients_zero_padded_rows():
    """18 real rows of 64, the rest zero (the engine's padded token rows): the padding adds nothing"""
    x, dy, A, B = _grad_case(64, 256, 256, 8, real_rows=18)
    dA, dB = _run_grads(x, dy, A, B, 1.0)
    xd, dyd = x[:18].double(), dy[:18].double()
    rB = dyd.t() @ (xd @ A.double().t())
    rA = (dyd @ B.double()).t() @ xd
    assert _rel(dA, rA) <= 2.0 ** -7 and _rel(dB, rB) <= 2.0 ** -7
    dA18, dB18 = _run_grads(x[:18].contiguous(), dy[:18], A, B, 1.0)
    assert torch.equal(dA, dA18) and torch.equal(dB, dB18)


# ---- the model ---------------------------------------------------------------------------------------------------
def _setup(B, seed=0):
    from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
    from vclip_amd.weights import make_synthetic_clips, make_vivit_weights
    sd = make_vivit_weights(SMALL, seed=seed)
    pix = make_synthetic_clips(B, SMALL["num_frames"], SMALL["image_size"], seed=1)
    labels = np.random.RandomState(2).randint(0, 2, size=B)
    model = VivitForVideoClassification(VivitConfig(**SMALL, id2label={0: "non-referral", 1: "referral"}))
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    return model, sd, torch.from_numpy(pix), torch.from_numpy(labels).long()


def _attach(model, randomize_b=True, **kw):
    from vclip_amd import lora
    lora.attach(model, **kw)
    if randomize_b:
        g = torch.Generator().manual_seed(9)
        with torch.no_grad():
            for k, p in model.lora_params.items():
                if k.endswith("lora_B__weight"):
                    p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))
    return model


def _ref_of(model, sd):
    from lora_ref import LoraRef
    from vclip_amd import lora
    lsd = lora.state_dict(model)
    cfg = lsd["lora_config"]
    return LoraRef(sd, SMALL, lsd, cfg["alpha"] / cfg["rank"], cfg["train_head"])


def _trainable(model):
    from vclip_amd import lora
    st = model._lora
    d = {n: st.param(model, n) for n in st.names}
    if st.train_head:
        d.update({n: model.P(n) for n in lora.HEAD})
    return d


def _compare(model, ref_grads, l2_tol=5e-2, cos_tol=0.998):
    worst = []
    tr = _trainable(model)
    assert sorted(tr) == sorted(ref_grads)
    for n, p in tr.items():
        assert p.grad is not None, n
        g, r = p.grad.detach().cpu().double().reshape(-1), ref_grads[n].double().reshape(-1)
        l2 = float((g - r).norm() / r.norm())
        cos = float(g @ r / (g.norm() * r.norm()))
        worst.append((l2, n, cos))
        assert l2 < l2_tol and cos > cos_tol, (n, l2, cos)
    for n, p in model.hf_state_dict().items():
        if n not in tr:
            assert p.grad is None and not p.requires_grad, n
    return max(worst)


def _step(model, pix, labels):
    out = model(pixel_values=pix.to(DEV))
    loss = torch.nn.functional.cross_entropy(out.logits, labels.to(DEV))
    loss.backward()
    return out.logits.detach().cpu(), float(loss.detach())


@pytest.mark.parametrize("targets,rank", [(("q", "v"), 4), (ALL6, 8)])
@pytest.mark.parametrize("B", [2, 3])
def test_model_gradients_match_autograd(B, targets, rank):
    model, sd, pix, labels = _setup(B)
    _attach(model, rank=rank, alpha=2.0 * rank, targets=targets)
    logits, loss = _step(model, pix, labels)
    ref_loss, ref_logits, ref_grads = _ref_of(model, sd).grads(pix, labels)
    np.testing.assert_allclose(logits.numpy(), ref_logits.numpy(), rtol=0, atol=1e-2)
    assert abs(loss - ref_loss) < 1e-2
    print("worst gradient (rel L2, name, cos):", _compare(model, ref_grads))


def test_model_gradients_with_zero_b():
    """freshly attached: dA is exactly 0 (it is c (dy B)^T x with B = 0), dB and the head match autograd"""
    model, sd, pix, labels = _setup(2)
    _attach(model, randomize_b=False, rank=4, targets=ALL6)
    _step(model, pix, labels)
    _, _, ref_grads = _ref_of(model, sd).grads(pix, labels)
    for n, p in _trainable(model).items():
        if n.endswith("lora_A.weight"):
            assert bool((p.grad == 0).all()) and not ref_grads[n].any(), n
    tr = _trainable(model)
    assert all(p.grad is None for n, p in model.hf_state_dict().items() if n not in tr)
    for n, r in ref_grads.items():
        if not n.endswith("lora_A.weight"):
            g = tr[n].grad.detach().cpu().double().reshape(-1)
            r = r.double().reshape(-1)
            assert float((g - r).norm() / r.norm()) < 5e-2 and float(g @ r / (g.norm() * r.norm())) > 0.998, n


def test_last_layer_only_stops_the_chain():
    """layers=1 of 2: the gradients match, and the backward records no weight gradient at all and no data-gradient
    GEMM of layer 0 (the chain ends at layer 1's q|k|v adapters)"""
    from vclip_amd import ops
    model, sd, pix, labels = _setup(2)
    _attach(model, rank=4, targets=("q", "v"), layers=1)
    assert sorted({int(n.split(".")[2]) for n in model._lora.names}) == [1]
    rec = ops.OpRecorder()
    with ops.recording(rec):
        _step(model, pix, labels)
    torch.cuda.synchronize()
    _, _, ref_grads = _ref_of(model, sd).grads(pix, labels)
    _compare(model, ref_grads)
    names = [op for _, op, *_ in rec.entries]
    assert "wgrad" not in names
    dgrad = [op for op in names if op.startswith("dgrad.")]
    assert sorted(dgrad) == ["dgrad.l1.fc1", "dgrad.l1.fc2", "dgrad.l1.o"], dgrad   # not even layer 1's own q|k|v^T
    assert names.count("lora_down") == 4 and names.count("lora_wgrad") == 4           # two adapters, dA and dB each


@pytest.mark.parametrize("targets,dgrad", [(("fc2",), []), (("fc1",), ["fc2"]), (("o", "fc2"), ["fc1", "fc2"])])
def test_chain_stops_at_the_lowest_layers_last_adapter(targets, dgrad):
    """the lowest adapted layer runs only the data-gradient GEMMs its last adapter gradient needs (fc2's needs none:
    its dy is the block's incoming gradient); the gradients still match"""
    from vclip_amd import ops
    model, sd, pix, labels = _setup(2)
    _attach(model, rank=4, targets=targets, layers=1)
    rec = ops.OpRecorder()
    with ops.recording(rec):
        _step(model, pix, labels)
    torch.cuda.synchronize()
    _compare(model, _ref_of(model, sd).grads(pix, labels)[2])
    got = sorted(op for _, op, *_ in rec.entries if op.startswith("dgrad."))
    assert got == sorted(f"dgrad.l1.{g}" for g in dgrad), got


def test_side_stream_off_and_accumulation():
    """the adapter gradients on the caller's stream are the side stream's bits; a second backward without zero_grad
    accumulates, as torch's"""
    model, sd, pix, labels = _setup(2)
    _attach(model, rank=4, targets=ALL6)
    gs = []
    for side in (True, False, True):
        model.zero_grad(set_to_none=True)
        x = pix.to(DEV)
        model(pixel_values=x)  # the engine exists after one forward
        model._train_engine(x.shape[0], x.device).side_wgrad = side
        _step(model, pix, labels)
        torch.cuda.synchronize()
        gs.append({n: p.grad.detach().clone() for n, p in _trainable(model).items()})
    for n in gs[0]:
        assert torch.equal(gs[0][n], gs[1][n]) and torch.equal(gs[0][n], gs[2][n]), n
    _step(model, pix, labels)  # no zero_grad: accumulates
    for n, p in _trainable(model).items():
        torch.testing.assert_close(p.grad, 2 * gs[0][n], rtol=1e-5, atol=1e-7)
    assert all(p.grad is None for n, p in model.hf_state_dict().items() if n not in _trainable(model))


def test_zero_adapters_leave_train_logits_bit_identical():
    plain, _, pix, labels = _setup(2)
    want = plain(pixel_values=pix.to(DEV)).logits.detach().clone()
    model, _, _, _ = _setup(2)
    _attach(model, randomize_b=False, rank=8, targets=ALL6)
    got = model(pixel_values=pix.to(DEV)).logits.detach()
    assert torch.equal(got, want)


def test_three_steps_of_the_reference_loop():
    """vclip AdamW over the requires_grad parameters vs torch AdamW on the reference's A, B and head.  B starts at
    0.02 randn, not 0: from B = 0 the first step's dA is exactly 0 and A's first update is weight decay alone, which
    would leave the 0.1 bar on A's accumulated update to two sign-like steps."""
    from vclip_amd.optim import AdamW
    model, sd, pix, labels = _setup(2)
    _attach(model, rank=4, alpha=8.0, targets=("q", "v"))
    ref = _ref_of(model, sd)
    start = {n: p.detach().cpu().clone() for n, p in _trainable(model).items()}
    frozen0 = {n: p.detach().clone() for n, p in model.hf_state_dict().items() if not p.requires_grad}
    params = [p for p in model.parameters() if p.requires_grad]
    ntrain = sum(p.numel() for p in params)
    assert ntrain == 2 * 2 * 4 * (256 + 256) + 2 * 256 + 2  # layers x targets x r (in + out), and the head
    opt = AdamW(params, lr=1e-3, weight_decay=0.01)
    ropt = torch.optim.AdamW(list(ref.trainable().values()), lr=1e-3, weight_decay=0.01)
    crit = torch.nn.CrossEntropyLoss()
    losses, rlosses = [], []
    for _ in range(3):
        opt.zero_grad()
        loss = crit(model(pixel_values=pix.to(DEV)).logits, labels.to(DEV))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        ropt.zero_grad()
        rl = crit(ref.forward(pix), labels)
        rl.backward()
        ropt.step()
        rlosses.append(float(rl.detach()))
    np.testing.assert_allclose(losses, rlosses, rtol=0, atol=2e-2)
    rt = ref.trainable()
    for n, p in _trainable(model).items():
        du = p.detach().cpu().double() - start[n].double()
        dr = rt[n].detach().double() - start[n].double()
        e = float((du - dr).abs().mean() / dr.abs().mean().clamp_min(1e-12))
        print(f"{n}: accumulated update error {e:.3f}")
        assert e < 0.1, (n, e)
    for n, p in model.hf_state_dict().items():
        if n in frozen0:
            assert torch.equal(p.detach(), frozen0[n]), n
    moments = 0
    for st in opt.state.values():
        moments += sum(v.numel() for k, v in st.items() if k in ("exp_avg", "exp_avg_sq"))
    assert moments == 2 * ntrain
    # and no gradient buffer of the full layout was made
    assert model._gflat is None and model._gscratch is None


def test_merge_is_bit_identical_and_the_model_trains_on():
    from vclip_amd import lora
    from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
    model, sd, pix, labels = _setup(2)
    _attach(model, rank=8, alpha=16.0, targets=ALL6)
    x = pix.to(DEV)
    model.eval()
    with torch.no_grad():
        attached = model(pixel_values=x).logits.clone()
    msd = lora.merged_state_dict(model)
    assert list(msd) == list(model.state_dict()) and "lora_params" in dict(model.named_children())
    fresh = VivitForVideoClassification(VivitConfig(**SMALL, id2label={0: "non-referral", 1: "referral"}))
    fresh.load_state_dict({k: v.cpu() for k, v in msd.items()})
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(fresh(pixel_values=x).logits, attached)
    plain = _setup(2)[0].eval()
    with torch.no_grad():
        assert not torch.equal(plain(pixel_values=x).logits, attached)  # the adapters do something
    assert lora.merge(model) is model and model._lora is None
    assert all(torch.equal(model.state_dict()[k], msd[k]) for k in msd)
    with torch.no_grad():
        assert torch.equal(model(pixel_values=x).logits, attached)
    # a plain model again: one full train step, every parameter gets a gradient
    assert all(p.requires_grad for p in model.parameters()) and len(list(model.parameters())) == len(msd)
    model.train()
    _step(model, pix, labels)
    assert all(p.grad is not None for p in model.parameters())
    assert bool(model.P("vivit.layers.0.mlp.fc1.weight").grad.abs().sum() > 0)


def test_unsupported_combinations_are_refused():
    from vclip_amd import dp, lora
    from vclip_amd.optim import AdamW
    from vclip_amd.vivit_train import GraphedTrainStep
    model, sd, pix, labels = _setup(2)
    _attach(model, rank=4)
    x, y = pix.to(DEV), labels.to(DEV)
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    with pytest.raises(NotImplementedError, match="GraphedTrainStep"):
        GraphedTrainStep(model, opt, torch.nn.CrossEntropyLoss(), x, y)
    with pytest.raises(NotImplementedError, match="GradAllReduce"):
        dp.GradAllReduce(model)
    model.grad_ready_hooks.append(lambda *a: None)
    with pytest.raises(NotImplementedError, match="grad_ready_hooks"):
        torch.nn.functional.cross_entropy(model(pixel_values=x).logits, y).backward()
    model.grad_ready_hooks.clear()
    model.eval()
    with pytest.raises(NotImplementedError, match="grad_rollout"):
        model.explain(x, method="grad_rollout")
    model.compute_dtype, model.precise_layers = torch.float16, 1
    with pytest.raises(NotImplementedError, match="precise_layers"):
        model(pixel_values=x)
    model.compute_dtype, model.precise_layers = torch.bfloat16, 0
    # merged, the model is an ordinary one: the same calls run
    lora.merge(model)
    assert model.explain(x, method="grad_rollout").saliency.shape[0] == 2
    model.train()
    opt = AdamW(model.parameters(), lr=1e-3)
    step = GraphedTrainStep(model, opt, torch.nn.CrossEntropyLoss(), x, y)
    assert bool(torch.isfinite(step(x, y)))
