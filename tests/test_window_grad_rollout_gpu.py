"""Class-specific Video Swin saliency on the GPU: the gradient-weighted window rollout step (csrc/window_rollout.hip,
vc_window_grad_rollout_step) against the same formula in fp64, its exact and structural cases, and
Swin3d.explain_class against the a / base rollout computed from the fp32 oracle's materialised probabilities and its
autograd gradients (tests/window_grad_rollout_ref.py).

Bounds (measured figures: DESIGN.md section 4):
  kernel  max|got - ref64| / max|ref64| <= 8 x the same formula in fp32 torch on the CPU against ref64, per shape (the
          sibling steps' bound): the bf16 inputs are identical and their products exact in fp32, so only the exp2
          rounding and the summation order differ.
  model   E(x) = max|x - ref| / max|ref| on the normalised maps, ref the fp32 oracle's stepwise map; E of the GPU map <=
          MODEL_FACTOR x E of the oracle with q, k rounded to bf16 before every softmax and v, dO before dP, per clip
          and target.  The factor is not derivable (the GPU chain also carries the bf16 GEMM rounding of the train
          path's forward and backward): by the rule of test_window_rollout_gpu.py's docstring it is the smallest power
          of two at least twice the largest measured ratio.  MEASURED_RATIOS below are E(gpu) / E(bf16 oracle) on the
          (T, target, clip) cases, sharpened TINY weights, B = 2: 2.03 to 4.85, at yardsticks of 0.96e-3 to 1.8e-3 and
          E(gpu) of 3.3e-3 to 5.7e-3; twice the largest is 9.7, so MODEL_FACTOR = 16 (window_grad_rollout_ref.py).
          16 x the largest yardstick (<= 0.031) stays under a quarter of the smallest E between the two classes' maps
          (0.75 / 4 = 0.19), which test_window_grad_rollout_cpu.py checks.
"""
import pytest
import torch

import window_grad_rollout_ref as G
import window_rollout_ref as R
from test_window_rollout_gpu import NAN16, STEP_CASES, make_table, rel_err
from vclip_amd import _lib, ops
from vclip_amd.weights import make_swin3d_weights, make_synthetic_video

pytestmark = pytest.mark.gpu
# E(gpu) / E(bf16 oracle): T = 8 then T = 4; per T the targets 0, 1 and None; per target clip 0, clip 1
MEASURED_RATIOS = (2.77, 2.95, 2.92, 2.03, 2.77, 2.03, 2.59, 4.85, 3.39, 3.75, 2.59, 4.85)
ALPHA_BETA = ((1.0, 1.0), (1.0, 0.0), (0.5, 1.0))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ kernel: inputs
def make_qkv(B, grid, C, seed, qmul=0.64):
    """bf16 q'|k|v rows in the token layout (scores q'.k over 32 dims of standard deviation 3.6), NaN in every row past
    B*T*H*W; v is read here, so it is real"""
    n = B * grid[0] * grid[1] * grid[2]
    x = torch.randn(n + 8, 3 * C, generator=torch.Generator().manual_seed(seed))
    x[:, :C] *= qmul
    x = x.to(torch.bfloat16)
    x.view(torch.int16)[n:] = torch.tensor(NAN16, dtype=torch.int16)
    return x


def make_dout(B, grid, C, seed, pitch=16):
    """bf16 dO rows with a leading dimension of C + pitch: NaN in the pitch columns and in every row past B*T*H*W"""
    n = B * grid[0] * grid[1] * grid[2]
    x = torch.randn(n + 8, C + pitch, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)
    nan = torch.tensor(NAN16, dtype=torch.int16)
    x.view(torch.int16)[n:] = nan
    x.view(torch.int16)[:, C:] = nan
    return x


def vectors(n, seed):
    """(r_in, a_in) pairs: uniform (a base-like r over a small a) and random"""
    g = torch.Generator().manual_seed(seed)
    return {"uniform": (torch.full((n,), 1.0 / n), torch.full((n,), 1e-4 / n)),
            "random": (torch.rand(n, generator=g) + 0.05, torch.rand(n, generator=g) * 0.1)}


def run_step(qkv_d, dout_d, table_d, r, a, B, grid, heads, window, shift, full, alpha, beta, base=None):
    """(a_out, r_out or None) on the host; the outputs and the scratch start as NaN"""
    nan = lambda k: torch.full((k,), float("nan"), device="cuda")  # noqa: E731
    a_out = nan(r.numel())
    r_out = None if base is None else nan(r.numel())
    work = ops.window_grad_rollout_work(B, grid, heads, "cuda").fill_(float("nan"))
    ops.window_grad_rollout_step(qkv_d, dout_d, table_d, r.cuda(), a.cuda(), B, grid, heads, window, shift, full, alpha, beta,
                                 work, a_out, base=None if base is None else base.cuda(), r_out=r_out)
    return a_out.cpu(), None if r_out is None else r_out.cpu()


# ------------------------------------------------------------------ 1. step against fp64
@pytest.mark.parametrize("B,grid,C,full,shift_full,tab_scale", STEP_CASES)
def test_window_grad_rollout_step_matches_fp64(B, grid, C, full, shift_full, tab_scale):
    heads = C // 32
    window, shift = R.O.window_and_shift(grid, full, shift_full)
    n = B * grid[0] * grid[1] * grid[2]
    qkv = make_qkv(B, grid, C, seed=C + sum(shift_full) + grid[0])
    dout = make_dout(B, grid, C, seed=C + grid[1])
    table = make_table(full, heads, seed=7, scale=tab_scale)
    qkv_d, dout_d, table_d = qkv.cuda(), dout.cuda(), table.cuda()
    assert dout_d.stride(0) > heads * 32
    errs, yard = {}, 0.0
    for name, (r, a) in vectors(n, seed=grid[1]).items():
        for alpha, beta in ALPHA_BETA:
            args = (qkv, dout, table, r, a, B, grid, heads, window, shift, full, alpha, beta)
            ref = G.grad_step_ref(*args, torch.float64)
            yard = max(yard, rel_err(G.grad_step_ref(*args, torch.float32), ref))
            got, _ = run_step(qkv_d, dout_d, table_d, r, a, B, grid, heads, window, shift, full, alpha, beta)
            assert torch.isfinite(got).all(), (name, alpha, beta)  # no NaN row or column, no padded slot reached it
            errs[(name, alpha, beta)] = rel_err(got, ref)
    print(f"window grad rollout step {(B, grid, C, tuple(window), tuple(shift), tab_scale)}: fp32 yardstick {yard:.3e}, "
          f"bound {8 * yard:.3e}, kernel " + ", ".join(f"{k[0]}/{k[1]}/{k[2]}: {v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) <= 8 * yard, (errs, yard)


# ------------------------------------------------------------------ 2. exact and structural cases
CASE = (2, (4, 6, 6), 64, (2, 3, 3), (1, 1, 1))


def _case_inputs(seed=3):
    B, grid, C, full, shift = CASE
    n = B * grid[0] * grid[1] * grid[2]
    r, a = vectors(n, seed=seed)["random"]
    return make_qkv(B, grid, C, seed=seed), make_dout(B, grid, C, seed=seed + 1), make_table(full, C // 32, seed=4), r, a, n


def test_zero_gradient_leaves_the_carried_part_and_r_out_is_a_out_plus_base():
    B, grid, C, full, shift = CASE
    qkv, dout, table, r, a, n = _case_inputs()
    heads = C // 32
    zero = dout.clone()
    zero[:n, :C] = 0
    for alpha, beta in ALPHA_BETA:
        got, _ = run_step(qkv.cuda(), zero.cuda(), table.cuda(), r, a, B, grid, heads, full, shift, full, alpha, beta)
        assert torch.equal(got, beta * a), (alpha, beta)
    base = torch.rand(n, generator=torch.Generator().manual_seed(9)) + 0.5
    a_out, r_out = run_step(qkv.cuda(), dout.cuda(), table.cuda(), r, a, B, grid, heads, full, shift, full, 1.0, 1.0, base)
    alone, _ = run_step(qkv.cuda(), dout.cuda(), table.cuda(), r, a, B, grid, heads, full, shift, full, 1.0, 1.0)
    assert torch.isfinite(a_out).all() and float((a_out - a).abs().max()) > 0
    assert torch.equal(r_out, a_out + base) and torch.equal(a_out, alone)


def test_constant_gradient_is_the_plain_step_scaled_and_its_negation_is_nothing():
    """every dO row and every v row equal to one vector c per head: dP = |c|^2 > 0 everywhere, so the step is |c|^2 x the
    plain rollout step's attention term; with dO negated every dP is negative and nothing is added"""
    B, grid, C, full, shift = CASE
    qkv, dout, table, r, a, n = _case_inputs(seed=5)
    heads = C // 32
    c = (torch.arange(32) % 5 - 2).float() * 0.25  # multiples of 1/4: c and |c|^2 are exact in bf16 / fp32
    c[0] = 0.75
    c2 = float((c.double() ** 2).sum())
    qkv[:n, 2 * C:] = c.repeat(heads).bfloat16()
    dout[:n, :C] = c.repeat(heads).bfloat16()
    got, _ = run_step(qkv.cuda(), dout.cuda(), table.cuda(), r, a, B, grid, heads, full, shift, full, 1.0, 0.0)
    plain = torch.full((n,), float("nan"), device="cuda")
    ops.window_rollout_step(qkv.cuda(), table.cuda(), r.cuda(), B, grid, heads, full, shift, full, 1.0,
                            ops.window_rollout_work(B, grid, heads, "cuda"), plain)
    want = c2 * plain.cpu().double()
    assert float(((got.double() - want).abs() / want).max()) <= 1e-6
    neg = dout.clone()
    neg[:n, :C] = -neg[:n, :C]
    for alpha, beta in ALPHA_BETA:
        got, _ = run_step(qkv.cuda(), neg.cuda(), table.cuda(), r, a, B, grid, heads, full, shift, full, alpha, beta)
        assert torch.equal(got, beta * a), (alpha, beta)


def test_window_grad_rollout_step_deterministic_and_batch_invariant():
    B, grid, C, full, shift = 3, (4, 6, 6), 64, (2, 3, 3), (1, 1, 1)
    heads, n1 = C // 32, 4 * 6 * 6
    qkv, dout = make_qkv(B, grid, C, seed=11), make_dout(B, grid, C, seed=12)
    table = make_table(full, heads, seed=5).cuda()
    r, a = vectors(B * n1, seed=5)["random"]
    x, _ = run_step(qkv.cuda(), dout.cuda(), table, r, a, B, grid, heads, full, shift, full, 1.0, 1.0)
    y, _ = run_step(qkv.cuda(), dout.cuda(), table, r, a, B, grid, heads, full, shift, full, 1.0, 1.0)
    assert torch.equal(x, y)
    q1, d1 = make_qkv(1, grid, C, seed=0), make_dout(1, grid, C, seed=1)
    q1[:n1] = qkv[n1:2 * n1]
    d1[:n1] = dout[n1:2 * n1]
    z, _ = run_step(q1.cuda(), d1.cuda(), table, r[n1:2 * n1].contiguous(), a[n1:2 * n1].contiguous(), 1, grid, heads, full,
                    shift, full, 1.0, 1.0)
    assert torch.equal(x[n1:2 * n1], z)


def test_an_oversized_window_is_refused_before_any_launch():
    """a window whose q' and dO rows cannot be staged in the LDS (784 slots): an error, the outputs untouched"""
    B, grid, C, full = 1, (16, 14, 14), 32, (8, 14, 7)
    n = 16 * 14 * 14
    qkv, dout = make_qkv(B, grid, C, seed=1).cuda(), make_dout(B, grid, C, seed=2).cuda()
    table = make_table(full, 1, seed=3).cuda()
    r, a = vectors(n, seed=1)["random"]
    a_out = torch.full((n,), float("nan"), device="cuda")
    work = ops.window_grad_rollout_work(B, grid, 1, "cuda").fill_(float("nan"))
    with pytest.raises(_lib.VclipError, match="448"):
        ops.window_grad_rollout_step(qkv, dout, table, r.cuda(), a.cuda(), B, grid, 1, full, (0, 0, 0), full, 1.0, 1.0, work,
                                     a_out)
    torch.cuda.synchronize()
    assert torch.isnan(a_out).all() and torch.isnan(work).all()


# ------------------------------------------------------------------ 3. model against the oracle
def _model(cfg, sd=None, seed=0):
    from vclip_amd.swin3d import Swin3d
    m = Swin3d({k: v for k, v in cfg.items() if k != "num_classes"}, num_classes=cfg["num_classes"])
    m.load_state_dict(make_swin3d_weights(cfg, seed=seed) if sd is None else sd)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def sharp():
    sd = R.sharpen({k: torch.from_numpy(v) for k, v in make_swin3d_weights(R.TINY, seed=0).items()})
    return sd, _model(R.TINY, sd)


_ORACLE = {}


def _oracle(sd, T, HW, tg):
    """(logits, grids, the fp32 oracle's normalised map, the bf16 yardstick's) for both clips explained as class tg;
    computed once per (T, tg) and shared"""
    if (T, tg) not in _ORACLE:
        video = torch.from_numpy(make_synthetic_video(2, T, HW, seed=3))
        logits, _, grids, mats = G.oracle_grads(sd, R.TINY, video, tg)
        _, _, _, mats16 = G.oracle_grads(sd, R.TINY, video, tg, round16=True)
        a, _ = G.rollout_stepwise(mats, grids)
        a16, _ = G.rollout_stepwise(mats16, grids)
        _ORACLE[(T, tg)] = (logits, grids, G.saliency(a), G.saliency(a16))
    return _ORACLE[(T, tg)]


@pytest.mark.parametrize("target", [0, 1, None])
@pytest.mark.parametrize("T,HW", [(8, 48), (4, 48)])
def test_explain_class_matches_the_oracle(sharp, T, HW, target):
    sd, m = sharp
    video = torch.from_numpy(make_synthetic_video(2, T, HW, seed=3)).cuda()
    before = m(video).clone()
    ex = m.explain_class(video, target=target)
    B = 2
    want_logits, grids, _, _ = _oracle(sd, T, HW, 0)
    t0, h0, w0 = grids[0]
    n0 = t0 * h0 * w0
    assert (t0, h0, w0) == (T // 2, HW // 4, HW // 4)
    assert tuple(ex.token_relevance.shape) == (B, n0) and tuple(ex.saliency.shape) == (B, t0, h0, w0)  # no CLS column
    assert tuple(ex.temporal.shape) == (B, t0) and tuple(ex.logits.shape) == (B, 2)
    assert all(x.dtype == torch.float32 for x in (ex.logits, ex.token_relevance, ex.saliency, ex.temporal))
    assert ex.logits.device.type == "cuda" and ex.token_relevance.device.type == "cpu"
    assert ex.method == "class_rollout"
    assert ex.target == ([target] * B if target is not None else ex.logits.argmax(dim=1).tolist())
    assert float((ex.logits.cpu() - want_logits).abs().max()) < 1e-2
    assert torch.isfinite(ex.token_relevance).all() and (ex.token_relevance >= 0).all() and (ex.saliency >= 0).all()
    assert ((ex.saliency.double().sum(dim=(1, 2, 3)) - 1).abs() < 1e-5).all()
    assert torch.equal(ex.temporal, ex.saliency.sum(dim=(2, 3)))
    sal = ex.saliency.reshape(B, n0)
    for b in range(B):
        _, _, ref, ref16 = _oracle(sd, T, HW, ex.target[b])
        yard, err = G.E(ref16[b], ref[b]), G.E(sal[b], ref[b])
        print(f"explain_class T = {T} target {target} clip {b} (class {ex.target[b]}): bf16 oracle yardstick {yard:.3e}, "
              f"GPU {err:.3e}, ratio {err / yard:.2f}")
        assert err <= G.MODEL_FACTOR * yard, (b, err, yard)
    # nothing of the model moved: no gradient on a parameter, the same forward bits
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(m(video), before)


def test_explain_class_leaves_the_forward_untouched_and_feeds_faithfulness():
    from vclip_amd.faithfulness import faithfulness
    m = _model(R.TINY)
    video = torch.from_numpy(make_synthetic_video(2, 8, 48, seed=3)).cuda()
    m.graph_replay = True
    before = m(video).clone()
    assert torch.equal(m(video), before)
    captures, packed, bias = m._graphs.captures, m._packed, m._bias_cache
    ws = dict(m._ws)
    bias_items = dict(bias)
    ex = m.explain_class(video, target=[1, 0])
    assert ex.target == [1, 0]
    again = m.explain_class(video, target=[1, 0])
    assert torch.equal(again.token_relevance, ex.token_relevance) and torch.equal(again.logits, ex.logits)
    assert torch.equal(m(video), before)
    assert m._graphs.captures == captures  # explain_class invalidated nothing
    assert m._packed is packed and m._bias_cache is bias
    assert set(m._bias_cache) == set(bias_items) and all(m._bias_cache[k] is v for k, v in bias_items.items())
    assert set(m._ws) == set(ws) and all(m._ws[k] is v for k, v in ws.items())
    assert all(p.grad is None for p in m.parameters()) and all(p.requires_grad for p in m.parameters())
    assert not m.training and m.EXPLAIN_METHODS == ("rollout",)
    m.graph_replay = False
    assert torch.equal(m(video), before)
    chk = faithfulness(m, video, ex, steps=4, target=ex.target)  # scored for the classes the map explains
    assert chk["target"] == [1, 0] and all(torch.isfinite(chk[k]).all() for k in ("deletion_auc", "insertion_auc"))
    # the refusals on the device
    for bad in (2, [0, 1, 0]):
        with pytest.raises(ValueError, match="target"):
            m.explain_class(video, target=bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain_class(video.cpu())
    with pytest.raises(ValueError, match=r"\[B, 3, T, H, W\]"):
        m.explain_class(video[:, :2].contiguous())
    with pytest.raises(ValueError, match="multiples of the patch size"):
        m.explain_class(video[:, :, :, :46].contiguous())
    with pytest.raises(ValueError, match="whole windows"):  # 40 / 4 = 10 rows: not whole windows of 3
        m.explain_class(video[:, :, :, :40, :40].contiguous())
    with pytest.raises(ValueError, match="method"):
        m.explain(video, method="class_rollout")
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.explain_class(video)
    m.eval()
    assert torch.equal(m(video), before)


# ------------------------------------------------------------------ 4. the chain: the skips change no data gradient
def test_frozen_chain_returns_the_data_gradients_of_the_full_chain_bit_for_bit():
    """the backwards that skip their weight gradients (needs_input_grad) hand on the same dO of every block as the chain
    that forms them, and the forward's logits are the same bits; with a stochastic-depth probability in the config, as
    Swin-T has, which both chains must leave off"""
    m = _model(dict(R.TINY, stochastic_depth_prob=0.5))
    assert m.stochastic_depth
    video = torch.from_numpy(make_synthetic_video(2, 4, 48, seed=3)).cuda()
    lf, df, qf = m._class_chain(video, [1, 0], frozen=True)
    lw, dw, qw = m._class_chain(video, [1, 0], frozen=False)
    assert torch.equal(lf, lw) and len(df) == len(dw) == sum(R.TINY["depths"])
    for x, y in zip(df, dw):
        assert x.dtype == torch.bfloat16 and torch.equal(x, y)
    for x, y in zip(qf, qw):
        assert torch.equal(x, y)
    assert all(p.grad is None for p in m.parameters()) and m.stochastic_depth
