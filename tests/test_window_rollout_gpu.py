"""Video Swin saliency on the GPU: the window rollout step and the PatchMerging hop (csrc/window_rollout.hip) against
the same formulas in fp64, and Swin3d.explain against attention rollout computed from the fp32 oracle's materialised
probabilities (tests/window_rollout_ref.py).

Bounds (measured figures: DESIGN.md section 4):
  kernel  max|got - ref64| / max|ref64| <= 8 x the same formula in fp32 torch on the CPU against ref64, per shape: the
          inputs are identical, so only the exp2 rounding and the summation order differ (the sibling steps' bound);
          sum r_out = sum r_in within 8 x the fp32 formula's own conservation error;
  model   E(x) = max|x - ref| / max|ref - 1/N_0| (the deviation from uniform is the signal) of the GPU map <=
          MODEL_FACTOR x E of the oracle with q and k rounded to bf16 before every softmax, per clip.  The factor is not
          derivable (the GPU also carries the forward's bf16 GEMM rounding): it is the smallest power of two at least
          twice the largest measured ratio, as test_grad_rollout_gpu.py's.  Measured E(gpu) / E(bf16 oracle) on the
          four (fixture, clip) cases, sharpened TINY weights, B = 2 (MEASURED_RATIOS): 2.59, 3.09, 2.07, 2.21, at
          yardsticks of 1.6e-3 to 2.4e-3 and E(gpu) of 4.2e-3 to 5.0e-3; twice the largest is 6.2, so MODEL_FACTOR = 8
          (window_rollout_ref.py).  8 x the yardstick (<= 0.019) stays under a quarter of the smallest wrong-rule E
          (0.33 / 4 = 0.083), which test_window_rollout_cpu.py checks.
"""
import numpy as np
import pytest
import torch

import window_rollout_ref as R
from vclip_amd import ops
from vclip_amd.weights import make_swin3d_weights, make_synthetic_video

pytestmark = pytest.mark.gpu
NAN16 = 0x7FC0  # a bf16 quiet NaN
# E(gpu) / E(bf16-q/k oracle), (T = 8, clip 0), (T = 8, clip 1), (T = 4, clip 0), (T = 4, clip 1)
MEASURED_RATIOS = (2.59, 3.09, 2.07, 2.21)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# ------------------------------------------------------------------ kernel: inputs
def make_qkv(B, grid, C, seed, qmul=0.64):
    """bf16 q'|k|v rows in the token layout (scores q'.k over 32 dims of standard deviation 3.6, extremes +-15), NaN in
    the v columns (never read) and in every row past B*T*H*W"""
    n = B * grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n + 8, 3 * C, generator=g)
    x[:, :C] *= qmul
    x = x.to(torch.bfloat16)
    nan = torch.tensor(NAN16, dtype=torch.int16)
    x.view(torch.int16)[n:] = nan
    x.view(torch.int16)[:, 2 * C:] = nan
    return x


def make_table(full, heads, seed, scale=0.5):
    ntab = (2 * full[0] - 1) * (2 * full[1] - 1) * (2 * full[2] - 1)
    return torch.randn(ntab, heads, generator=torch.Generator().manual_seed(seed)) * scale


def r_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return {"uniform": torch.full((n,), 1.0 / n), "random": torch.rand(n, generator=g) + 0.05}


def run_step(qkv_d, table_d, r, B, grid, heads, window, shift, full, alpha):
    out = torch.full((r.numel(),), float("nan"), device="cuda")
    work = ops.window_rollout_work(B, grid, heads, "cuda").fill_(float("nan"))
    ops.window_rollout_step(qkv_d, table_d, r.cuda(), B, grid, heads, window, shift, full, alpha, work, out)
    return out.cpu()


STEP_CASES = [(2, (4, 6, 6), 32, (2, 3, 3), (0, 0, 0), 0.5),
              (2, (4, 6, 6), 64, (2, 3, 3), (1, 1, 1), 0.5),
              (1, (16, 14, 14), 96, (8, 7, 7), (4, 3, 3), 0.5),   # the full 392-token window, padded to 448
              (1, (16, 7, 7), 64, (8, 7, 7), (4, 3, 3), 0.5),     # window == grid in h, w: the shift dropped there
              (1, (2, 6, 6), 32, (2, 3, 3), (1, 1, 1), 0.5),      # t == window: the t shift dropped
              (2, (4, 6, 6), 64, (2, 3, 3), (1, 1, 1), 5.0)]      # a table of trained magnitude


# ------------------------------------------------------------------ 1. step against fp64, conservation
@pytest.mark.parametrize("B,grid,C,full,shift_full,tab_scale", STEP_CASES)
def test_window_rollout_step_matches_fp64(B, grid, C, full, shift_full, tab_scale):
    heads = C // 32
    window, shift = R.O.window_and_shift(grid, full, shift_full)
    n = B * grid[0] * grid[1] * grid[2]
    qkv = make_qkv(B, grid, C, seed=C + sum(shift_full) + grid[0])
    table = make_table(full, heads, seed=7, scale=tab_scale)
    qkv_d, table_d = qkv.cuda(), table.cuda()
    errs, yard, cons, cons_yard = {}, 0.0, 0.0, 0.0
    for name, r in r_inputs(n, seed=grid[1]).items():
        for alpha in (1.0, 0.5):
            ref = R.step_ref(qkv, table, r, B, grid, heads, window, shift, full, alpha, torch.float64)
            ref32 = R.step_ref(qkv, table, r, B, grid, heads, window, shift, full, alpha, torch.float32)
            yard = max(yard, rel_err(ref32, ref))
            got = run_step(qkv_d, table_d, r, B, grid, heads, window, shift, full, alpha)
            assert torch.isfinite(got).all(), (name, alpha)  # no NaN row or column, no padded slot reached it
            errs[(name, alpha)] = rel_err(got, ref)
            total = float(r.double().sum())
            cons = max(cons, abs(float(got.double().sum()) - total) / total)
            cons_yard = max(cons_yard, abs(float(ref32.double().sum()) - total) / total)
    print(f"window rollout step {(B, grid, C, tuple(window), tuple(shift), tab_scale)}: fp32 yardstick {yard:.3e}, bound "
          f"{8 * yard:.3e}, kernel " + ", ".join(f"{k[0]}/a={k[1]}: {v:.3e}" for k, v in errs.items())
          + f"; conservation kernel {cons:.3e}, fp32 formula {cons_yard:.3e}")
    assert max(errs.values()) <= 8 * yard, (errs, yard)
    assert cons <= 8 * cons_yard, (cons, cons_yard)


# ------------------------------------------------------------------ 2. exact and structural cases
def test_window_rollout_step_alpha_and_uniform_attention():
    """q = 0, a zero table and no shift give a uniform P per window: r_out[j] = alpha * mean_win(r_in) + (1 - alpha) *
    r_in[j]; and r_out - (1 - alpha) r_in scales with alpha"""
    B, grid, C, full = 2, (4, 6, 6), 64, (2, 3, 3)
    heads, n = C // 32, 2 * 4 * 6 * 6
    qkv = make_qkv(B, grid, C, seed=1)
    qkv[:n, :C] = 0
    table = torch.zeros(3 * 5 * 5, heads)
    r = r_inputs(n, seed=2)["random"]
    win_mean = R._unpartition(R._partition(r.reshape(B, *grid, 1), full, (0, 0, 0)).mean(1, keepdim=True).expand(-1, 18, -1)
                              .contiguous(), B, grid, full, (0, 0, 0)).reshape(-1).double()
    for alpha in (1.0, 0.5, 0.25):
        got = run_step(qkv.cuda(), table.cuda(), r, B, grid, heads, full, (0, 0, 0), full, alpha).double()
        want = alpha * win_mean + (1 - alpha) * r.double()
        assert float(((got - want).abs() / want).max()) <= 1e-6, alpha
    # the attention term is linear in alpha on real scores too
    qkv = make_qkv(B, grid, C, seed=3)
    table = make_table(full, heads, seed=4)
    one = run_step(qkv.cuda(), table.cuda(), r, B, grid, heads, full, (1, 1, 1), full, 1.0).double()
    half = run_step(qkv.cuda(), table.cuda(), r, B, grid, heads, full, (1, 1, 1), full, 0.5).double()
    assert float((half - (0.5 * one + 0.5 * r.double())).abs().max()) <= 1e-6 * float(one.max())


def test_window_rollout_step_deterministic_and_batch_invariant():
    B, grid, C, full, shift = 3, (4, 6, 6), 64, (2, 3, 3), (1, 1, 1)
    heads, n1 = C // 32, 4 * 6 * 6
    qkv = make_qkv(B, grid, C, seed=11)
    table = make_table(full, heads, seed=5).cuda()
    r = r_inputs(B * n1, seed=5)["random"]
    a = run_step(qkv.cuda(), table, r, B, grid, heads, full, shift, full, 0.5)
    b = run_step(qkv.cuda(), table, r, B, grid, heads, full, shift, full, 0.5)
    assert torch.equal(a, b)
    one = make_qkv(1, grid, C, seed=0)
    one[:n1] = qkv[n1:2 * n1]
    c = run_step(one.cuda(), table, r[n1:2 * n1].contiguous(), 1, grid, heads, full, shift, full, 0.5)
    assert torch.equal(a[n1:2 * n1], c)


# ------------------------------------------------------------------ 3. the hop
@pytest.mark.parametrize("grid", [(2, 6, 6), (2, 5, 7)])
def test_merge_rollout_spread(grid):
    B = 2
    T, H, W = grid
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    rp = torch.rand(B * T * H2 * W2, generator=torch.Generator().manual_seed(H)) + 0.05
    out = torch.full((B * T * H * W,), float("nan"), device="cuda")
    got = ops.merge_rollout_spread(rp.cuda(), B, grid, out).cpu()
    assert torch.equal(got, R.spread_ref(rp, B, grid))  # shares of 1, 1/2 and 1/4 are exact in fp32
    assert abs(float(got.double().sum()) - float(rp.double().sum())) <= 1e-6 * float(rp.double().sum())
    if H % 2 and W % 2:  # the corner parent has one child, which gets the whole share
        assert torch.equal(got.reshape(B, T, H, W)[:, :, H - 1, W - 1], rp.reshape(B, T, H2, W2)[:, :, H2 - 1, W2 - 1])
        assert torch.equal(got.reshape(B, T, H, W)[:, :, H - 1, 0] * 2, rp.reshape(B, T, H2, W2)[:, :, H2 - 1, 0])


# ------------------------------------------------------------------ 4. model against the oracle
def _model(cfg, sd=None, seed=0):
    from vclip_amd.swin3d import Swin3d
    m = Swin3d({k: v for k, v in cfg.items() if k != "num_classes"}, num_classes=cfg["num_classes"])
    m.load_state_dict(make_swin3d_weights(cfg, seed=seed) if sd is None else sd)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def sharp():
    sd = R.sharpen({k: torch.from_numpy(v) for k, v in make_swin3d_weights(R.TINY, seed=0).items()})
    return sd, _model(R.TINY, sd)


@pytest.mark.parametrize("T,HW", [(8, 48), (4, 48)])
def test_explain_matches_oracle_rollout(sharp, T, HW):
    sd, m = sharp
    video = torch.from_numpy(make_synthetic_video(2, T, HW, seed=3))
    with torch.no_grad():
        want_logits, grids, mats = R.oracle_probs(sd, R.TINY, video)
        _, _, mats16 = R.oracle_probs(sd, R.TINY, video, round_qk=True)
    ex = m.explain(video.cuda(), residual=0.5)
    B, (t0, h0, w0) = 2, grids[0]
    n0 = t0 * h0 * w0
    assert (t0, h0, w0) == (T // 2, HW // 4, HW // 4)
    assert tuple(ex.token_relevance.shape) == (B, n0) and tuple(ex.saliency.shape) == (B, t0, h0, w0)  # no CLS column
    assert tuple(ex.temporal.shape) == (B, t0) and tuple(ex.logits.shape) == (B, 2)
    assert all(x.dtype == torch.float32 for x in (ex.logits, ex.token_relevance, ex.saliency, ex.temporal))
    assert ex.logits.device.type == "cuda" and ex.token_relevance.device.type == "cpu"
    assert ex.method == "rollout" and ex.target is None
    assert float((ex.logits.cpu() - want_logits).abs().max()) < 1e-2
    assert torch.isfinite(ex.token_relevance).all() and (ex.saliency >= 0).all()
    assert ((ex.saliency.double().sum(dim=(1, 2, 3)) - 1).abs() < 1e-5).all()
    assert ((ex.token_relevance.double().sum(1) - 1).abs() < 1e-5).all()  # every step and hop conserves the sum
    assert torch.equal(ex.temporal, ex.saliency.sum(dim=(2, 3)))
    ref, ref16 = R.rollout_stepwise(mats, grids, 0.5), R.rollout_stepwise(mats16, grids, 0.5)
    sal = ex.saliency.reshape(B, n0)
    for b in range(B):
        yard, err = R.E(ref16[b], ref[b]), R.E(ex.token_relevance[b], ref[b])
        print(f"explain T = {T} clip {b}: bf16 q/k oracle yardstick {yard:.3e}, GPU {err:.3e}, ratio {err / yard:.2f}, "
              f"saliency {R.E(sal[b], ref[b]):.3e}")
        assert err <= R.MODEL_FACTOR * yard, (b, err, yard)
        assert R.E(sal[b], ref[b]) <= R.MODEL_FACTOR * yard, (b, yard)
    other = m.explain(video.cuda(), residual=0.25)
    assert float((other.saliency - ex.saliency).abs().max()) > 1e-4  # residual reaches the map


# ------------------------------------------------------------------ 5. refusals on the device, the forward untouched
def test_explain_refusals_and_forward_untouched():
    m = _model(R.TINY)
    video = torch.from_numpy(make_synthetic_video(2, 8, 48, seed=3)).cuda()
    m.graph_replay = True
    before = m(video).clone()
    assert torch.equal(m(video), before)
    captures, packed, bias = m._graphs.captures, m._packed, m._bias_cache
    ws = dict(m._ws)
    bias_items = dict(bias)
    m.explain(video)
    assert torch.equal(m(video), before)
    assert m._graphs.captures == captures  # explain invalidated nothing
    assert m._packed is packed and m._bias_cache is bias
    assert set(m._bias_cache) == set(bias_items) and all(m._bias_cache[k] is v for k, v in bias_items.items())
    assert set(m._ws) == set(ws) and all(m._ws[k] is v for k, v in ws.items())
    assert all(p.grad is None for p in m.parameters())
    m.graph_replay = False
    assert torch.equal(m(video), before)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.explain(video)
    m.eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain(video.cpu())
    for method in ("cls_attention", "grad_rollout"):
        with pytest.raises(ValueError, match="method"):
            m.explain(video, method=method)
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match="residual"):
            m.explain(video, residual=bad)
    with pytest.raises(ValueError, match=r"\[B, 3, T, H, W\]"):
        m.explain(video[:, :2].contiguous())
    with pytest.raises(ValueError, match=r"\[B, 3, T, H, W\]"):
        m.explain(video[0])
    with pytest.raises(ValueError, match="multiples of the patch size"):
        m.explain(video[:, :, :, :46].contiguous())
    with pytest.raises(ValueError, match="whole windows"):  # 40 / 4 = 10 rows: not whole windows of 3
        m.explain(video[:, :, :, :40, :40].contiguous())
    assert torch.equal(m(video), before)


# ------------------------------------------------------------------ 6. full size once
def test_explain_swin_t_full_size_memory():
    """Swin-T 32 x 224^2 at B = 1: 12 steps and 3 hops, finite, the sums hold; prints the call's peak extra device
    memory (the kept q|k|v of the 12 blocks is 165 MB; a stored heads x 392 x 392 matrix per window and block is
    never made)"""
    from vclip_amd.swin3d import create_model
    m = create_model(None, "tiny", num_classes=2, device="cuda").eval()
    video = torch.from_numpy(make_synthetic_video(1, 32, 224, seed=3)).cuda()
    m(video)  # the packed weights and the forward's workspace exist before the measurement
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ex = m.explain(video)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    kept = sum(q.numel() * 2 for q in m._explain_buffers(1, m.geometry(1, 32, 224, 224), video.device)["QKV"])
    print(f"explain Swin-T B = 1: kept q|k|v {kept / 1e6:.1f} MB, peak extra device memory {extra / 1e6:.1f} MB")
    assert tuple(ex.saliency.shape) == (1, 16, 56, 56) and tuple(ex.token_relevance.shape) == (1, 16 * 56 * 56)
    assert torch.isfinite(ex.token_relevance).all() and torch.isfinite(ex.logits).all()
    assert (ex.saliency >= 0).all()
    assert abs(float(ex.saliency.double().sum()) - 1) < 1e-5
    assert abs(float(ex.token_relevance.double().sum()) - 1) < 1e-5
    assert torch.equal(ex.temporal, ex.saliency.sum(dim=(2, 3)))
    assert np.isfinite(extra)
