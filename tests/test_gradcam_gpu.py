"""ResNet3D saliency on the GPU: the four kernels of csrc/cam.hip against the same formulas in fp64, and
ResNet3d.explain (Grad-CAM / HiResCAM at res5 and res4) against plain autograd on the fp32 oracle (tests/gradcam_ref.py).

Bounds (measured figures: DESIGN.md section 4):
  kernel  max|got - ref64| / max|ref64| <= 8 x the same formula in fp32 torch on the CPU (cast to the kernel's output
          format: bf16 for vc_cam_seed and vc_relu_bwd) against ref64, per shape and on identical inputs (the sibling
          kernels' bound).  Padding columns and the rows past B*T*H*W hold NaN: every output must be finite.
  model   E(x) = max|x - ref| / max|ref| of the GPU's signed map (token_relevance) against fp32 autograd, per clip, <=
          MODEL_FACTOR x E of the same autograd with every stored activation and conv weight rounded to bf16.  The
          factor is not derivable (the GPU also rounds the gradients to bf16 and folds BatchNorm before the cast): it
          is the smallest power of two at least twice the largest measured ratio, as test_window_rollout_gpu.py's.
          Measured E(gpu) / E(bf16 oracle) on the 32 (fixture, layer, method, target, clip) cases
          (gradcam_ref.MEASURED_RATIOS): 0.52 to 2.94, at yardsticks of 2.9e-3 to 5.2e-2 and E(gpu) of 5.0e-3 to 4.1e-2;
          twice the largest is 5.9, so MODEL_FACTOR = 8.  8 x the yardstick alone exceeds half of the smallest wrong-rule
          E in the sixteen res4 cases (tests/test_gradcam_cpu.py prints them: a dropped conv_b mask moves the map by
          0.05 to 0.3), so each case's bound is the smaller of the two (gradcam_ref.bound): every case of both targets is
          compared, none is left out, and no wrong rule of the CPU test is within the bound.
"""
import pytest
import torch

import gradcam_ref as R
from vclip_amd import ops
from vclip_amd.weights import make_resnet3d_weights, make_synthetic_video

pytestmark = pytest.mark.gpu
NAN16 = 0x7FC0  # a bf16 quiet NaN
SHAPES = [(2, (3, 5, 5), 64, 72), (1, (8, 7, 7), 2048, 2048)]  # B, grid, C, ld
POOLS = {(3, 5, 5): (2, 2, 2), (8, 7, 7): (4, 7, 7)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def bf16_rows(n, C, ld, seed, extra=8, scale=1.0):
    """bf16 [n + extra, ld]: N(0, scale) in [:n, :C], NaN in the padding columns and the rows past n"""
    x = (torch.randn(n + extra, ld, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.bfloat16)
    nan = torch.tensor(NAN16, dtype=torch.int16)
    x.view(torch.int16)[n:] = nan
    x.view(torch.int16)[:, C:] = nan
    return x


def f32_rows(n, C, ld, seed, extra=8):
    x = torch.randn(n + extra, ld, generator=torch.Generator().manual_seed(seed))
    x[n:] = float("nan")
    x[:, C:] = float("nan")
    return x


def nan_out(n, ld, extra=8):
    return torch.full((n + extra, ld), float("nan"), dtype=torch.bfloat16, device="cuda")


# ------------------------------------------------------------------ 1. kernels against fp64
@pytest.mark.parametrize("B,grid,C,ld", SHAPES)
def test_cam_seed_matches_fp64(B, grid, C, ld):
    pool = POOLS[grid]
    n = B * grid[0] * grid[1] * grid[2]
    wc = torch.randn(3, C, generator=torch.Generator().manual_seed(C))
    target = [2, 0][:B]
    rows = lambda t: t.permute(0, 2, 3, 4, 1).reshape(n, C)  # noqa: E731
    ref = rows(R.head_seed(wc, target, grid, pool))
    ref32 = rows(R.head_seed(wc, target, grid, pool, dtype=torch.float32)).bfloat16()
    out = nan_out(n, ld)
    ops.cam_seed(wc.cuda(), torch.tensor(target, dtype=torch.int32, device="cuda"), B, grid, C, pool, out)
    got = out.cpu()
    assert torch.isfinite(got[:n, :C]).all()
    assert torch.isnan(got[n:]).all() and torch.isnan(got[:, C:]).all()  # nothing written past the rows / columns
    yard, err = rel_err(ref32, ref), rel_err(got[:n, :C], ref)
    print(f"cam_seed {(B, grid, C, pool)}: fp32 formula (bf16 out) {yard:.3e}, bound {8 * yard:.3e}, kernel {err:.3e}")
    assert err <= 8 * yard
    # a pool covering the whole grid: the position-independent seed
    full = nan_out(n, ld)
    ops.cam_seed(wc.cuda(), torch.tensor(target, dtype=torch.int32, device="cuda"), B, grid, C, grid, full)
    f = full.cpu()[:n, :C].reshape(B, -1, C)
    assert torch.equal(f, f[:, :1].expand_as(f))
    with pytest.raises(RuntimeError, match="pool"):
        ops.cam_seed(wc.cuda(), torch.tensor(target, dtype=torch.int32, device="cuda"), B, grid, C,
                     (grid[0] + 1, 1, 1), out)


@pytest.mark.parametrize("B,grid,C,ld", SHAPES)
@pytest.mark.parametrize("d1_f32", [True, False])
def test_relu_bwd_matches_fp64(B, grid, C, ld, d1_f32):
    n = B * grid[0] * grid[1] * grid[2]
    y = bf16_rows(n, C, ld, seed=1)
    y[:n:3, :C:5] = 0  # exact zeros mask the gradient too (y > 0, not y >= 0)
    d1 = f32_rows(n, C, ld, seed=2) if d1_f32 else bf16_rows(n, C, ld, seed=2)
    d2s = {"none": None, "bf16": bf16_rows(n, C, ld, seed=3), "f32": f32_rows(n, C, ld, seed=4)}
    for with_y in (True, False):
        for name, d2 in d2s.items():
            s64 = d1[:n, :C].double() + (d2[:n, :C].double() if d2 is not None else 0)
            s32 = d1[:n, :C].float() + (d2[:n, :C].float() if d2 is not None else 0)
            keep = y[:n, :C].float() > 0 if with_y else torch.ones(n, C, dtype=torch.bool)
            ref, ref32 = s64 * keep, (s32 * keep).bfloat16()
            out = nan_out(n, ld)
            ops.relu_bwd(y.cuda() if with_y else None, d1.cuda(), n, C, out, d2.cuda() if d2 is not None else None)
            got = out.cpu()
            assert torch.isfinite(got[:n, :C]).all(), (with_y, name)
            assert torch.isnan(got[n:]).all() and torch.isnan(got[:, C:]).all()
            assert (got[:n, :C][~keep] == 0).all()
            yard, err = rel_err(ref32, ref), rel_err(got[:n, :C], ref)
            print(f"relu_bwd {(B, grid, C)} d1 {'f32' if d1_f32 else 'bf16'} d2 {name} y {with_y}: fp32 formula "
                  f"(bf16 out) {yard:.3e}, kernel {err:.3e}")
            assert err <= 8 * yard, (with_y, name)


@pytest.mark.parametrize("B,grid,C,ld", SHAPES)
def test_cam_weights_and_map_match_fp64(B, grid, C, ld):
    N = grid[0] * grid[1] * grid[2]
    n = B * N
    g, x = bf16_rows(n, C, ld, seed=5, scale=0.01), bf16_rows(n, C, ld, seed=6)
    gd, xd = g.cuda(), x.cuda()
    g64, x64 = g[:n, :C].double(), x[:n, :C].double()
    work = ops.cam_weights_work(B, C, "cuda").fill_(float("nan"))
    alpha = torch.full((B, C), float("nan"), device="cuda")
    ops.cam_weights(gd, B, N, C, work, alpha)
    a = alpha.cpu()
    assert torch.isfinite(a).all()
    ref = g64.reshape(B, N, C).mean(1)
    yard, err = rel_err(g[:n, :C].float().reshape(B, N, C).mean(1), ref), rel_err(a, ref)
    print(f"cam_weights {(B, grid, C)}: fp32 formula {yard:.3e}, bound {8 * yard:.3e}, kernel {err:.3e}")
    assert err <= 8 * yard
    for mode, w, ref, ref32 in (
            ("gradcam", alpha, (a.double().repeat_interleave(N, 0) * x64).sum(1),
             (a.repeat_interleave(N, 0) * x[:n, :C].float()).sum(1)),
            ("hirescam", gd, (g64 * x64).sum(1), (g[:n, :C].float() * x[:n, :C].float()).sum(1))):
        out = torch.full((n,), float("nan"), device="cuda")
        ops.cam_map(mode, xd, w, B, N, C, out)
        got = out.cpu()
        assert torch.isfinite(got).all(), mode
        yard, err = rel_err(ref32, ref), rel_err(got, ref)
        print(f"cam_map {mode} {(B, grid, C)}: fp32 formula {yard:.3e}, bound {8 * yard:.3e}, kernel {err:.3e}")
        assert err <= 8 * yard, mode
        assert (got < 0).any() and (got > 0).any()  # signed: no ReLU in the kernel


def test_cam_reductions_deterministic_and_batch_invariant():
    B, grid, C, ld = 2, (3, 5, 5), 64, 72
    N = grid[0] * grid[1] * grid[2]
    g, x = bf16_rows(B * N, C, ld, seed=7, scale=0.01), bf16_rows(B * N, C, ld, seed=8)

    def run(g, x, B):
        gd, xd = g.cuda(), x.cuda()
        alpha = torch.empty((B, C), device="cuda")
        ops.cam_weights(gd, B, N, C, ops.cam_weights_work(B, C, "cuda"), alpha)
        maps = [ops.cam_map(m, xd, w, B, N, C, torch.empty(B * N, device="cuda")).cpu()
                for m, w in (("gradcam", alpha), ("hirescam", gd))]
        return [alpha.cpu()] + maps

    one, two = run(g, x, B), run(g, x, B)
    assert all(torch.equal(p, q) for p, q in zip(one, two))
    solo = run(g[:N + 8].clone(), x[:N + 8].clone(), 1)  # clip 0 alone (its rows, then 8 rows of other data)
    assert torch.equal(solo[0][0], one[0][0])
    assert torch.equal(solo[1], one[1][:N]) and torch.equal(solo[2], one[2][:N])


# ------------------------------------------------------------------ 2. the model against autograd
@pytest.fixture(scope="module")
def small():
    from vclip_amd.resnet3d import ResNet3d
    sd = make_resnet3d_weights(R.SMALL, seed=0)
    m = ResNet3d(R.SMALL)
    m.load_state_dict(sd)
    return {k: torch.from_numpy(v) for k, v in sd.items()}, m.cuda().eval()


@pytest.fixture(scope="module")
def refs(small):
    """per (fixture, layer, target): the fp32 autograd maps and the same with bf16 storage, computed once"""
    sd, _ = small
    out = {}
    for fi, (B, T, HW, seed) in enumerate(R.FIXTURES):
        video = torch.from_numpy(make_synthetic_video(B, T, HW, seed=seed))
        for layer in R.LAYERS:
            for t in (0, 1):
                out[(fi, layer, t)] = (video, R.autograd_cam(sd, R.SMALL, video, layer, t),
                                       R.autograd_cam(sd, R.SMALL, video, layer, t, rounding=R.BF16))
    return out


def test_explain_matches_autograd(small, refs):
    sd, m = small
    bias = sd["blocks.5.proj.bias"]
    ratios, fails = [], []
    for fi, (B, T, HW, seed) in enumerate(R.FIXTURES):
        for layer in ("res5", "res4"):
            for method in R.METHODS:
                for t in (0, 1):
                    video, ref, ref16 = refs[(fi, layer, t)]
                    vd = video.cuda()
                    plain = m(vd)
                    ex = m.explain(vd, method=method, target=t, layer=layer)
                    grid = tuple(ref["A"].shape[2:])
                    n = grid[0] * grid[1] * grid[2]
                    assert tuple(ex.token_relevance.shape) == (B, n) and tuple(ex.saliency.shape) == (B,) + grid
                    assert tuple(ex.temporal.shape) == (B, T) and tuple(ex.logits.shape) == (B, 2)
                    assert all(x.dtype == torch.float32 for x in (ex.logits, ex.token_relevance, ex.saliency, ex.temporal))
                    assert ex.logits.device.type == "cuda" and ex.token_relevance.device.type == "cpu"
                    assert ex.method == method and ex.target == [t] * B
                    assert torch.equal(ex.logits, plain)  # bit for bit: the same launches on other buffers
                    assert torch.equal(m(vd), plain)      # and no workspace of the forward was disturbed
                    assert torch.isfinite(ex.token_relevance).all()
                    # saliency = relu(map) / its per-clip sum (0 when nothing is positive); temporal its spatial sum
                    pos = ex.token_relevance.double().clamp_min(0)
                    tot = pos.sum(1, keepdim=True)
                    want = torch.where(tot > 0, pos / tot.clamp_min(1e-300), torch.zeros_like(pos)).float()
                    assert torch.equal(ex.saliency.reshape(B, n), want) and (ex.saliency >= 0).all()
                    assert torch.equal(ex.temporal, ex.saliency.sum(dim=(2, 3)))
                    for b in range(B):
                        rmap = ref[method][b].reshape(n)
                        empty = not bool((rmap > 0).any())
                        s = float(ex.saliency[b].double().sum())
                        assert (s == 0.0) if empty else abs(s - 1) < 1e-5, (fi, layer, method, t, b, s, empty)
                        yard, err = R.E(ref16[method][b].reshape(n), rmap), R.E(ex.token_relevance[b], rmap)
                        ratios.append(round(err / yard, 2))
                        lim = R.bound((fi, layer, method, t, b), yard)
                        print(f"explain fixture {fi} {layer} {method} target {t} clip {b}: bf16 oracle yardstick {yard:.3e}, "
                              f"bound {lim:.3e}, GPU {err:.3e}, ratio {err / yard:.2f}, positive {int((rmap > 0).sum())}/{n}")
                        if not err <= lim:
                            fails.append((fi, layer, method, t, b, err, yard, lim))
                    if layer == "res5" and method == "hirescam":  # the head is linear in res5
                        total = ex.token_relevance.double().sum(1)
                        want_sum = (ex.logits[:, t].cpu() - bias[t]).double()
                        assert float(((total - want_sum).abs() / want_sum.abs()).max()) <= 1e-2
    print("measured ratios:", tuple(ratios), "largest", max(ratios))
    assert not fails, fails


def test_explain_targets(small, refs):
    _, m = small
    video = refs[(0, "res5", 0)][0].cuda()
    logits = m(video)
    auto = m.explain(video)  # gradcam at res5 for each clip's argmax
    assert auto.method == "gradcam" and auto.target == logits.argmax(1).tolist()
    mixed = m.explain(video, target=[1, 0])
    t0, t1 = m.explain(video, target=0), m.explain(video, target=torch.tensor([1, 1]))
    assert torch.equal(mixed.token_relevance[0], t1.token_relevance[0])
    assert torch.equal(mixed.token_relevance[1], t0.token_relevance[1])
    assert mixed.target == [1, 0] and t1.target == [1, 1]
    one = m.explain(video[:1].contiguous(), target=1)  # clip 0's map does not depend on B
    assert torch.equal(one.token_relevance[0], t1.token_relevance[0])


def test_explain_refusals_and_forward_untouched(small, refs):
    _, m = small
    video = refs[(0, "res5", 0)][0].cuda()
    m.graph_replay = True
    before = m(video).clone()
    assert torch.equal(m(video), before)
    captures, packed, ws = m._graphs.captures, m._packed, dict(m._ws)
    m.explain(video, method="hirescam", layer="res4")
    assert torch.equal(m(video), before)
    assert m._graphs.captures == captures and m._packed is packed  # explain invalidated nothing
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
    for method in ("rollout", "grad_rollout", "cam"):
        with pytest.raises(ValueError, match="method"):
            m.explain(video, method=method)
    for layer in ("res2", "res3", "stem"):
        with pytest.raises(ValueError, match="layer"):
            m.explain(video, layer=layer)
    for bad in (2, -1, [0], [0, 1, 0], 0.5, True, torch.tensor([0.0, 1.0]), "referral"):
        with pytest.raises(ValueError, match="target"):
            m.explain(video, target=bad)
    with pytest.raises(ValueError, match=r"\[B, 3, T, H, W\]"):
        m.explain(video[:, :2].contiguous())
    with pytest.raises(ValueError, match=r"\[B, 3, T, H, W\]"):
        m.explain(video[0])
    with pytest.raises(ValueError, match="head pool"):  # 32 x 32 frames end on a 1 x 1 map: the (2, 2, 2) pool does not fit
        m.explain(video[:, :, :, :32, :32].contiguous())
    assert torch.equal(m(video), before)
