"""ResNet50-LSTM saliency on the GPU: the two kernels of csrc/frame_cam.hip against the same formulas in fp64, and
VideoResNet50LSTM.explain / explain_stream_begin against plain autograd on the fp32 reference (tests/lstm_cam_ref.py).

Bounds (measured figures: DESIGN.md section 4):
  kernel  max|got - ref64| / max|ref64| <= 8 x the same formula in fp32 torch on the CPU (cast to bf16 for
          vc_frame_avgpool_bwd) against ref64, per shape and on identical inputs (the sibling kernels' bound in
          test_gradcam_gpu.py).  Padding columns and the rows past N*P hold NaN; outputs are pre-filled with NaN and
          over-allocated: exactly the N*P and N entries, or the [N*P, C] block, are written and finite.
  model   E(x) = max|x - ref| / max|ref| of the signed map (token_relevance) and of frame_relevance against fp32 autograd,
          per video, <= MODEL_FACTOR x E of the same autograd with every stored activation, conv weight, pooled feature
          and inter-layer h rounded to bf16.  The factor is not derivable (the GPU also folds BatchNorm before the cast,
          rounds W_ih and dpre to bf16 for the MFMA GEMMs and, at res4, the chain's gradients): it is the smallest power
          of two at least twice the largest measured ratio, as test_gradcam_gpu.py's.  Measured E(gpu) / E(bf16
          reference) on the 160 comparisons (lstm_cam_ref.MEASURED_RATIOS): 0.01 to 4.43 for frame_relevance, 0.30 to 3.37
          at res5, 0.39 to 1.76 at res4, at yardsticks of 1.3e-2 to 2.3e-1; twice the largest is 8.9, so MODEL_FACTOR = 16.
          Each case's bound is capped at half its smallest wrong-rule E of tests/test_lstm_cam_cpu.py
          (lstm_cam_ref.bound); every (fixture, layer, method, target, video) is compared, none is left out.
          Target 0's reference is minus target 1's: test_lstm_cam_cpu.py shows autograd agrees to 1e-6.
"""
import pytest
import torch

import lstm_cam_ref as R
from vclip_amd import ops

pytestmark = pytest.mark.gpu
NAN16 = 0x7FC0  # a bf16 quiet NaN
SHAPES = [(3, 4, 64, 72), (2, 49, 2048, 2048), (5, 1, 2048, 2048)]  # N, P, C, ld
EXTRA = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def bf16_rows(n, C, ld, seed):
    """bf16 [n + EXTRA, ld]: N(0, 1) in [:n, :C], NaN in the padding columns and the rows past n"""
    x = torch.randn(n + EXTRA, ld, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)
    nan = torch.tensor(NAN16, dtype=torch.int16)
    x.view(torch.int16)[n:] = nan
    x.view(torch.int16)[:, C:] = nan
    return x


def f32_rows(n, C, ld, seed, scale=0.01):
    x = torch.randn(n + EXTRA, ld, generator=torch.Generator().manual_seed(seed)) * scale
    x[n:] = float("nan")
    x[:, C:] = float("nan")
    return x


def run_frame_cam(x, g, N, P, C):
    """(map [N*P + EXTRA], frame_rel [N + EXTRA]) on the host: the kernel writes the leading N*P / N entries of NaN buffers"""
    m = torch.full((N * P + EXTRA,), float("nan"), device="cuda")
    fr = torch.full((N + EXTRA,), float("nan"), device="cuda")
    ops.frame_cam(x.cuda(), g.cuda(), N, P, C, m[: N * P], fr[:N])
    return m.cpu(), fr.cpu()


# ------------------------------------------------------------------ 1. kernels against fp64
@pytest.mark.parametrize("N,P,C,ld", SHAPES)
def test_frame_cam_matches_fp64(N, P, C, ld):
    n = N * P
    x, g = bf16_rows(n, C, ld, seed=1), f32_rows(N, C, ld + 8, seed=2)  # g: ldg > C
    m, fr = run_frame_cam(x, g, N, P, C)
    assert torch.isfinite(m[:n]).all() and torch.isfinite(fr[:N]).all()
    assert torch.isnan(m[n:]).all() and torch.isnan(fr[N:]).all()  # nothing written past the N*P / N entries
    x64, g64 = x[:n, :C].double().reshape(N, P, C), g[:N, :C].double()
    ref = (g64[:, None] * x64).sum(-1) / P
    x32, g32 = x[:n, :C].float().reshape(N, P, C), g[:N, :C]
    ref32 = (g32[:, None] * x32).sum(-1) / P
    for what, got, r64, r32 in (("map", m[:n].reshape(N, P), ref, ref32), ("frame_rel", fr[:N], ref.sum(1), ref32.sum(1))):
        yard, err = rel_err(r32, r64), rel_err(got, r64)
        print(f"frame_cam {what} {(N, P, C, ld)}: fp32 formula {yard:.3e}, bound {8 * yard:.3e}, kernel {err:.3e}")
        assert err <= 8 * yard, what
    assert (m[:n] < 0).any() and (m[:n] > 0).any()  # signed: no ReLU in the kernel
    if P == 1:  # gradient x input on pooled features: one entry per frame, the frame sum is the entry
        assert torch.equal(m[:n], fr[:N])
    m2, fr2 = run_frame_cam(x, g, N, P, C)  # fixed summation order: two runs are equal
    assert torch.equal(m2[:n], m[:n]) and torch.equal(fr2[:N], fr[:N])
    # frame 0 alone (its rows, then rows of other data) equals frame 0 within the batch
    m1, fr1 = run_frame_cam(x[: P + EXTRA].clone(), g[: 1 + EXTRA].clone(), 1, P, C)
    assert torch.equal(m1[:P], m[:P]) and torch.equal(fr1[:1], fr[:1])


@pytest.mark.parametrize("N,P,C,ld", SHAPES)
def test_frame_avgpool_bwd_matches_fp64(N, P, C, ld):
    n = N * P
    g = f32_rows(N, C, ld + 8, seed=3)

    def run(g, N):
        out = torch.full((N * P + EXTRA, ld), float("nan"), dtype=torch.bfloat16, device="cuda")
        ops.frame_avgpool_bwd(g.cuda(), N, P, C, out)
        return out.cpu()

    got = run(g, N)
    assert torch.isfinite(got[:n, :C]).all()
    assert torch.isnan(got[n:]).all() and torch.isnan(got[:, C:]).all()  # exactly the [N*P, C] block is written
    ref = (g[:N, :C].double() / P).repeat_interleave(P, 0)
    ref32 = (g[:N, :C] / P).bfloat16().repeat_interleave(P, 0)
    yard, err = rel_err(ref32, ref), rel_err(got[:n, :C], ref)
    print(f"frame_avgpool_bwd {(N, P, C, ld)}: fp32 formula (bf16 out) {yard:.3e}, bound {8 * yard:.3e}, kernel {err:.3e}")
    assert err <= 8 * yard
    assert torch.equal(run(g, N)[:n, :C], got[:n, :C])
    assert torch.equal(run(g[: 1 + EXTRA].clone(), 1)[:P, :C], got[:P, :C])


def test_kernel_wrappers_refuse_bad_arguments():
    x, g = bf16_rows(8, 64, 64, seed=4).cuda(), f32_rows(2, 64, 64, seed=5).cuda()
    m, fr = torch.empty(8, device="cuda"), torch.empty(2, device="cuda")
    from vclip_amd._lib import VclipError
    for args in ((x, g, 2, 4, 60, m, fr), (x, g, 2, 16, 64, torch.empty(32, device="cuda"), fr), (x, g, 2, 4, 64, m[:7], fr),
                 (x, g.bfloat16(), 2, 4, 64, m, fr), (x, g, 2, 4, 64, m, torch.empty(3, device="cuda")),
                 (x.cpu(), g, 2, 4, 64, m, fr), (x, g, 2, 0, 64, m, fr)):
        with pytest.raises(VclipError):
            ops.frame_cam(*args)
    out = torch.empty(8, 64, dtype=torch.bfloat16, device="cuda")
    for args in ((g, 2, 4, 60, out), (g, 2, 8, 64, out), (g, 2, 4, 64, out.float()), (g.cpu(), 2, 4, 64, out), (g, 0, 4, 64, out)):
        with pytest.raises(VclipError):
            ops.frame_avgpool_bwd(*args)


# ------------------------------------------------------------------ 2. the model against autograd
@pytest.fixture(scope="module")
def model():
    from vclip_amd.resnet50_lstm import VideoResNet50LSTM
    m = VideoResNet50LSTM(R.HIDDEN, R.LAYERS_LSTM, 0.5)
    m.load_state_dict(R.weights())
    return m.cuda().eval()


@pytest.fixture(scope="module")
def refs():
    """per fixture: (video, lengths, [per video (fp32 autograd for target 1, the same with bf16 storage)]), computed once"""
    p = R.weights()
    out = {}
    for name in R.FIXTURES:
        video, lengths, vids = R.fixture_video(name)
        out[name] = (video, lengths, [(R.autograd_cam(p, fr, 1), R.autograd_cam(p, fr, 1, rounding=R.BF16)) for fr in vids])
    return out


def host_saliency(rel, shape):
    pos = rel.double().clamp_min(0)
    tot = pos.sum()
    return (pos / tot if float(tot) > 0 else torch.zeros_like(pos)).float().reshape(shape)


def test_explain_matches_autograd(model, refs):
    ratios, fails = {}, []
    for name, (video, lengths, vids) in refs.items():
        vd = video.cuda()
        nseq = len(vids)
        plain = (model(vd) if lengths is None else model.forward_ragged(vd, lengths)).clone()
        ws, packed = model._ws, model.backbone._packed
        got = {}
        for layer in R.LAYERS:
            for method in R.METHODS:
                for t in (0, 1):
                    ex = model.explain(vd, method=method, target=t, layer=layer, lengths=lengths)
                    got[(layer, method, t)] = ex
                    hl = 2 if layer == "res5" else 4
                    assert ex.logits.dtype == torch.float32 and ex.logits.device.type == "cuda"
                    assert tuple(ex.logits.shape) == (nseq, 1) and torch.equal(ex.logits, plain)  # bit for bit
                    assert ex.method == method and ex.target == [t] * nseq
                    if lengths is None:
                        T = video.shape[2]
                        assert tuple(ex.token_relevance.shape) == (nseq, T * hl * hl)
                        assert tuple(ex.saliency.shape) == (nseq, T, hl, hl) and tuple(ex.temporal.shape) == (nseq, T)
                        assert tuple(ex.frame_relevance.shape) == (nseq, T)
                    else:
                        for what in ("token_relevance", "saliency", "temporal", "frame_relevance"):
                            assert isinstance(getattr(ex, what), list) and len(getattr(ex, what)) == nseq, what
                    for b in range(nseq):
                        n = vids[b][0]["g"].shape[0]
                        # video b's entry, of a dense [B, ...] tensor or of a ragged list
                        rel, sal, tem, frel = ex.token_relevance[b], ex.saliency[b], ex.temporal[b], ex.frame_relevance[b]
                        for x, shape in ((rel, (n * hl * hl,)), (sal, (n, hl, hl)), (tem, (n,)), (frel, (n,))):
                            assert x.dtype == torch.float32 and x.device.type == "cpu" and tuple(x.shape) == shape
                            assert torch.isfinite(x).all()
                        # saliency = relu(map) / its per-video sum (0 when nothing is positive); temporal its spatial sum
                        assert torch.equal(sal, host_saliency(rel, (n, hl, hl))) and (sal >= 0).all()
                        assert torch.equal(tem, sal.sum(dim=(1, 2)))
                        ref, ref16 = vids[b]
                        s = 1.0 if t else -1.0
                        for q, x in (((layer, method), rel), ("frame", frel)):
                            r, r16 = s * ref[q].reshape(-1), s * ref16[q].reshape(-1)
                            yard, err = R.E(r16, r), R.E(x, r)
                            lim = R.bound((name, b, q), yard)
                            ratios.setdefault(q, []).append(round(err / yard, 2))
                            print(f"explain {name} video {b} {layer} {method} target {t} {q}: bf16 yardstick {yard:.3e}, bound "
                                  f"{lim:.3e}, GPU {err:.3e}, ratio {err / yard:.2f}, positive {int((r > 0).sum())}/{r.numel()}")
                            if not err <= lim:
                                fails.append((name, b, layer, method, t, q, err, yard, lim))
        # exact properties
        for layer in R.LAYERS:
            for method in R.METHODS:
                e0, e1 = got[(layer, method, 0)], got[(layer, method, 1)]
                for b in range(nseq):  # every step is linear in the seed's sign and no mask depends on it
                    assert torch.equal(e0.token_relevance[b], -e1.token_relevance[b]), (name, layer, method, b)
                    assert torch.equal(e0.frame_relevance[b], -e1.frame_relevance[b])
        for t in (0, 1):  # at res5 both methods run the same launches
            a, h = got[("res5", "gradcam", t)], got[("res5", "hirescam", t)]
            assert all(torch.equal(a.token_relevance[b], h.token_relevance[b]) for b in range(nseq))
        # nothing of the forward was disturbed
        again = model(vd) if lengths is None else model.forward_ragged(vd, lengths)
        assert torch.equal(again, plain)
        assert model._ws is ws and model.backbone._packed is packed
        assert all(p.grad is None for p in model.parameters())
    for q, v in ratios.items():
        print(f"measured ratios {q}: smallest {min(v)}, largest {max(v)}")
    assert not fails, fails


def test_explain_targets_and_batch_invariance(model, refs):
    video, lengths, _ = refs["ragged3"]
    vd = video.cuda()
    logits = model.forward_ragged(vd, lengths)
    auto = model.explain(vd, lengths=lengths)  # gradcam at res5 for each video's predicted class
    assert auto.method == "gradcam" and auto.target == [int(v >= 0) for v in logits[:, 0].tolist()]
    mixed = model.explain(vd, target=[1, 0, 1], lengths=lengths)
    t0, t1 = model.explain(vd, target=0, lengths=lengths), model.explain(vd, target=torch.tensor([1, 1, 1]), lengths=lengths)
    assert mixed.target == [1, 0, 1] and t1.target == [1, 1, 1]
    for b, src in enumerate((t1, t0, t1)):
        assert torch.equal(mixed.token_relevance[b], src.token_relevance[b])
        assert torch.equal(mixed.frame_relevance[b], src.frame_relevance[b])
    # a video explained alone equals the same video inside a ragged batch, at both layers
    for layer, method in (("res5", "gradcam"), ("res4", "gradcam"), ("res4", "hirescam")):
        batch = model.explain(vd, method=method, target=1, layer=layer, lengths=lengths)
        r0 = 0
        for b, n in enumerate(lengths):
            one = model.explain(vd[:, :, r0: r0 + n].contiguous(), method=method, target=1, layer=layer, lengths=(n,))
            assert torch.equal(one.logits[0], batch.logits[b])
            assert torch.equal(one.token_relevance[0], batch.token_relevance[b]), (layer, method, b)
            assert torch.equal(one.frame_relevance[0], batch.frame_relevance[b])
            r0 += n
    # the dense layout is the ragged one with equal lengths
    dv, _, _ = refs["dense"]
    dd = dv.cuda()
    dense = model.explain(dd, method="hirescam", target=1, layer="res4")
    flat = dd.permute(1, 0, 2, 3, 4).reshape(3, 1, -1, R.HW, R.HW).permute(1, 0, 2, 3, 4).contiguous()
    rag = model.explain(flat, method="hirescam", target=1, layer="res4", lengths=(dv.shape[2],) * dv.shape[0])
    for b in range(dv.shape[0]):
        assert torch.equal(dense.token_relevance[b], rag.token_relevance[b])
        assert torch.equal(dense.frame_relevance[b], rag.frame_relevance[b])


def test_explain_refusals(model, refs):
    video, lengths, _ = refs["ragged3"]
    vd = video.cuda()
    dense = refs["dense"][0].cuda()
    before = model.forward_ragged(vd, lengths).clone()
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.explain(dense)
    with pytest.raises(RuntimeError, match="eval"):
        model.explain_stream_begin(2)
    model.eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        model.explain(dense.cpu())
    for method in ("rollout", "grad_rollout", "cam"):
        with pytest.raises(ValueError, match="method"):
            model.explain(dense, method=method)
    for layer in ("res2", "res3", "stem"):
        with pytest.raises(ValueError, match="layer"):
            model.explain(dense, layer=layer)
    for bad in (2, -1, [0], [0, 1, 0], 0.5, True, torch.tensor([0.0, 1.0]), "referral"):
        with pytest.raises(ValueError, match="target"):
            model.explain(dense, target=bad)
    with pytest.raises(ValueError, match="target"):
        model.explain(vd, target=[0, 1], lengths=lengths)
    with pytest.raises(ValueError, match=r"\[B, 3, T, H, W\]"):
        model.explain(dense[:, :2].contiguous())
    with pytest.raises(ValueError, match=r"\[B, 3, T, H, W\]"):
        model.explain(dense[0])
    for bad in ((3, 1, 5), (3, 0, 7), (), (3, 1, 6, 1)):
        with pytest.raises(ValueError, match="lengths"):
            model.explain(vd, lengths=bad)
    with pytest.raises(ValueError, match=r"\[1, 3, N, H, W\]"):
        model.explain(dense, lengths=(5, 5))
    with pytest.raises(ValueError, match="B must be"):
        model.explain_stream_begin(0)
    assert torch.equal(model.forward_ragged(vd, lengths), before)


# ------------------------------------------------------------------ 3. whole recordings
SESSION_LENGTHS = (7, 3)
SESSION_CHUNK = 3


def test_explain_session(model):
    from vclip_amd.weights import make_synthetic_video
    recs = [torch.from_numpy(make_synthetic_video(1, n, R.HW, seed=21 + i)).cuda() for i, n in enumerate(SESSION_LENGTHS)]
    rounds, pos = [], [0, 0]
    while any(p < n for p, n in zip(pos, SESSION_LENGTHS)):
        lens = [min(SESSION_CHUNK, n - p) for p, n in zip(pos, SESSION_LENGTHS)]
        rounds.append((torch.cat([r[:, :, p: p + k] for r, p, k in zip(recs, pos, lens) if k], dim=2), lens))
        pos = [p + k for p, k in zip(pos, lens)]
    assert [lens for _, lens in rounds] == [[3, 3], [3, 0], [1, 0]]
    whole = torch.cat(recs, dim=2)

    def run(target):
        sess, state = model.explain_stream_begin(2), None
        for clip, lens in rounds:
            want_logits, state, want_frames = model.forward_stream(clip, lens, state, frame_logits=True)
            logits, frames = sess.push(clip, lens)
            assert torch.equal(logits, want_logits) and torch.equal(frames, want_frames)  # exactly forward_stream's
        return sess, sess.finish(target=target), want_logits

    for target in (1, 0, None, [0, 1]):
        sess, ex, last = run(target)
        ref = model.explain(whole, target=target, layer="res5", lengths=SESSION_LENGTHS)
        assert ex.target == ref.target and (target is None or ex.target == ([target] * 2 if isinstance(target, int) else target))
        assert torch.equal(ex.logits, last) and ex.logits.device.type == "cuda" and tuple(ex.logits.shape) == (2, 1)
        assert ex.token_relevance is None and ex.saliency is None
        assert isinstance(ex.frame_relevance, list) and len(ex.frame_relevance) == 2
        for b, n in enumerate(SESSION_LENGTHS):
            fr, tem = ex.frame_relevance[b], ex.temporal[b]
            assert fr.dtype == torch.float32 and fr.device.type == "cpu" and tuple(fr.shape) == (n,) == tuple(tem.shape)
            print(f"session target {target} recording {b}: chunked {fr.tolist()} whole {ref.frame_relevance[b].tolist()}")
            assert torch.equal(fr, ref.frame_relevance[b]), (target, b)  # chunked == whole, bit for bit
            assert torch.equal(tem, host_saliency(fr, (n,)))
            s = float(tem.double().sum())
            assert abs(s - 1) < 1e-5 if bool((fr > 0).any()) else s == 0.0
        with pytest.raises(RuntimeError, match="finish"):
            sess.finish()
        with pytest.raises(RuntimeError, match="finish"):
            sess.push(*rounds[0])
    with pytest.raises(ValueError, match="target"):
        run([1])
    with pytest.raises(ValueError, match="target"):
        run(2)
    sess = model.explain_stream_begin(2)
    with pytest.raises(RuntimeError, match="before any push"):
        sess.finish()
    with pytest.raises(ValueError, match="recordings"):
        sess.push(rounds[0][0], [3, 2, 1])
    assert all(p.grad is None for p in model.parameters())
