"""The saliency faithfulness test on the GPU: the two kernels of csrc/perturb.hip against tests/faithfulness_ref.py, and
perturbation_curve / faithfulness on one tiny model per family (the seeded synthetic weights and shapes of the families'
own GPU tests) against the same model run on clips masked by the CPU reference.

Bounds:
  vc_perturb_clips         torch.equal to the indexing reference: the kernel is a pure select.
  vc_gaussian_blur_planes  max|out - ref64| / max|ref64| <= 8 x the same reference in fp32 torch on the CPU against
                           ref64, per shape, all three on the same inputs and the same f32 taps (the sibling kernels'
                           bound, test_grad_rollout_gpu.py); a constant plane within 1 ulp.
  curves                   every step's logits within 1e-2 of the model on the reference's masked clip (the project's
                           model bound: equality is not promised, the GEMM tile pick depends on the row count).

No test here asserts that a map is GOOD (deletion_gain > 0, a falling deletion curve): the weights are synthetic and
untrained, so that would be a property of the seed, not of the code.  What is pinned is that the curve is the model's
score on exactly the clips the protocol defines.
"""
import json
import os

import numpy as np
import pytest
import torch

import faithfulness_ref as R
from vclip_amd import ops

pytestmark = pytest.mark.gpu
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_TOL = 1e-2
STEPS = 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# ------------------------------------------------------------------ 1. vc_perturb_clips
PERTURB_SHAPES = [(1, 3, 2, 8, 8, (1, 2, 2)), (2, 3, 8, 64, 64, (4, 4, 4)), (1, 3, 4, 50, 70, (4, 2, 3)),
                  (2, 3, 4, 32, 32, (2, 8, 8)), (1, 1, 3, 7, 5, (3, 7, 5))]  # B, C, T, H, W, grid


def perturb_inputs(B, C, T, H, W, grid, layout):
    g = torch.Generator().manual_seed(B * 1000 + H)
    shape = (B, T, C, H, W) if layout == "btchw" else (B, C, T, H, W)
    clip, base = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    clip.view(-1)[::7] = -0.0  # the select copies bits: signed zeros and NaN payloads survive
    clip.view(-1)[3::11] = float("nan")
    rank = R.ranks_of(torch.rand((B,) + grid, generator=g))  # a random map: ragged masked sets
    return clip, base, rank


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("B,C,T,H,W,grid", PERTURB_SHAPES)
def test_perturb_clips_equals_indexing(B, C, T, H, W, grid, layout):
    clip, base, rank = perturb_inputs(B, C, T, H, W, grid, layout)
    N = grid[0] * grid[1] * grid[2]
    cd, bd, rd = clip.cuda(), base.cuda(), rank.cuda()
    for ks in ([N // 2], R.step_counts(N, 10), [0], [N]):  # F = 1 and 11, nothing and everything touched
        kd = torch.tensor(ks, dtype=torch.int32, device="cuda")
        for mode in ("deletion", "insertion"):
            for b_host, b_dev in ((None, None), (base, bd)):
                got = ops.perturb_clips(cd, rd, kd, grid, layout, mode, base=b_dev).cpu()
                assert tuple(got.shape) == (len(ks),) + tuple(clip.shape)
                assert same_bits(got, R.perturb(clip, b_host, rank, ks, grid, layout, mode)), (ks, mode, b_host is None)
                if ks in ([0], [N]):
                    whole = (ks == [0]) == (mode == "deletion")  # the clip itself, or the base alone
                    want = clip if whole else (torch.zeros_like(clip) if b_host is None else base)
                    assert same_bits(got[0], want)
    assert same_bits(cd.cpu(), clip) and same_bits(bd.cpu(), base) and torch.equal(rd.cpu(), rank)  # inputs untouched


def test_perturb_clips_unaligned_pointers_take_the_scalar_path():
    B, C, T, H, W, grid = PERTURB_SHAPES[2]
    clip, base, rank = perturb_inputs(B, C, T, H, W, grid, "bcthw")
    n = clip.numel()
    cd = torch.empty(n + 1, device="cuda")[1:].view(clip.shape).copy_(clip)  # 4 bytes past a 16-byte boundary
    od = torch.empty(3 * n + 3, device="cuda")[3:].view((3,) + tuple(clip.shape))
    ks = [0, 7, 24]
    kd = torch.tensor(ks, dtype=torch.int32, device="cuda")
    got = ops.perturb_clips(cd, rank.cuda(), kd, grid, "bcthw", "deletion", base=base.cuda(), out=od)
    assert got.data_ptr() % 16 != 0 and cd.data_ptr() % 16 != 0
    assert same_bits(got.cpu(), R.perturb(clip, base, rank, ks, grid, "bcthw", "deletion"))


def test_perturb_clips_op_refusals():
    from vclip_amd._lib import VclipError
    clip = torch.zeros(1, 3, 4, 8, 8, device="cuda")
    rank = torch.zeros(1, 8, dtype=torch.int32, device="cuda")
    k = torch.tensor([0, 8], dtype=torch.int32, device="cuda")
    ok = dict(clip=clip, rank=rank, k=k, grid=(2, 2, 2), layout="bcthw", mode="deletion")
    ops.perturb_clips(**ok)
    for kw in (dict(layout="bthwc"), dict(mode="blur"), dict(grid=(5, 2, 2)), dict(grid=(2, 2)), dict(clip=clip.double()),
               dict(clip=clip[:, :, :, :, ::2]), dict(rank=rank.long()), dict(rank=rank[:, :7]), dict(k=k.long()),
               dict(base=clip[0]), dict(out=torch.empty(1, 1, 3, 4, 8, 8, device="cuda")), dict(k=k.cpu())):
        with pytest.raises(VclipError):
            ops.perturb_clips(**dict(ok, **kw))


# ------------------------------------------------------------------ 2. vc_gaussian_blur_planes
BLUR_SHAPES = [(3, 5, 7), (6, 64, 64), (1, 33, 130), (2, 224, 224)]  # planes, H, W


@pytest.mark.parametrize("planes,H,W", BLUR_SHAPES)
def test_gaussian_blur_matches_fp64(planes, H, W):
    x = torch.randn(planes, H, W, generator=torch.Generator().manual_seed(W))
    for ksize, sigma in ((11, 5.0), (31, 2.5), (1, 1.0)):
        w = ops.gaussian_taps(ksize, sigma)
        assert torch.equal(w, R.taps(ksize, sigma))
        ref, ref32 = R.blur(x, w, torch.float64), R.blur(x, w, torch.float32)
        xd = x.cuda()
        got = ops.gaussian_blur_planes(xd, ksize, sigma).cpu()
        assert torch.equal(xd.cpu(), x) and torch.isfinite(got).all()
        yard, err = rel_err(ref32, ref), rel_err(got, ref)
        print(f"blur {(planes, H, W)} ksize {ksize} sigma {sigma}: fp32 reference {yard:.3e}, bound {8 * yard:.3e}, kernel {err:.3e}")
        assert err <= 8 * yard


def test_gaussian_blur_constant_deterministic_and_batch_invariant():
    for c in (1.0, 0.3, -2.5, 1e-3):
        x = torch.full((2, 40, 70), c, device="cuda")
        got = ops.gaussian_blur_planes(x).cpu()
        ulp = float(np.spacing(np.float32(abs(c))))
        assert float((got.double() - float(np.float32(c))).abs().max()) <= ulp, c
    x = torch.randn(6, 64, 100, generator=torch.Generator().manual_seed(0)).cuda()
    one, two = ops.gaussian_blur_planes(x), ops.gaussian_blur_planes(x)
    assert torch.equal(one, two)
    assert torch.equal(ops.gaussian_blur_planes(x[:1].clone())[0], one[0])  # plane 0 blurred alone
    five = ops.gaussian_blur_planes(x.reshape(1, 2, 3, 64, 100))            # any leading dimensions: the same planes
    assert tuple(five.shape) == (1, 2, 3, 64, 100) and torch.equal(five.reshape(6, 64, 100), one)


def test_gaussian_blur_op_refusals():
    from vclip_amd._lib import VclipError
    x = torch.zeros(2, 8, 8, device="cuda")
    for kw in (dict(ksize=10), dict(ksize=33), dict(ksize=0), dict(sigma=0.0), dict(sigma=-1.0), dict(out=x),
               dict(work=x), dict(out=torch.empty(2, 8, 9, device="cuda")), dict(work=torch.empty(100, device="cuda"))):
        with pytest.raises(VclipError):
            ops.gaussian_blur_planes(x, **kw)
    for bad in (x.double(), x[:, :, ::2], x[0, 0]):
        with pytest.raises(VclipError):
            ops.gaussian_blur_planes(bad)


# ------------------------------------------------------------------ 3. one tiny model per family
def _vivit():
    from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
    from vclip_amd.weights import make_vivit_weights
    g = np.load(os.path.join(GD, "vivit_tiny.npz"))
    cfg = json.loads(str(g["config"]))
    m = VivitForVideoClassification(VivitConfig(**cfg, id2label={0: "non-referral", 1: "referral"}))
    m.load_state_dict(make_vivit_weights(cfg, seed=0))
    return m, torch.from_numpy(g["pixel_values"])[:2].contiguous(), dict(method="rollout")


def _timesformer():
    from vclip_amd.timesformer import TimesformerConfig, TimesformerForVideoClassification
    from vclip_amd.weights import make_timesformer_weights
    g = np.load(os.path.join(GD, "timesformer_tiny.npz"))
    cfg = json.loads(str(g["config"]))
    m = TimesformerForVideoClassification(TimesformerConfig(**cfg, id2label={0: "non-referral", 1: "referral"}))
    m.load_state_dict(make_timesformer_weights(cfg, seed=0))
    return m, torch.from_numpy(g["pixel_values"])[:2].contiguous(), dict(method="cls_attention")


def _swin():
    import window_rollout_ref as WR
    from vclip_amd.swin3d import Swin3d
    from vclip_amd.weights import make_swin3d_weights, make_synthetic_video
    m = Swin3d({k: v for k, v in WR.TINY.items() if k != "num_classes"}, num_classes=WR.TINY["num_classes"])
    m.load_state_dict(make_swin3d_weights(WR.TINY, seed=0))
    return m, torch.from_numpy(make_synthetic_video(2, 4, 48, seed=3)), {}


def _resnet3d():
    import gradcam_ref as GR
    from vclip_amd.resnet3d import ResNet3d
    from vclip_amd.weights import make_resnet3d_weights, make_synthetic_video
    m = ResNet3d(GR.SMALL)
    m.load_state_dict(make_resnet3d_weights(GR.SMALL, seed=0))
    B, T, HW, seed = GR.FIXTURES[0]
    return m, torch.from_numpy(make_synthetic_video(B, T, HW, seed=seed)), dict(method="hirescam", layer="res4")


def _lstm():
    import lstm_cam_ref as LR
    from vclip_amd.resnet50_lstm import VideoResNet50LSTM
    m = VideoResNet50LSTM(LR.HIDDEN, LR.LAYERS_LSTM, 0.5)
    m.load_state_dict(LR.weights())
    return m, LR.fixture_video("dense")[0], dict(method="gradcam", layer="res4")


FAMILIES = {"vivit": _vivit, "timesformer": _timesformer, "swin": _swin, "resnet3d": _resnet3d, "lstm": _lstm}


@pytest.fixture(scope="module", params=sorted(FAMILIES))
def case(request):
    """(family, model, clip on the host, clip on the GPU, layout, the Explanation, its grid and reference ranks), once"""
    fam = request.param
    m, clip, how = FAMILIES[fam]()
    m = m.cuda().eval()
    layout = "btchw" if fam in ("vivit", "timesformer") else "bcthw"
    cd = clip.cuda()
    ex = m.explain(cd, **how)
    return fam, m, clip, cd, layout, ex, tuple(ex.saliency.shape[1:]), R.ranks_of(ex.saliency)


def logits_of(fam, m, x):
    out = m(pixel_values=x).logits if fam in ("vivit", "timesformer") else m(x)
    return out.float().cpu().clone()


def close(got, want):
    return float((got - want).abs().max()) <= MODEL_TOL


def check_curve(fam, m, clip, layout, grid, curve, rank, base, mode):
    """every step's logits against the model on the reference's masked clip; score and auc from the returned logits"""
    B = clip.shape[0]
    N = rank.shape[1]
    ks = R.step_counts(N, STEPS)
    assert curve.fractions.dtype == torch.float64 and curve.fractions.tolist() == [k / N for k in ks]
    assert curve.logits.dtype == torch.float32 and tuple(curve.logits.shape[:2]) == (B, STEPS + 1)
    assert curve.logits.device.type == "cpu" and tuple(curve.score.shape) == (B, STEPS + 1)
    masked = R.perturb(clip, base, rank, ks, grid, layout, mode)
    for i in range(STEPS + 1):
        want = logits_of(fam, m, masked[i].cuda())
        err = float((curve.logits[:, i] - want).abs().max())
        print(f"{fam} {mode} step {i} (k = {ks[i]} of {N}): max|logits - model(masked)| {err:.3e}")
        assert err <= MODEL_TOL, (fam, mode, i, err)
    t = torch.tensor(curve.target)
    if curve.logits.shape[2] == 1:
        p = torch.sigmoid(curve.logits[:, :, 0])
        want_score = torch.where(t[:, None] == 1, p, 1.0 - p)
    else:
        want_score = torch.softmax(curve.logits, dim=2)[torch.arange(B), :, t]
    assert curve.score.dtype == torch.float32 and torch.equal(curve.score, want_score)
    assert curve.auc.dtype == torch.float64 and torch.equal(curve.auc, R.trapezoid(curve.score, curve.fractions))



def test_deletion_and_insertion_curves_score_the_reference_masked_clips(case):
    from vclip_amd.faithfulness import perturbation_curve
    fam, m, clip, cd, layout, ex, grid, rank = case
    plain = logits_of(fam, m, cd)
    want_target = (plain[:, 0] > 0).long().tolist() if fam == "lstm" else plain.argmax(1).tolist()
    dele = perturbation_curve(m, cd, ex, mode="deletion", steps=STEPS)
    ins = perturbation_curve(m, cd, ex.saliency, mode="insertion", steps=STEPS)  # the bare map scores the same way
    assert (dele.mode, dele.baseline, dele.order) == ("deletion", "zero", "relevance") and ins.mode == "insertion"
    assert dele.target == want_target and ins.target == want_target  # the unperturbed clip's prediction
    check_curve(fam, m, clip, layout, grid, dele, rank, None, "deletion")
    check_curve(fam, m, clip, layout, grid, ins, rank, None, "insertion")
    assert close(dele.logits[:, 0], plain) and close(ins.logits[:, STEPS], plain)
    zeros = logits_of(fam, m, torch.zeros_like(cd))
    assert close(dele.logits[:, STEPS], zeros) and close(ins.logits[:, 0], zeros)
    # a map on the GPU, an asked class, two steps per forward: the same clips, the other class's score
    other = [1 - t for t in want_target]
    again = perturbation_curve(m, cd, ex.saliency.cuda(), mode="deletion", steps=STEPS, target=other, chunk=2 * clip.shape[0])
    assert again.target == other and close(again.logits, dele.logits)
    assert float((again.score + dele.score - 1).abs().max()) < 1e-2  # two labels (the LSTM: the logit's two signs)


def test_random_order_is_seeded_and_differs_from_the_relevance_order(case):
    from vclip_amd.faithfulness import cell_ranks, perturbation_curve
    fam, m, clip, cd, layout, ex, grid, rank = case
    one = perturbation_curve(m, cd, ex, order="random", seed=3, steps=STEPS)
    two = perturbation_curve(m, cd, ex, order="random", seed=3, steps=STEPS)
    assert one.order == "random" and torch.equal(one.logits, two.logits) and torch.equal(one.auc, two.auc)
    r3, r4 = cell_ranks(ex.saliency, "random", 3), cell_ranks(ex.saliency, "random", 4)
    assert not torch.equal(r3, rank) and not torch.equal(r3, r4)
    check_curve(fam, m, clip, layout, grid, one, r3, None, "deletion")  # the curve is the seeded permutation's
    mid = [R.step_counts(rank.shape[1], STEPS)[STEPS // 2]]
    assert not torch.equal(R.perturb(clip, None, r3, mid, grid, layout, "deletion"),
                           R.perturb(clip, None, rank, mid, grid, layout, "deletion"))  # other masks than the map's


def test_blur_baseline(case):
    from vclip_amd.faithfulness import BLUR_KSIZE, BLUR_SIGMA, perturbation_curve
    fam, m, clip, cd, layout, ex, grid, rank = case
    blurred = R.blur(clip, R.taps(BLUR_KSIZE, BLUR_SIGMA), torch.float32)
    assert (BLUR_KSIZE, BLUR_SIGMA) == (11, 5.0)
    ins = perturbation_curve(m, cd, ex, mode="insertion", baseline="blur", steps=STEPS)
    assert ins.baseline == "blur"
    assert close(ins.logits[:, 0], logits_of(fam, m, blurred.cuda()))  # nothing inserted yet: the canvas
    assert close(ins.logits[:, STEPS], logits_of(fam, m, cd))
    check_curve(fam, m, clip, layout, grid, ins, rank, blurred, "insertion")


def test_faithfulness_keys_and_model_state(case):
    from vclip_amd.faithfulness import PerturbationCurve, faithfulness
    fam, m, clip, cd, layout, ex, grid, rank = case
    graphed = hasattr(m, "graph_replay")
    if graphed:
        m.graph_replay = True
    before = logits_of(fam, m, cd)
    assert torch.equal(logits_of(fam, m, cd.clone()), before)  # a second tensor of the shape: the static-input graph
    captures = m._graphs.captures if graphed else None
    packed, ws = m._packed, dict(m._ws)
    f = faithfulness(m, cd, ex, steps=STEPS, seed=1)
    assert set(f) == {"deletion_auc", "insertion_auc", "random_deletion_auc", "deletion_gain", "deletion", "insertion",
                      "random_deletion", "target", "steps", "baseline"}
    B = clip.shape[0]
    for k in ("deletion_auc", "insertion_auc", "random_deletion_auc", "deletion_gain"):
        assert f[k].dtype == torch.float64 and tuple(f[k].shape) == (B,) and torch.isfinite(f[k]).all()
    assert torch.equal(f["deletion_gain"], f["random_deletion_auc"] - f["deletion_auc"])
    for k, mode, order in (("deletion", "deletion", "relevance"), ("insertion", "insertion", "relevance"),
                           ("random_deletion", "deletion", "random")):
        c = f[k]
        assert isinstance(c, PerturbationCurve) and (c.mode, c.order, c.baseline) == (mode, order, "zero")
        assert c.target == f["target"] and torch.equal(f[f"{k}_auc"], c.auc)
        assert bool(((c.score >= 0) & (c.score <= 1)).all())
    assert f["steps"] == STEPS and f["baseline"] == "zero"
    # the model is as it was: the same logits, no new capture, the same packed weights and workspaces, no gradients
    assert torch.equal(logits_of(fam, m, cd), before)
    if graphed:
        assert m._graphs.captures == captures
        m.graph_replay = False
    assert m._packed is packed and set(m._ws) == set(ws) and all(m._ws[k] is v for k, v in ws.items())
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(logits_of(fam, m, cd), before)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        faithfulness(m, cd, ex)
    m.eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        faithfulness(m, clip, ex)
