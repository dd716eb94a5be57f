"""RISE saliency on the GPU: the two kernels of csrc/rise.hip against the float64 reference tests/rise_ref.py, the
planted scorer through the kernels, and rise_map on one tiny model per family (the seeded synthetic weights and shapes
of tests/test_faithfulness_gpu.py) against the same model run on the reference's masked clips.

Bounds, with u = 2^-24 (fp32 unit roundoff), derived from the fixed operation order and not from a measured error:

  the mask      Each fraction f = float(r) / float(S) is one correctly rounded division: relative error <= u.  A step is
                fmaf(f, b - a, a), a convex combination (f in [0, 1)), so it passes on its inputs' error e and adds at
                most u for f's error (|b - a| <= 1), u for the rounded b - a and u for its own rounding: e + 3u.  The
                four x steps see exact bits (b - a exact): <= 2u.  Then y: <= 5u, then t: <= 8u.  So |m - m_ref| <= 8u
                over three divisions and seven steps, and the computed m stays in [0, 1].
  vc_rise_apply out = fmaf(m, x, (1 - m) * z): the mask error times (|x| + |z|), u|z| for 1 - m, u|z| for the product,
                u(|x| + |z|) for the fma: <= 11u (|x| + |z|).  Asserted: |out - ref| <= 32 u (|x| + |z|) per element.
                Where the eight corner bits agree every step returns the bit, and m = 1 gives fmaf(1, x, 0 * z) = x,
                m = 0 gives fmaf(0, x, z) = z, bit for bit (without a base: 0 * x, a zero of x's sign).
  vc_rise_accumulate  a = fmaf(w_f, m_f, a) over f in order with w >= 0: F roundings of non-decreasing partial sums,
                each <= u ref(1 + O(Fu)), plus the mask error sum_f w_f 8u.  Asserted:
                |acc - ref| <= u ((F + 2) ref + 32 sum_f w_f) per pixel.
  rise_map      mask_logits within 1e-2 of the model on the reference's masked clip (the project's model bound, as in
                test_faithfulness_gpu.py); the maps against the reference accumulate of the returned mask_scores within
                the accumulate bound carried through the two normalisations (see check_maps).

No test here asserts that a map of an untrained model is good; the planted scorer is what shows that the method points
where the score comes from."""
import pytest
import torch

import rise_ref as R
from vclip_amd import ops

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SHAPES = [(1, 3, 2, 8, 8, (1, 2, 2)), (2, 3, 8, 64, 64, (4, 4, 4)),
          (1, 3, 4, 50, 70, (2, 3, 4)),   # extents the cells do not divide, quads that straddle rows
          (1, 1, 3, 7, 5, (3, 7, 5)),     # every S == 1, and 105 elements: the scalar path
          (2, 3, 4, 32, 32, (1, 1, 1))]   # B, C, T, H, W, cells


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def mask_counts():
    return (1, 5, ops.rise_mask_tile() + 5)  # the last: two staging rounds, the second partly filled


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def inputs(B, C, T, H, W, cells, layout, F):
    g = torch.Generator().manual_seed(B * 1000 + H + F)
    shape = (B, T, C, H, W) if layout == "btchw" else (B, C, T, H, W)
    clip, base = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    bits, shifts = R.sample(T, H, W, cells, 0.5, F, seed=F)
    return clip, base, bits, shifts


# ------------------------------------------------------------------ 1. vc_rise_apply
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("B,C,T,H,W,cells", SHAPES)
def test_rise_apply_matches_fp64(B, C, T, H, W, cells, layout):
    for F in mask_counts():
        clip, base, bits, shifts = inputs(B, C, T, H, W, cells, layout, F)
        cd, bd, bitd, shd = clip.cuda(), base.cuda(), bits.cuda(), shifts.cuda()
        m = R.masks_all(bits, shifts, T, H, W, cells)
        same = torch.stack([R.corners_equal(bits, shifts, n, T, H, W, cells) for n in range(F)])
        spread = (lambda t: t[:, None, :, None]) if layout == "btchw" else (lambda t: t[:, None, None])
        for b_host, b_dev in ((None, None), (base, bd)):
            got = ops.rise_apply(cd, bitd, shd, cells, layout, base=b_dev).cpu()
            assert tuple(got.shape) == (F,) + tuple(clip.shape)
            ref = R.apply(clip, b_host, m, layout)
            scale = clip.double().abs() + (0.0 if b_host is None else base.double().abs())
            excess = float(((got.double() - ref).abs() - 32 * U * scale[None]).max())
            worst = float(((got.double() - ref).abs() / scale[None]).max() / U)
            print(f"apply {(B, C, T, H, W, cells)} {layout} F {F} base {b_host is not None}: max err {worst:.2f} u(|x|+|z|), bound 32")
            assert excess <= 0.0, (F, b_host is None, worst)
            # equal corners: the clip's bits where the mask is 1, the base's where it is 0
            one = spread(same & (m == 1.0)).expand_as(got)
            zero = spread(same & (m == 0.0)).expand_as(got)
            xs = clip[None].expand_as(got)
            assert same_bits(got[one], xs[one])
            if b_host is None:
                assert bool((got[zero] == 0.0).all())
            else:
                assert same_bits(got[zero], base[None].expand_as(got)[zero])
        assert same_bits(cd.cpu(), clip) and same_bits(bd.cpu(), base)  # the inputs are untouched
        assert torch.equal(bitd.cpu(), bits) and torch.equal(shd.cpu(), shifts)


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("B,C,T,H,W,cells", SHAPES)
def test_rise_apply_constant_grids_copy_bits(B, C, T, H, W, cells, layout):
    clip, base, bits, shifts = inputs(B, C, T, H, W, cells, layout, 5)
    cd, bd, shd = clip.cuda(), base.cuda(), shifts.cuda()
    ones, zeros = torch.ones_like(bits).cuda(), torch.zeros_like(bits).cuda()
    for copy in ops.rise_apply(cd, ones, shd, cells, layout, base=bd).cpu():
        assert same_bits(copy, clip)
    for copy in ops.rise_apply(cd, ones, shd, cells, layout).cpu():
        assert same_bits(copy, clip)
    for copy in ops.rise_apply(cd, zeros, shd, cells, layout, base=bd).cpu():
        assert same_bits(copy, base)
    assert bool((ops.rise_apply(cd, zeros, shd, cells, layout) == 0.0).all())


def test_rise_apply_unaligned_pointers_take_the_scalar_path():
    B, C, T, H, W, cells = SHAPES[2]
    clip, base, bits, shifts = inputs(B, C, T, H, W, cells, "bcthw", 3)
    n = clip.numel()
    cd = torch.empty(n + 1, device="cuda")[1:].view(clip.shape).copy_(clip)  # 4 bytes past a 16-byte boundary
    od = torch.empty(3 * n + 3, device="cuda")[3:].view((3,) + tuple(clip.shape))
    got = ops.rise_apply(cd, bits.cuda(), shifts.cuda(), cells, "bcthw", base=base.cuda(), out=od)
    assert got.data_ptr() % 16 != 0 and cd.data_ptr() % 16 != 0
    aligned = ops.rise_apply(clip.cuda(), bits.cuda(), shifts.cuda(), cells, "bcthw", base=base.cuda())
    assert same_bits(got.cpu(), aligned.cpu())  # the vector path computes the same bits


def test_rise_op_refusals():
    from vclip_amd._lib import VclipError
    clip = torch.zeros(1, 3, 4, 8, 8, device="cuda")
    bits, shifts = (t.cuda() for t in R.sample(4, 8, 8, (2, 2, 2), 0.5, 3, 0))
    ok = dict(clip=clip, bits=bits, shifts=shifts, cells=(2, 2, 2), layout="bcthw")
    ops.rise_apply(**ok)
    for kw in (dict(layout="bthwc"), dict(cells=(5, 2, 2)), dict(cells=(2, 2)), dict(cells=(2, 2, 3)), dict(clip=clip.double()),
               dict(clip=clip[:, :, :, :, ::2]), dict(bits=bits.int()), dict(bits=bits[:, :3]), dict(shifts=shifts.long()),
               dict(shifts=shifts[:2]), dict(base=clip[0]), dict(out=torch.empty(1, 1, 3, 4, 8, 8, device="cuda")),
               dict(shifts=shifts.cpu())):
        with pytest.raises(VclipError):
            ops.rise_apply(**dict(ok, **kw))
    acc, w = torch.zeros(1, 4, 8, 8, device="cuda"), torch.ones(3, 1, device="cuda")
    ok = dict(acc=acc, bits=bits, shifts=shifts, w=w, cells=(2, 2, 2))
    assert ops.rise_accumulate(**ok) is acc
    for kw in (dict(acc=acc[0]), dict(acc=acc.double()), dict(w=w[:2]), dict(w=torch.ones(3, 2, device="cuda")), dict(w=w.double()),
               dict(cells=(2, 2, 9)), dict(bits=bits[:2]), dict(w=w.cpu())):
        with pytest.raises(VclipError):
            ops.rise_accumulate(**dict(ok, **kw))


# ------------------------------------------------------------------ 2. vc_rise_accumulate
@pytest.mark.parametrize("B,C,T,H,W,cells", SHAPES)
def test_rise_accumulate_matches_fp64_and_is_split_invariant(B, C, T, H, W, cells):
    for F in mask_counts():
        bits, shifts = R.sample(T, H, W, cells, 0.5, F, seed=10 + F)
        w = torch.rand(F, B, generator=torch.Generator().manual_seed(F))  # random, non-negative
        bitd, shd, wd = bits.cuda(), shifts.cuda(), w.cuda()
        m = R.masks_all(bits, shifts, T, H, W, cells)
        ref = R.accumulate(torch.zeros(B, T, H, W), m, w)
        got = ops.rise_accumulate(torch.zeros(B, T, H, W, device="cuda"), bitd, shd, wd, cells)
        bound = U * ((F + 2) * ref + 32 * w.double().sum(dim=0)[:, None, None, None])
        err = (got.cpu().double() - ref).abs()
        print(f"accumulate {(B, T, H, W, cells)} F {F}: max err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), F
        again = ops.rise_accumulate(torch.zeros(B, T, H, W, device="cuda"), bitd, shd, wd, cells)
        assert same_bits(again, got)  # two runs
        one = ops.rise_accumulate(torch.zeros(1, T, H, W, device="cuda"), bitd, shd, wd[:, :1].contiguous(), cells)
        two = ops.rise_accumulate(torch.zeros(2, T, H, W, device="cuda"), bitd, shd, wd[:, [0, 0]].contiguous() if B == 1
                                  else wd[:, :2].contiguous(), cells)
        assert same_bits(one[0], two[0]) and same_bits(one[0], got[0])  # clip 0 does not depend on B
        if F > 8:  # one launch against consecutive chunks (1, 7, rest)
            parts = torch.zeros(B, T, H, W, device="cuda")
            for lo, hi in ((0, 1), (1, 8), (8, F)):
                ops.rise_accumulate(parts, bitd[lo:hi], shd[lo:hi], wd[lo:hi], cells)
            assert same_bits(parts, got)
        assert torch.equal(bitd.cpu(), bits) and torch.equal(shd.cpu(), shifts) and same_bits(wd.cpu(), w)


def test_accumulate_and_apply_share_one_mask():
    """a clip of ones under mask f is the mask itself: accumulate with weight 1 on one mask gives apply's bits"""
    B, C, T, H, W, cells = SHAPES[2]
    bits, shifts = (t.cuda() for t in R.sample(T, H, W, cells, 0.5, 4, 0))
    masks = ops.rise_apply(torch.ones(1, 1, T, H, W, device="cuda"), bits, shifts, cells, "bcthw")
    for f in range(4):
        acc = ops.rise_accumulate(torch.zeros(1, T, H, W, device="cuda"), bits[f:f + 1], shifts[f:f + 1],
                                  torch.ones(1, 1, device="cuda"), cells)
        assert same_bits(acc[0], masks[f, 0, 0])


# ------------------------------------------------------------------ 3. the planted scorer through the kernels
def test_planted_scorer_through_the_kernels():
    shape, cells, box = (1, 3, 4, 32, 32), (2, 4, 4), (8, 20, 10, 22)
    bits, shifts, ref_scores, ref_map = R.planted(R.PLANTED_SEED, shape=shape, cells=cells, masks=256, box=box)
    bitd, shd = bits.cuda(), shifts.cuda()
    masked = ops.rise_apply(torch.ones(shape, device="cuda"), bitd, shd, cells, "bcthw")  # [256, 1, 3, 4, 32, 32]
    scores = masked[..., box[0]:box[1], box[2]:box[3]].mean(dim=(2, 3, 4, 5))                # [256, 1], on the device
    assert float((scores.cpu().double() - ref_scores).abs().max()) < 1e-5
    sal = ops.rise_accumulate(torch.zeros(1, 4, 32, 32, device="cuda"), bitd, shd, scores.contiguous(), cells).cpu()
    assert R.planted_holds(sal.double(), box)
    assert float((sal.double() - ref_map).abs().max()) <= 1e-4 * float(ref_map.max())


# ------------------------------------------------------------------ 4. rise_map, one tiny model per family
MASKS, CELLS, KEEP, SEED, STEPS = 48, (None, 4, 4), 0.5, 2, 4


@pytest.fixture(scope="module", params=["lstm", "resnet3d", "swin", "timesformer", "vivit"])
def case(request):
    """(family, model, host clip, device clip, layout, cells, reference masks f64 [F, T, H, W], the model's logits on the
    reference's masked clips [B, F, labels], the unperturbed logits), computed once"""
    import test_faithfulness_gpu as FG
    fam = request.param
    m, clip, _ = FG.FAMILIES[fam]()
    m = m.cuda().eval()
    layout = "btchw" if fam in ("vivit", "timesformer") else "bcthw"
    T = clip.shape[1] if layout == "btchw" else clip.shape[2]
    H, W = clip.shape[3], clip.shape[4]
    cells = (max(1, T // 8), CELLS[1], CELLS[2])
    bits, shifts = R.sample(T, H, W, cells, KEEP, MASKS, SEED)
    masks = R.masks_all(bits, shifts, T, H, W, cells)
    masked = R.apply(clip, None, masks, layout).float()
    want = torch.stack([FG.logits_of(fam, m, masked[f].cuda()) for f in range(MASKS)], dim=1)
    return fam, m, clip, clip.cuda(), layout, cells, masks, want, FG.logits_of(fam, m, clip.cuda())


def check_maps(ex, masks, keep):
    """saliency and token_relevance against the reference accumulate of the returned scores.  With ref the f64 sum and
    b = u ((F + 2) ref + 32 sum w) the accumulate bound per pixel: token_relevance = fl(acc / (F keep)) adds one rounding
    (F keep is exact here), within the F + 2; saliency = acc / sum(acc) in f64, rounded once:
    |acc_i / Sa - ref_i / Sr| <= (b_i + ref_i sum(b) / Sr) / Sa, plus u ref_i / Sr for the rounding."""
    F = masks.shape[0]
    B = ex.mask_scores.shape[0]
    w = ex.mask_scores.t().contiguous()  # [F, B]
    ref = R.accumulate(torch.zeros((B,) + tuple(masks.shape[1:])), masks, w)
    b = U * ((F + 2) * ref + 32 * w.double().sum(dim=0)[:, None, None, None])
    rel = ex.token_relevance.double().reshape(ref.shape) * (F * keep)
    assert bool(((rel - ref).abs() <= b).all())
    Sr = ref.sum(dim=(1, 2, 3), keepdim=True)
    Sa = Sr - b.sum(dim=(1, 2, 3), keepdim=True)  # the least the kernel's sum can be
    tol = (b + ref * b.sum(dim=(1, 2, 3), keepdim=True) / Sr) / Sa + U * ref / Sr
    assert bool(((ex.saliency.double() - ref / Sr).abs() <= tol).all())


@pytest.mark.parametrize("chunk", [16, 48])
def test_rise_map_scores_the_reference_masked_clips(case, chunk):
    import test_faithfulness_gpu as FG
    from vclip_amd.rise import RiseExplanation, rise_map
    from vclip_amd.vivit import Explanation
    fam, m, clip, cd, layout, cells, masks, want, plain = case
    B = clip.shape[0]
    T, H, W = masks.shape[1:]
    want_target = (plain[:, 0] > 0).long().tolist() if fam == "lstm" else plain.argmax(1).tolist()
    ex = rise_map(m, cd, masks=MASKS, cells=CELLS, keep=KEEP, seed=SEED, chunk=chunk)
    assert isinstance(ex, RiseExplanation) and isinstance(ex, Explanation) and ex.method == "rise"
    assert ex.target == want_target  # target None: the unperturbed clip's prediction
    assert (ex.masks, ex.cells, ex.keep, ex.seed, ex.baseline) == (MASKS, cells, KEEP, SEED, "zero")
    assert float((ex.logits.float().cpu() - plain).abs().max()) <= FG.MODEL_TOL
    assert ex.mask_logits.dtype == torch.float32 and tuple(ex.mask_logits.shape[:2]) == (B, MASKS)
    err = float((ex.mask_logits - want).abs().max())
    print(f"{fam} chunk {chunk}: max|mask_logits - model(reference masked clip)| {err:.3e}")
    assert err <= FG.MODEL_TOL
    spread = float((ex.mask_logits.max(dim=1).values - ex.mask_logits.min(dim=1).values).max())
    print(f"{fam} chunk {chunk}: the logits range over {spread:.3e} across the masks")
    assert spread > 0.0  # the masked clips reach the model: the comparison above is not of constants
    t = torch.tensor(ex.target)
    if ex.mask_logits.shape[2] == 1:
        p = torch.sigmoid(ex.mask_logits[:, :, 0])
        score = torch.where(t[:, None] == 1, p, 1.0 - p)
    else:
        score = torch.softmax(ex.mask_logits, dim=2)[torch.arange(B), :, t]
    assert ex.mask_scores.dtype == torch.float32 and torch.equal(ex.mask_scores, score)
    assert ex.saliency.dtype == torch.float32 and tuple(ex.saliency.shape) == (B, T, H, W)
    assert ex.token_relevance.dtype == torch.float32 and tuple(ex.token_relevance.shape) == (B, T * H * W)
    assert tuple(ex.temporal.shape) == (B, T) and torch.equal(ex.temporal, ex.saliency.sum(dim=(2, 3)))
    assert ex.saliency.device.type == "cpu" and bool((ex.saliency >= 0).all())
    assert float((ex.saliency.double().sum(dim=(1, 2, 3)) - 1).abs().max()) < 1e-5
    check_maps(ex, masks, KEEP)


def test_rise_map_target_baseline_and_faithfulness(case):
    import test_faithfulness_gpu as FG
    from vclip_amd.faithfulness import BLUR_KSIZE, BLUR_SIGMA, PerturbationCurve, faithfulness
    from vclip_amd.rise import rise_map
    import faithfulness_ref as FR
    fam, m, clip, cd, layout, cells, masks, want, plain = case
    B = clip.shape[0]
    mine = rise_map(m, cd, masks=MASKS, cells=CELLS, keep=KEEP, seed=SEED, chunk=16)
    other = [1 - t for t in mine.target]
    ex = rise_map(m, cd, target=other, masks=MASKS, cells=CELLS, keep=KEEP, seed=SEED, chunk=16)
    assert ex.target == other and torch.equal(ex.mask_logits, mine.mask_logits)  # the same clips, the other class's score
    assert float((ex.mask_scores + mine.mask_scores - 1).abs().max()) < 1e-2
    check_maps(ex, masks, KEEP)
    again = rise_map(m, cd, target=other, masks=MASKS, cells=CELLS, keep=KEEP, seed=SEED, chunk=16)
    assert torch.equal(again.saliency, ex.saliency) and torch.equal(again.mask_logits, ex.mask_logits)
    # blur: a masked-out pixel shows the blurred clip
    blurred = FR.blur(clip, FR.taps(BLUR_KSIZE, BLUR_SIGMA), torch.float32)
    bl = rise_map(m, cd, masks=8, cells=CELLS, keep=KEEP, seed=SEED, baseline="blur", chunk=8)
    assert bl.baseline == "blur"
    bits8, shifts8 = R.sample(masks.shape[1], masks.shape[2], masks.shape[3], cells, KEEP, 8, SEED)
    masked = R.apply(clip, blurred, R.masks_all(bits8, shifts8, *masks.shape[1:], cells), layout).float()
    ref8 = torch.stack([FG.logits_of(fam, m, masked[f].cuda()) for f in range(8)], dim=1)
    assert float((bl.mask_logits - ref8).abs().max()) <= FG.MODEL_TOL
    # the result goes straight into the faithfulness test, whose grid is then the pixel grid
    f = faithfulness(m, cd, mine, steps=STEPS)
    N = masks.shape[1] * masks.shape[2] * masks.shape[3]
    for k in ("deletion", "insertion", "random_deletion"):
        c = f[k]
        assert isinstance(c, PerturbationCurve) and tuple(c.score.shape) == (B, STEPS + 1)
        assert c.fractions.tolist() == [(i * N // STEPS) / N for i in range(STEPS + 1)]
    assert f["target"] == mine.target
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        rise_map(m, cd, masks=4, cells=CELLS)
    m.eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        rise_map(m, clip, masks=4, cells=CELLS)
