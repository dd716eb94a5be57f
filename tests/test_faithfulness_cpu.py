"""CPU-side checks of the saliency faithfulness test: the host arithmetic of vclip_amd/faithfulness.py (ranks, step
counts, trapezoid), the two entry points of csrc/perturb.hip (declared, exported, signed, refusing bad arguments before
any HIP call), the op wrappers and perturbation_curve refusing instead of falling back, and the --saliency_check flag
of the four clip families' inference parsers."""
import ctypes

import numpy as np
import pytest
import torch

import faithfulness_ref as R
import vclip_amd._lib as L
from vclip_amd import ops
from vclip_amd.build import LIB_PATH, build

PERTURB, BLUR = "vc_perturb_clips", "vc_gaussian_blur_planes"
TINY = dict(image_size=64, num_frames=4, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=128,
            num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, hidden_act="gelu_fast",
            layer_norm_eps=1e-6, qkv_bias=True)
BASE = ["--video_path", "x.npy", "--model_path", "y.pth"]
SALIENCY_OF = {"vivit": "rollout", "timesformer": "cls_attention", "swin": "rollout", "resnet3d": "hirescam"}


# ------------------------------------------------------------------ host arithmetic
def test_relevance_ranks_are_the_stable_descending_order():
    from vclip_amd.faithfulness import cell_ranks
    g = torch.Generator().manual_seed(0)
    sal = torch.rand(3, 2, 3, 4, generator=g)
    sal[1, 0, 0, :] = sal[1, 1, 2, 3]  # ties inside a map
    rank = cell_ranks(sal)
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (3, 24)
    assert torch.equal(rank, R.ranks_of(sal))
    flat = sal.reshape(3, -1)
    for b in range(3):
        assert sorted(rank[b].tolist()) == list(range(24))  # a permutation
        order = torch.argsort(rank[b].long())               # cells in the order of removal
        v = flat[b][order]
        assert bool((v[:-1] >= v[1:]).all())                # descending
        same = v[:-1] == v[1:]
        assert bool((order[:-1][same] < order[1:][same]).all())  # equal cells: the lower index first
    # an all-equal map: the identity
    assert torch.equal(cell_ranks(torch.full((2, 2, 3, 3), 0.25)), torch.arange(18, dtype=torch.int32).expand(2, 18))
    with pytest.raises(ValueError, match="order"):
        cell_ranks(sal, order="ascending")


def test_random_ranks_are_seeded_permutations():
    from vclip_amd.faithfulness import cell_ranks
    sal = torch.zeros(3, 2, 4, 4)
    a, b, c = cell_ranks(sal, "random", seed=5), cell_ranks(sal, "random", seed=5), cell_ranks(sal, "random", seed=6)
    assert a.dtype == torch.int32 and torch.equal(a, b) and not torch.equal(a, c)
    for row in a:
        assert sorted(row.tolist()) == list(range(32))
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2])  # one draw per clip
    assert torch.equal(cell_ranks(sal[:1], "random", seed=5)[0], a[0])   # drawn in clip order


@pytest.mark.parametrize("N,steps", [(784, 10), (3, 10), (1, 4), (7, 7), (50, 1), (196, 3)])
def test_step_counts(N, steps):
    from vclip_amd.faithfulness import step_counts
    k = step_counts(N, steps)
    assert len(k) == steps + 1 and k[0] == 0 and k[-1] == N
    assert all(a <= b for a, b in zip(k, k[1:])) and k == [(i * N) // steps for i in range(steps + 1)]
    assert k == R.step_counts(N, steps)
    with pytest.raises(ValueError, match="steps"):
        step_counts(N, 0)


def test_trapezoid_matches_numpy():
    from vclip_amd.faithfulness import trapezoid
    trapz = getattr(np, "trapezoid", None) or np.trapz
    x = torch.tensor([0.0, 0.1, 0.25, 0.5, 0.8, 1.0], dtype=torch.float64)
    y = torch.tensor([[0.9, 0.7, 0.65, 0.2, 0.1, 0.05], [0.1, 0.1, 0.4, 0.8, 0.95, 1.0]])
    got = trapezoid(y, x)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,)
    np.testing.assert_allclose(got.numpy(), trapz(y.double().numpy(), x.numpy(), axis=1), rtol=1e-14, atol=0)
    assert torch.equal(got, R.trapezoid(y, x))
    assert float(trapezoid(torch.full((1, 6), 0.5), x)[0]) == 0.5


def test_taps_of_the_op_and_the_reference_agree():
    for ksize, sigma in ((11, 5.0), (31, 2.5), (1, 1.0), (5, 0.3)):
        w = ops.gaussian_taps(ksize, sigma)
        assert w.dtype == torch.float32 and torch.equal(w, R.taps(ksize, sigma))
        assert torch.equal(w, w.flip(0)) and abs(float(w.double().sum()) - 1) < 1e-6


# ------------------------------------------------------------------ the C-ABI
def test_symbols_declared_exported_and_signed():
    build()
    raw = ctypes.CDLL(LIB_PATH)
    for name, nargs in ((PERTURB, 17), (BLUR, 9)):
        assert name in L.header_functions() and hasattr(raw, name)
        argtypes, restype = L.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs and argtypes[-1] is ctypes.c_void_p  # the stream last
    assert L.SIGNATURES[BLUR][0][5] is ctypes.c_float  # sigma


def test_perturb_entry_point_refuses_bad_arguments_before_any_hip_call():
    build()
    lib = L.load()
    f = getattr(lib, PERTURB)
    err = lambda: lib.vc_last_error().decode()  # noqa: E731
    clip, base, rank, k, out = (ctypes.c_void_p(a << 20) for a in (1, 2, 3, 4, 5))

    def args(**kw):
        # (clip, base, rank, k, B, C, T, H, W, layout, Tg, Hg, Wg, F, mode, out, stream)
        d = dict(clip=clip, base=base, rank=rank, k=k, B=1, C=3, T=4, H=8, W=8, layout=0, Tg=2, Hg=2, Wg=2, F=3, mode=0,
                 out=out)
        d.update(kw)
        return tuple(d.values()) + (None,)

    for nm in ("clip", "rank", "k", "out"):
        assert f(*args(**{nm: None})) != 0 and "null" in err()
    for layout in (2, -1):
        assert f(*args(layout=layout)) != 0 and "layout" in err()
    for mode in (2, -1):
        assert f(*args(mode=mode)) != 0 and "mode" in err()
    for nm in ("B", "C", "T", "H", "W", "F"):
        assert f(*args(**{nm: 0})) != 0 and "shape" in err()
    for kw in (dict(Tg=5), dict(Hg=9), dict(Wg=9), dict(Tg=0), dict(Hg=-1), dict(Wg=0)):
        assert f(*args(**kw)) != 0 and "grid" in err()
    assert f(*args(B=1 << 20, H=64, W=64)) != 0 and "2^31" in err()
    assert f(*args(clip=ctypes.c_void_p((1 << 20) + 2))) != 0 and "aligned" in err()
    n = 1 * 3 * 4 * 8 * 8 * 4  # bytes of one copy
    for kw in (dict(out=clip), dict(out=ctypes.c_void_p((1 << 20) + n - 4)), dict(out=ctypes.c_void_p((1 << 20) - 3 * n + 4)),
               dict(out=base), dict(out=rank), dict(out=k)):
        assert f(*args(**kw)) != 0 and "alias" in err()


def test_blur_entry_point_refuses_bad_arguments_before_any_hip_call():
    build()
    lib = L.load()
    f = getattr(lib, BLUR)
    err = lambda: lib.vc_last_error().decode()  # noqa: E731
    a, b, c = (ctypes.c_void_p(v << 20) for v in (1, 2, 3))
    # (in, planes, H, W, ksize, sigma, out, work, stream)
    assert f(None, 2, 8, 8, 11, 5.0, b, c, None) != 0 and "null" in err()
    assert f(a, 2, 8, 8, 11, 5.0, None, c, None) != 0 and "null" in err()
    assert f(a, 2, 8, 8, 11, 5.0, b, None, None) != 0 and "null" in err()
    for shape in ((0, 8, 8), (2, 0, 8), (2, 8, -1)):
        assert f(a, *shape, 11, 5.0, b, c, None) != 0 and "shape" in err()
    for ksize in (10, 0, 33, 32, -3):
        assert f(a, 2, 8, 8, ksize, 5.0, b, c, None) != 0 and "ksize" in err()
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert f(a, 2, 8, 8, 11, sigma, b, c, None) != 0 and "sigma" in err()
    assert f(a, 2, 8, 8, 11, 5.0, a, c, None) != 0 and "alias" in err()
    assert f(a, 2, 8, 8, 11, 5.0, b, ctypes.c_void_p((2 << 20) + 4), None) != 0 and "alias" in err()


def test_op_wrappers_reject_cpu_tensors():
    clip = torch.zeros(1, 4, 3, 8, 8)
    rank = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(L.VclipError):
        ops.perturb_clips(clip, rank, torch.tensor([0, 8], dtype=torch.int32), (2, 2, 2), "btchw", "deletion")
    with pytest.raises(L.VclipError):
        ops.gaussian_blur_planes(clip)


# ------------------------------------------------------------------ perturbation_curve
def test_perturbation_curve_refusals_on_the_cpu():
    import vclip_amd
    from vclip_amd.faithfulness import PerturbationCurve, faithfulness, perturbation_curve
    from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
    assert vclip_amd.perturbation_curve is perturbation_curve and vclip_amd.PerturbationCurve is PerturbationCurve
    assert vclip_amd.faithfulness.faithfulness is faithfulness  # the module, exported from the package
    m = VivitForVideoClassification(VivitConfig(**TINY)).eval()
    pix, sal = torch.zeros(2, 4, 3, 64, 64), torch.rand(2, 2, 4, 4, generator=torch.Generator().manual_seed(0))
    with pytest.raises(RuntimeError, match="GPU only"):
        perturbation_curve(m, pix, sal)
    with pytest.raises(RuntimeError, match="GPU only"):
        faithfulness(m, pix, sal)
    for steps in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="steps"):
            perturbation_curve(m, pix, sal, steps=steps)
    bad = sal.clone()
    bad[1, 0, 2, 3] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        perturbation_curve(m, pix, bad)
    bad[1, 0, 2, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        perturbation_curve(m, pix, bad)
    for wrong in (sal[:1], sal[0], sal.reshape(2, 2, 16), torch.cat([sal, sal])):  # batch / rank do not fit the clip
        with pytest.raises(ValueError, match="does not fit"):
            perturbation_curve(m, pix, wrong)
    for big in (torch.rand(2, 5, 4, 4), torch.rand(2, 2, 65, 4), torch.rand(2, 2, 4, 65)):
        with pytest.raises(ValueError, match="larger than the clip"):
            perturbation_curve(m, pix, big)
    for kw in (dict(mode="occlusion"), dict(baseline="mean"), dict(order="ascending")):
        with pytest.raises(ValueError, match=list(kw)[0]):
            perturbation_curve(m, pix, sal, **kw)
    for target in (2, [0], 0.5):
        with pytest.raises(ValueError, match="target"):
            perturbation_curve(m, pix, sal, target=target)
    with pytest.raises(TypeError, match="family"):
        perturbation_curve(torch.nn.Linear(2, 2).eval(), pix, sal)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        perturbation_curve(m, pix, sal)


# ------------------------------------------------------------------ the parsers
@pytest.mark.parametrize("fam", sorted(SALIENCY_OF))
def test_saliency_check_flag(fam):
    from vclip_amd.apps import FAMILIES, build_parser
    p = build_parser(FAMILIES[fam], inference=True, saliency=True)
    assert p.parse_args(BASE).saliency_check is None
    a = p.parse_args(BASE + ["--saliency", SALIENCY_OF[fam], "--saliency_check", "4"])
    assert a.saliency_check == 4 and a.saliency == SALIENCY_OF[fam]
    for extra in (["--saliency_check", "4"],  # without --saliency
                  ["--saliency", SALIENCY_OF[fam], "--saliency_check", "0"],
                  ["--saliency", SALIENCY_OF[fam], "--saliency_check", "-2"],
                  ["--saliency", SALIENCY_OF[fam], "--saliency_check", "x"],
                  ["--saliency", SALIENCY_OF[fam], "--saliency_check", "2.5"],
                  ["--saliency", SALIENCY_OF[fam], "--saliency_check"]):
        with pytest.raises(SystemExit):
            p.parse_args(BASE + extra)
    two = build_parser(FAMILIES[fam], inference=True)  # the two-argument form does not know the flag
    assert not hasattr(two.parse_args(BASE), "saliency_check")
    with pytest.raises(SystemExit):
        two.parse_args(BASE + ["--saliency_check", "4"])
    with pytest.raises(SystemExit):
        build_parser(FAMILIES[fam], inference=False, saliency=True).parse_args(["--data_dir", "d", "--log_dir", "l",
                                                                                "--model_dir", "m", "--saliency_check", "4"])


def test_lstm_parser_has_no_saliency_check():
    from vclip_amd.apps import FAMILIES, build_parser
    for inference in (True, False):
        with pytest.raises(SystemExit):
            build_parser(FAMILIES["lstm"], inference=inference, saliency=True).parse_args(["--saliency_check", "4"])
