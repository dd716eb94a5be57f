"""CPU-side checks of the class-specific Video Swin saliency surface (Swin3d.explain_class, --saliency class_rollout,
vc_window_grad_rollout_step): the entry is declared, exported and signed and refuses bad arguments before any HIP call;
the op and `explain_class` refuse CPU tensors instead of falling back; the parsers take the new method for Swin only;
and the reference the GPU tests compare against (tests/window_grad_rollout_ref.py) checks itself on the tiny model: the
stepwise a / base rollout against the dense matrix product, the rule's dP = dO . v^T against autograd's own dlogit/dP,
and the discrimination condition -- the maps of the two classes must differ by at least four times the bound the GPU
model test allows, and a (the part through an attention) must be so far below base (the identity path) that a map
formed as r - base, or with the identity path left in, could not pass."""
import ctypes

import pytest
import torch

import vclip_amd._lib as L
import window_grad_rollout_ref as G
import window_rollout_ref as R
from vclip_amd import ops
from vclip_amd.build import LIB_PATH, build
from vclip_amd.weights import make_swin3d_weights, make_synthetic_video

STEP = "vc_window_grad_rollout_step"
CLIPS = ((8, 48), (4, 48))  # (T, H = W): stage grids (4, 12, 12) -> (4, 6, 6), and (2, 12, 12) -> (2, 6, 6) (t clamped)
BASE = ["--video_path", "x.npy", "--model_path", "y.pth"]


def test_grad_step_symbol_declared_exported_and_signed():
    build()
    lib = ctypes.CDLL(LIB_PATH)
    assert STEP in L.header_functions() and hasattr(lib, STEP)
    argtypes, restype = L.SIGNATURES[STEP]
    assert restype is ctypes.c_int and len(argtypes) == 30 and argtypes[-1] is ctypes.c_void_p  # the stream last
    assert argtypes[3] is ctypes.c_int64  # lddo
    assert argtypes[23] is ctypes.c_float and argtypes[24] is ctypes.c_float  # alpha, beta
    assert argtypes[26] is ctypes.c_int64  # work_elems
    assert callable(ops.window_grad_rollout_step) and callable(ops.window_grad_rollout_work)


def test_grad_step_refuses_bad_arguments_before_any_hip_call():
    build()
    lib = L.load()
    f = getattr(lib, STEP)
    q, d, tab, rin, ain, base, work, aout, rout = (ctypes.c_void_p(64 + (i << 20)) for i in range(9))
    ntok = 2 * 4 * 6 * 6

    def call(qkv=q, ld=96, dout=d, lddo=32, table=tab, r_in=rin, a_in=ain, bs=base, B=2, T=4, H=6, W=6, heads=1, hd=32,
             win=(2, 3, 3), sh=(1, 1, 1), full=(2, 3, 3), alpha=1.0, beta=1.0, wk=work, we=3 * ntok, a_out=aout, r_out=rout):
        return f(qkv, ld, dout, lddo, table, r_in, a_in, bs, B, T, H, W, heads, hd, *win, *sh, *full, alpha, beta, wk, we,
                 a_out, r_out, None)

    err = lambda: lib.vc_last_error().decode()  # noqa: E731
    for kw in (dict(qkv=None), dict(dout=None), dict(table=None), dict(r_in=None), dict(a_in=None), dict(wk=None),
               dict(a_out=None)):
        assert call(**kw) != 0 and "null" in err()
    assert call(bs=None) != 0 and "come together" in err()  # base without r_out, and the reverse
    assert call(r_out=None) != 0 and "come together" in err()
    assert call(hd=64) != 0 and "head_dim" in err()
    assert call(B=0) != 0 and "shape" in err()
    assert call(ld=88) != 0 and "leading dimension" in err()
    assert call(lddo=24) != 0 and "leading dimension" in err()  # narrower than heads*32
    assert call(lddo=36) != 0 and "leading dimension" in err()  # not a multiple of 8
    assert call(heads=2) != 0 and "leading dimension" in err()
    assert call(win=(2, 4, 3)) != 0 and "whole windows" in err()
    assert call(sh=(2, 1, 1)) != 0 and "shift" in err()
    assert call(win=(4, 3, 3)) != 0 and "full window" in err()
    # an oversized window (its q' and dO rows cannot be staged): refused by volume, nothing launched
    assert call(T=16, H=14, W=14, win=(8, 14, 7), sh=(0, 0, 0), full=(8, 14, 7)) != 0 and "448" in err()
    assert call(dout=ctypes.c_void_p(72)) != 0 and "aligned" in err()
    assert call(a_in=ctypes.c_void_p((1 << 20) + 2)) != 0 and "aligned" in err()
    assert call(we=3 * ntok - 1) != 0 and "work too small" in err()
    for kw in (dict(a_out=rin), dict(a_out=ain), dict(a_out=base), dict(r_out=rin), dict(r_out=ain), dict(r_out=aout),
               dict(a_out=ctypes.c_void_p(ain.value + 4 * (ntok - 1))), dict(wk=ctypes.c_void_p(aout.value + 16)),
               dict(wk=ctypes.c_void_p(ain.value + 16))):
        assert call(**kw) != 0 and "alias" in err(), kw
    assert call(B=1 << 20, T=64, H=63, W=63, win=(2, 3, 3)) != 0 and "too large" in err()


def test_grad_step_op_rejects_cpu_tensors():
    qkv, do, tab = torch.zeros(512, 128, dtype=torch.bfloat16), torch.zeros(512, 32, dtype=torch.bfloat16), torch.zeros(75, 1)
    r = torch.zeros(2 * 4 * 6 * 6)
    with pytest.raises(L.VclipError):
        ops.window_grad_rollout_step(qkv, do, tab, r, r.clone(), 2, (4, 6, 6), 1, (2, 3, 3), (0, 0, 0), (2, 3, 3), 1.0, 1.0,
                                     torch.zeros(3 * 288), torch.zeros(288))


def _swin(cfg=R.TINY):
    from vclip_amd.swin3d import Swin3d
    return Swin3d({k: v for k, v in cfg.items() if k != "num_classes"}, num_classes=cfg["num_classes"])


def test_explain_class_refusals_on_the_cpu_and_explain_untouched():
    m = _swin().eval()
    assert m.EXPLAIN_METHODS == ("rollout",)
    video = torch.zeros(1, 3, 4, 48, 48)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain_class(video)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain_class(video, target=1)
    for bad in (2, -1, [0, 5]):
        with pytest.raises(ValueError, match="target"):
            m.explain_class(video, target=bad)
    with pytest.raises(ValueError, match="target"):
        m.explain_class(video, target=0.5)
    with pytest.raises(ValueError, match="method"):  # the new map has a method of its own
        m.explain(video, method="class_rollout")
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.explain_class(video)
    assert all(p.grad is None for p in m.parameters())


def test_class_rollout_flags():
    from vclip_amd.apps import CLASS_SPECIFIC_SALIENCY, FAMILIES, build_parser
    p = build_parser(FAMILIES["swin"], inference=True, saliency=True)  # the parser run_inference builds
    a = p.parse_args(BASE + ["--saliency", "class_rollout"])
    assert a.saliency == "class_rollout" and a.saliency_class is None
    a = p.parse_args(BASE + ["--saliency", "class_rollout", "--saliency_class", "1", "--saliency_check", "4"])
    assert a.saliency == "class_rollout" and a.saliency_class == 1 and a.saliency_check == 4
    assert CLASS_SPECIFIC_SALIENCY["swin"] == ("rise", "class_rollout")
    assert CLASS_SPECIFIC_SALIENCY["timesformer"] == ("rise",)
    with pytest.raises(SystemExit):  # TimeSformer has no such chain
        build_parser(FAMILIES["timesformer"], inference=True, saliency=True).parse_args(BASE + ["--saliency", "class_rollout"])
    with pytest.raises(SystemExit):  # the two-argument parser keeps its flag surface
        build_parser(FAMILIES["swin"], inference=True).parse_args(BASE + ["--saliency", "class_rollout"])
    for extra in (["--saliency", "grad_rollout"], ["--saliency", "rollout", "--saliency_class", "1"]):
        with pytest.raises(SystemExit):
            p.parse_args(BASE + extra)


# ------------------------------------------------------------------ the reference checks itself
def _sd(sharp):
    sd = {k: torch.from_numpy(v) for k, v in make_swin3d_weights(R.TINY, seed=0).items()}
    return R.sharpen(sd) if sharp else sd


@pytest.fixture(scope="module", params=[(T, HW, sharp) for T, HW in CLIPS for sharp in (True, False)],
                ids=lambda c: f"T{c[0]}-{'sharp' if c[2] else 'plain'}")
def case(request):
    """per target class (0, 1) of one B = 2 fixture: (grids, fp32 oracle matrices, the bf16-yardstick ones)"""
    T, HW, sharp = request.param
    sd = _sd(sharp)
    video = torch.from_numpy(make_synthetic_video(2, T, HW, seed=3))
    out = {}
    for tg in (0, 1):
        _, target, grids, mats = G.oracle_grads(sd, R.TINY, video, tg)
        _, _, _, mats16 = G.oracle_grads(sd, R.TINY, video, tg, round16=True)
        assert target == [tg, tg]
        out[tg] = (grids, mats, mats16)
    return out


def test_reference_forward_matches_the_oracle_logits_and_picks_the_argmax():
    from oracle.swin3d_ref import swin3d_forward
    sd = _sd(False)
    video = torch.from_numpy(make_synthetic_video(2, 4, 48, seed=3))
    logits, target, grids, mats = G.oracle_grads(sd, R.TINY, video)
    with torch.no_grad():
        want = swin3d_forward(sd, R.TINY, video)
    assert float((logits - want).abs().max()) < 1e-6 and target == want.argmax(1).tolist()
    assert grids == [(2, 12, 12), (2, 6, 6)] and [len(st) for st in mats] == [2, 2]


def test_rule_dP_is_autograds_gradient_of_the_logit_in_fp64():
    """dO . v^T, which the kernel forms from the chain's dO, is dlogit/dP as autograd gives it for the kept P"""
    sd = _sd(True)
    video = torch.from_numpy(make_synthetic_video(2, 4, 48, seed=3))
    for tg in (0, 1):
        _, _, _, mats = G.oracle_grads(sd, R.TINY, video, tg, dtype=torch.float64)
        for st in mats:
            for d in st:
                assert d["dP_autograd"] is not None and d["dP_autograd"].dtype == torch.float64
                scale = float(d["dP_autograd"].abs().max())
                assert scale > 0 and float((d["dP_rule"] - d["dP_autograd"]).abs().max()) <= 1e-10 * scale


def test_reference_stepwise_rollout_equals_the_dense_product(case):
    for tg in (0, 1):
        grids, mats, _ = case[tg]
        n0 = grids[0][0] * grids[0][1] * grids[0][2]
        (ad, bd), (a, b) = G.rollout_dense(mats, grids), G.rollout_stepwise(mats, grids)
        assert tuple(a.shape) == (2, n0) and (a >= 0).all()
        assert float((ad - a).abs().max()) <= 1e-12 * float(a.abs().max())
        assert float((bd - b).abs().max()) <= 1e-12 * float(b.abs().max())
        assert float((b.sum(1) - 1).abs().max()) < 1e-12  # the identity path alone conserves the seed's sum


def test_the_classes_are_told_apart_and_the_identity_split_is_visible(case):
    yards, diffs = [], []
    for b in range(2):
        sal = {}
        for tg in (0, 1):
            grids, mats, mats16 = case[tg]
            a, base = G.rollout_stepwise(mats, grids)
            a16, _ = G.rollout_stepwise(mats16, grids)
            sal[tg] = G.saliency(a)[b]
            yards.append(G.E(G.saliency(a16)[b], sal[tg]))
            ratio = float(a[b].sum() / base[b].sum())
            peak = float(sal[tg].max() / sal[tg].mean())
            # r = base + a normalised is the uniform map to 1e-4: keeping the identity path in, or forming a as r - base
            # in fp32 (2^-24 of base is 1e-3 of a at the least), cannot pass for the map
            with_identity = G.E(G.saliency((a + base))[b], sal[tg])
            print(f"clip {b} target {tg}: yardstick {yards[-1]:.2e}, sum a / sum base {ratio:.2e}, max / mean {peak:.2f}, "
                  f"E with the identity path kept {with_identity:.3f}")
            assert 5.5e-5 <= ratio <= 1.8e-4  # the figures of both T, both clips, sharpened and plain weights
            assert 2.3 <= peak <= 4.2
            assert with_identity >= 4 * G.MODEL_FACTOR * yards[-1]
        diffs.append(G.E(sal[1], sal[0]))
    print(f"E between the target-0 and target-1 maps: {diffs}")
    assert 0.5e-3 <= min(yards) and max(yards) <= 2.5e-3
    assert min(diffs) >= 0.7
    assert G.MODEL_FACTOR * max(yards) <= 0.25 * min(diffs)  # the condition the factor was chosen under
