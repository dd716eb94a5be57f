"""CPU-side checks of the Video Swin saliency surface: the window rollout step and the PatchMerging hop are declared,
exported and signed and refuse bad arguments before any HIP call; the ops and `Swin3d.explain` refuse CPU tensors
instead of falling back; and the reference the GPU tests compare against checks itself on the tiny model: the stepwise
rollout against the dense matrix product, the row sums, the conservation of the relevance, and the discrimination
check -- every wrong rule (shift mask dropped, bias dropped, residual 1 instead of 0.5) must move the map by at least
four times the bound the GPU model test allows, or that test could not tell the rules apart."""
import ctypes

import pytest
import torch

import vclip_amd._lib as L
import window_rollout_ref as R
from vclip_amd import ops
from vclip_amd.build import LIB_PATH, build
from vclip_amd.weights import make_swin3d_weights, make_synthetic_video

STEP, SPREAD = "vc_window_rollout_step", "vc_merge_rollout_spread"
CLIPS = ((8, 48), (4, 48))  # (T, H = W): stage grids (4, 12, 12) -> (4, 6, 6), and (2, 12, 12) -> (2, 6, 6) (t clamped)


def test_window_rollout_symbols_declared_exported_and_signed():
    build()
    lib = ctypes.CDLL(LIB_PATH)
    for name, nargs in ((STEP, 24), (SPREAD, 7)):
        assert name in L.header_functions()
        assert hasattr(lib, name)
        argtypes, restype = L.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs and argtypes[-1] is ctypes.c_void_p  # the stream last
    assert L.SIGNATURES[STEP][0][19] is ctypes.c_float  # alpha
    assert L.SIGNATURES[STEP][0][21] is ctypes.c_int64  # work_elems


def test_window_rollout_entry_points_refuse_bad_arguments_before_any_hip_call():
    build()
    lib = L.load()
    f = getattr(lib, STEP)
    q, tab, rin, work, rout = (ctypes.c_void_p(64 + (i << 20)) for i in range(5))
    ntok = 2 * 4 * 6 * 6

    def call(qkv=q, ld=96, table=tab, r_in=rin, B=2, T=4, H=6, W=6, heads=1, hd=32, win=(2, 3, 3), sh=(1, 1, 1),
             full=(2, 3, 3), alpha=0.5, wk=work, we=3 * ntok, r_out=rout):
        return f(qkv, ld, table, r_in, B, T, H, W, heads, hd, *win, *sh, *full, alpha, wk, we, r_out, None)

    err = lambda: lib.vc_last_error().decode()  # noqa: E731
    for kw in (dict(qkv=None), dict(table=None), dict(r_in=None), dict(wk=None), dict(r_out=None)):
        assert call(**kw) != 0 and "null" in err()
    assert call(hd=64) != 0 and "head_dim" in err()
    assert call(B=0) != 0 and "shape" in err()
    assert call(ld=88) != 0 and "leading dimension" in err()  # narrower than 3*heads*32
    assert call(heads=2) != 0 and "leading dimension" in err()
    assert call(win=(2, 4, 3)) != 0 and "whole windows" in err()
    assert call(sh=(2, 1, 1)) != 0 and "shift" in err()
    assert call(win=(4, 3, 3)) != 0 and "full window" in err()
    assert call(T=16, H=14, W=14, win=(8, 14, 7), sh=(0, 0, 0), full=(8, 14, 7)) != 0 and "448" in err()
    assert call(qkv=ctypes.c_void_p(72)) != 0 and "aligned" in err()
    assert call(r_in=ctypes.c_void_p((1 << 20) + 2)) != 0 and "aligned" in err()
    assert call(we=3 * ntok - 1) != 0 and "work too small" in err()
    assert call(r_out=rin) != 0 and "alias" in err()
    assert call(r_out=ctypes.c_void_p(rin.value + 4 * (ntok - 1))) != 0 and "alias" in err()  # the last element overlaps
    assert call(wk=ctypes.c_void_p(rout.value + 16)) != 0 and "alias" in err()
    assert call(B=1 << 20, T=64, H=63, W=63, win=(2, 3, 3)) != 0 and "too large" in err()
    g = getattr(lib, SPREAD)
    assert g(None, 1, 2, 6, 6, rout, None) != 0 and "null" in err()
    assert g(rin, 1, 2, 6, 6, None, None) != 0 and "null" in err()
    assert g(rin, 0, 2, 6, 6, rout, None) != 0 and "shape" in err()
    assert g(ctypes.c_void_p(rin.value + 1), 1, 2, 6, 6, rout, None) != 0 and "aligned" in err()
    assert g(rin, 1, 2, 6, 6, rin, None) != 0 and "alias" in err()


def test_window_rollout_ops_reject_cpu_tensors():
    qkv, tab = torch.zeros(256, 128, dtype=torch.bfloat16), torch.zeros(3 * 5 * 5, 1)
    r = torch.zeros(2 * 4 * 6 * 6)
    with pytest.raises(L.VclipError):
        ops.window_rollout_step(qkv, tab, r, 2, (4, 6, 6), 1, (2, 3, 3), (0, 0, 0), (2, 3, 3), 0.5, torch.zeros(3 * 288),
                                torch.zeros(288))
    with pytest.raises(L.VclipError):
        ops.merge_rollout_spread(torch.zeros(2 * 3 * 3), 1, (2, 6, 6), torch.zeros(2 * 6 * 6))


def _swin(cfg=R.TINY):
    from vclip_amd.swin3d import Swin3d
    return Swin3d({k: v for k, v in cfg.items() if k != "num_classes"}, num_classes=cfg["num_classes"])


def test_explain_refusals_on_the_cpu():
    m = _swin().eval()
    assert m.EXPLAIN_METHODS == ("rollout",)
    video = torch.zeros(1, 3, 4, 48, 48)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain(video)
    for method in ("cls_attention", "grad_rollout", "gradcam"):  # no CLS token, and no class-specific chain
        with pytest.raises(ValueError, match="method"):
            m.explain(video, method=method)
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="residual"):
            m.explain(video, residual=bad)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.explain(video)


@pytest.fixture(scope="module", params=CLIPS, ids=lambda c: f"T{c[0]}")
def case(request):
    """(grids, per-variant matrices, the same with bf16 q / k) of the sharpened tiny model on one B = 2 fixture"""
    T, HW = request.param
    sd = R.sharpen({k: torch.from_numpy(v) for k, v in make_swin3d_weights(R.TINY, seed=0).items()})
    video = torch.from_numpy(make_synthetic_video(2, T, HW, seed=3))
    with torch.no_grad():
        _, grids, mats = R.oracle_probs(sd, R.TINY, video, variants=R.VARIANTS)
        _, _, mats16 = R.oracle_probs(sd, R.TINY, video, round_qk=True)
    return grids, mats, mats16


def test_reference_oracle_restatement_matches_the_oracle_logits():
    from oracle.swin3d_ref import swin3d_forward
    sd = {k: torch.from_numpy(v) for k, v in make_swin3d_weights(R.TINY, seed=0).items()}
    for T, HW in CLIPS:
        video = torch.from_numpy(make_synthetic_video(2, T, HW, seed=3))
        with torch.no_grad():
            logits, grids, mats = R.oracle_probs(sd, R.TINY, video)
            want = swin3d_forward(sd, R.TINY, video)
        assert float((logits - want).abs().max()) < 1e-6
        assert grids == [(T // 2, 12, 12), (T // 2, 6, 6)] and [len(st) for st in mats] == [2, 2]


def test_reference_stepwise_rollout_equals_the_dense_product(case):
    grids, mats, _ = case
    n0 = grids[0][0] * grids[0][1] * grids[0][2]
    for alpha in (0.5, 1.0):
        for st in R.step_matrices(mats, alpha):
            for M in st:
                assert float((M.sum(-1) - 1).abs().max()) < 1e-6  # fp32 softmax rows
        dense, step = R.rollout_dense(mats, grids, alpha), R.rollout_stepwise(mats, grids, alpha)
        assert tuple(step.shape) == (2, n0)
        assert float((dense - step).abs().max()) < 1e-12
        assert float((step.sum(1) - 1).abs().max()) < 1e-6  # sum r is conserved through steps and hops
        assert (step >= 0).all()


def test_reference_hop_matrix_rows_sum_to_one_on_odd_grids():
    for grid in ((2, 6, 6), (2, 5, 7), (1, 1, 1)):
        M = R.hop_matrix(grid)
        assert float((M.sum(1) - 1).abs().max()) < 1e-15 and float((M.sum(0) > 0).double().min()) == 1.0
        T, H, W = grid
        rp = torch.rand(2 * T * ((H + 1) // 2) * ((W + 1) // 2), dtype=torch.float64)
        want = (rp.reshape(2, -1) @ M).reshape(-1)
        assert float((R.spread_ref(rp, 2, grid) - want).abs().max()) < 1e-15


def test_reference_step_is_one_dense_step_matrix():
    """step_ref (what the kernel test compares against) is r (alpha A + (1 - alpha) I) for the A its own softmax gives,
    scattered through the oracle's partition: shifted, with the window clamped in t"""
    B, grid, heads, full = 2, (2, 6, 6), 2, (2, 3, 3)
    window, shift = R.O.window_and_shift(grid, full, (1, 1, 1))
    n = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * n, 3 * heads * 32, generator=g)
    qkv[:, :heads * 32] *= 0.6
    qkv = qkv.bfloat16()
    table = torch.randn(3 * 5 * 5, heads, generator=g) * 0.5
    r = torch.rand(B * n, generator=g, dtype=torch.float64) + 0.05
    got = R.step_ref(qkv, table, r, B, grid, heads, window, shift, full, 0.5, torch.float64)
    x = qkv.double().reshape(B, *grid, 3, heads, 32)
    xw = R._partition(x.reshape(B, *grid, -1), window, shift).reshape(-1, 18, 3, heads, 32)
    s = torch.einsum("wihd,wjhd->whij", xw[:, :, 0], xw[:, :, 1])
    s = s + R.LOG2E * R.O.relative_position_bias(table.double(), full, window)
    s = s.masked_fill(R.region_mask(grid, window, shift).unsqueeze(1).repeat(B, 1, 1, 1), -100.0 * 1e3)
    p = torch.softmax(s * 0.6931471805599453, dim=-1).mean(1).reshape(B, -1, 18, 18)
    A = R.scatter_dense(p, R.window_tokens(grid, window, shift), n)
    want = 0.5 * torch.einsum("bi,bij->bj", r.reshape(B, n), A) + 0.5 * r.reshape(B, n)
    assert float((got.reshape(B, n) - want).abs().max()) < 1e-12
    assert float((A.sum(-1) - 1).abs().max()) < 1e-12


def test_wrong_rules_are_told_apart_by_the_model_bound(case):
    """E of every wrong rule >= 4 x MODEL_FACTOR x the bf16-q/k yardstick, the bound of the GPU model test"""
    grids, mats, mats16 = case
    ref = R.rollout_stepwise(mats, grids, 0.5)
    yard = R.E(R.rollout_stepwise(mats16, grids, 0.5), ref)
    wrong = {"no_shift": R.E(R.rollout_stepwise(mats, grids, 0.5, "no_shift"), ref),
             "no_bias": R.E(R.rollout_stepwise(mats, grids, 0.5, "no_bias"), ref),
             "residual_1": R.E(R.rollout_stepwise(mats, grids, 1.0), ref)}
    dev = float((ref * ref.shape[1] - 1).abs().max())
    print(f"grids {grids}: yardstick {yard:.3e}, bound {R.MODEL_FACTOR * yard:.3e}, wrong rules "
          + ", ".join(f"{k} {v:.3f}" for k, v in wrong.items()) + f", max deviation from uniform {dev:.3f}")
    assert yard > 0
    assert R.MODEL_FACTOR * yard <= 0.25 * 0.33  # the condition the factor was chosen under
    for name, e in wrong.items():
        assert e >= 4 * R.MODEL_FACTOR * yard, (name, e, yard)
