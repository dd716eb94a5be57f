"""CPU-side checks of the TimeSformer saliency surface: the temporal rollout step is declared, exported and signed and
refuses bad arguments before any HIP call; the op and `explain` refuse CPU tensors instead of falling back; and the
reference the GPU tests compare against checks itself on the tiny golden: the stepwise rollout against the dense
S x S product, the row sums, and the restated oracle loop against the golden logits."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import divided_rollout_ref as R
import vclip_amd._lib as L
from vclip_amd import ops
from vclip_amd.build import LIB_PATH, build
from vclip_amd.weights import make_timesformer_weights

GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "vc_temporal_rollout_step"
TINY = dict(image_size=64, patch_size=16, num_frames=4, num_channels=3, hidden_size=128, num_hidden_layers=2,
            num_attention_heads=2, intermediate_size=256)


def test_temporal_rollout_symbol_declared_exported_and_signed():
    build()
    assert NAME in L.header_functions()
    assert hasattr(ctypes.CDLL(LIB_PATH), NAME)
    argtypes, restype = L.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == 12 and argtypes[-1] is ctypes.c_void_p  # the stream last
    assert argtypes[8] is ctypes.c_float  # alpha
    assert len(L.SIGNATURES["vc_attention_rollout_step"][0]) == 13  # the spatial step keeps its signature


def test_temporal_rollout_entry_point_refuses_bad_arguments_before_any_hip_call():
    build()
    lib = L.load()
    f = getattr(lib, NAME)
    p, q, r = ctypes.c_void_p(64), ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)
    # (qkv, ld, r_frame_in, B, P, T, H, head_dim, alpha, r_clip_out, r_frame_out, stream)
    for args in ((None, 384, p, 1, 3, 4, 2, 64, 0.5, q, r, None), (p, 384, None, 1, 3, 4, 2, 64, 0.5, q, r, None),
                 (p, 384, p, 1, 3, 4, 2, 64, 0.5, None, r, None)):
        assert f(*args) != 0
        assert "null" in lib.vc_last_error().decode()
    assert f(p, 768, p, 1, 3, 4, 2, 128, 0.5, q, r, None) != 0
    assert "head_dim" in lib.vc_last_error().decode()
    assert f(p, 384, p, 1, 3, 33, 2, 64, 0.5, q, r, None) != 0
    assert "T > 32" in lib.vc_last_error().decode()
    assert f(p, 384, p, 0, 3, 4, 2, 64, 0.5, q, r, None) != 0
    assert "shape" in lib.vc_last_error().decode()
    assert f(p, 380, p, 1, 3, 4, 2, 64, 0.5, q, r, None) != 0  # ld narrower than 3*H*64
    assert f(ctypes.c_void_p(72), 384, p, 1, 3, 4, 2, 64, 0.5, q, r, None) != 0
    assert "aligned" in lib.vc_last_error().decode()
    assert f(p, 384, q, 1, 3, 4, 2, 64, 0.5, q, r, None) != 0  # r_clip_out on r_frame_in
    assert "alias" in lib.vc_last_error().decode()
    assert f(p, 384, q, 1, 3, 4, 2, 64, 0.5, r, ctypes.c_void_p((1 << 20) + 16), None) != 0  # r_frame_out inside it
    assert "alias" in lib.vc_last_error().decode()


def test_temporal_rollout_op_rejects_cpu_tensors():
    with pytest.raises(L.VclipError):
        ops.temporal_rollout_step(torch.zeros(64, 384, dtype=torch.bfloat16), torch.zeros(4, 4), 1, 3, 4, 2, 0.5,
                                  torch.zeros(1, 13), torch.zeros(4, 4))


def test_explain_refusals_on_the_cpu():
    from vclip_amd.timesformer import TimesformerConfig, TimesformerForVideoClassification
    m = TimesformerForVideoClassification(TimesformerConfig(**TINY)).eval()
    assert m.EXPLAIN_METHODS == ("rollout", "cls_attention")
    pix = torch.zeros(1, 4, 3, 64, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain(pix)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain(pix, method="cls_attention")
    for method in ("gradcam", "grad_rollout"):  # the class-specific method is ViViT's only
        with pytest.raises(ValueError, match="method"):
            m.explain(pix, method=method)
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="residual"):
            m.explain(pix, residual=bad)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.explain(pix)


@pytest.fixture(scope="module")
def tiny():
    g = np.load(os.path.join(GD, "timesformer_tiny.npz"))
    cfg = json.loads(str(g["config"]))
    sd = {k: torch.from_numpy(v) for k, v in make_timesformer_weights(cfg, seed=0).items()}
    with torch.no_grad():
        logits, probs = R.oracle_probs(sd, cfg, torch.from_numpy(g["pixel_values"]))
    return cfg, torch.from_numpy(g["logits"]), logits, probs


def test_reference_oracle_restatement_matches_the_golden_logits(tiny):
    cfg, want, logits, probs = tiny
    assert float((logits - want).abs().max()) < 1e-6
    B, P, T, H = 3, 16, 4, 2
    assert len(probs) == cfg["num_hidden_layers"]
    assert all(tuple(at.shape) == (B, P, H, T, T) and tuple(as_.shape) == (B, T, H, 1 + P, 1 + P) for at, as_ in probs)


def test_reference_stepwise_rollout_equals_the_dense_product(tiny):
    _, _, _, probs = tiny
    for alpha in (0.5, 1.0):
        for at, as_ in probs:
            for M in R.layer_matrices(at, as_, alpha):
                assert float((M.sum(-1) - 1).abs().max()) < 1e-6  # fp32 softmax rows
        dense, step = R.rollout_dense(probs, alpha), R.rollout_stepwise(probs, alpha)
        assert tuple(step.shape) == (3, 65)
        assert float((dense - step).abs().max()) < 1e-12
        assert float((step.sum(1) - 1).abs().max()) < 1e-6
    # cls_attention: the CLS row of the last layer's spatial matrix alone at alpha = 1
    _, Ms = R.layer_matrices(*probs[-1], 1.0)
    assert float((Ms[:, 0, :] - R.cls_attention_row(probs)).abs().max()) < 1e-12


def test_reference_temporal_step_is_one_temporal_matrix():
    """temporal_step_ref (what the kernel test compares against) is r A_t for the A_t its own softmax gives"""
    B, P, T, H = 2, 3, 4, 2
    g = torch.Generator().manual_seed(0)
    S = 1 + P * T
    qkv = torch.randn(B * S, 3 * H * 64, generator=g)
    qkv[:, :H * 64] *= 0.45
    qkv = qkv.bfloat16()
    rf = torch.rand(B * T, 1 + P, generator=g) + 0.05
    clip, frame = R.temporal_step_ref(qkv, rf, B, P, T, H, 0.5, torch.float64)
    x = qkv.double().reshape(B, S, 3, H, 64)[:, 1:].reshape(B, P, T, 3, H, 64)
    s = torch.einsum("bpthd,bpkhd->bphtk", x[:, :, :, 0], x[:, :, :, 1])
    at = torch.softmax(s * np.log(2.0), dim=-1)
    as_ = torch.eye(1 + P, dtype=torch.float64).expand(B, T, H, 1 + P, 1 + P)
    Mt, _ = R.layer_matrices(at, as_, 0.5)
    r = torch.cat([rf.double().reshape(B, T, 1 + P)[:, :, 0].sum(1, keepdim=True),
                   rf.double().reshape(B, T, 1 + P)[:, :, 1:].transpose(1, 2).reshape(B, P * T)], 1)
    assert float((torch.einsum("bi,bij->bj", r, Mt) - clip).abs().max()) < 1e-12
    fr = frame.reshape(B, T, 1 + P)
    assert torch.equal(fr[:, :, 1:].transpose(1, 2).reshape(B, P * T), clip[:, 1:])
    assert torch.equal(fr[:, :, 0], (clip[:, 0] / T)[:, None].expand(B, T))
