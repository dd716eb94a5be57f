"""CPU-side checks of the class-specific ViViT saliency (gradient-weighted rollout): the step's entry point is
declared, exported and has a ctypes signature, and refuses bad arguments before any HIP call; the op and `explain`
refuse CPU tensors; `target` is checked; the CLI flags exist for ViViT inference only."""
import ctypes

import pytest
import torch

import vclip_amd._lib as L
from vclip_amd import apps, ops
from vclip_amd.build import LIB_PATH, build

TINY = dict(image_size=64, num_frames=4, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=128,
            num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)
NAME = "vc_attention_grad_rollout_step"


def test_grad_rollout_symbol_declared_exported_and_signed():
    build()
    assert NAME in L.header_functions()
    assert hasattr(ctypes.CDLL(LIB_PATH), NAME)
    argtypes, restype = L.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == 16 and argtypes[-1] is ctypes.c_void_p  # the stream last
    assert argtypes[10] is ctypes.c_float and argtypes[11] is ctypes.c_float  # alpha, beta
    assert len(L.SIGNATURES["vc_attention_rollout_step"][0]) == 13  # the sibling keeps its signature


def test_grad_rollout_entry_point_refuses_bad_arguments_before_any_hip_call():
    build()
    lib = L.load()
    f = getattr(lib, NAME)
    p = ctypes.c_void_p(64)
    # (qkv, ld, dO, lddo, lse, r_in, B, S, H, head_dim, alpha, beta, work, work_elems, r_out, stream)
    assert f(None, 384, p, 128, p, p, 1, 33, 2, 64, 1.0, 1.0, p, 66, p, None) != 0
    assert "null" in lib.vc_last_error().decode()
    assert f(p, 384, None, 128, p, p, 1, 33, 2, 64, 1.0, 1.0, p, 66, p, None) != 0
    assert "null" in lib.vc_last_error().decode()
    assert f(p, 768, p, 256, p, p, 1, 33, 2, 128, 1.0, 1.0, p, 66, p, None) != 0
    assert "head_dim" in lib.vc_last_error().decode()
    assert f(p, 384, p, 128, p, p, 1, 33, 2, 64, 1.0, 1.0, p, 65, p, None) != 0
    assert "work" in lib.vc_last_error().decode()
    assert f(p, 384, p, 128, p, p, 0, 33, 2, 64, 1.0, 1.0, p, 66, p, None) != 0
    assert f(p, 384, p, 120, p, p, 1, 33, 2, 64, 1.0, 1.0, p, 66, p, None) != 0  # dO narrower than H*64
    assert "dO" in lib.vc_last_error().decode()


def test_grad_rollout_op_rejects_cpu_tensors():
    with pytest.raises(L.VclipError):
        ops.attention_grad_rollout_step(torch.zeros(64, 384, dtype=torch.bfloat16),
                                        torch.zeros(64, 128, dtype=torch.bfloat16), torch.zeros(66), torch.zeros(1, 33),
                                        1, 33, 2, 1.0, 1.0, torch.zeros(66), torch.zeros(1, 33))


def test_explain_grad_rollout_refusals_on_the_cpu():
    from vclip_amd.vivit import Explanation, VivitConfig, VivitForVideoClassification
    m = VivitForVideoClassification(VivitConfig(**TINY)).eval()
    assert "grad_rollout" in m.EXPLAIN_METHODS
    pix = torch.zeros(1, 4, 3, 64, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain(pix, method="grad_rollout")
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain(pix, method="grad_rollout", target=1)
    for method in ("rollout", "cls_attention"):
        with pytest.raises(ValueError, match="target"):  # a target is for the class-specific method only
            m.explain(pix, method=method, target=1)
    for bad in (2, -1, [0, 5], torch.tensor([7])):
        with pytest.raises(ValueError, match="out of range"):
            m.explain(pix, method="grad_rollout", target=bad)
    with pytest.raises(ValueError, match="target"):
        m.explain(pix, method="grad_rollout", target=0.5)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.explain(pix, method="grad_rollout")
    assert Explanation(None, None, None, None, "rollout").target is None


def test_grad_rollout_flags_parse_for_vivit_inference_only():
    base = ["--video_path", "v.npy", "--model_path", "m.pth"]
    p = apps.build_parser(apps.FAMILIES["vivit"], inference=True)
    a = p.parse_args(base + ["--saliency", "grad_rollout"])
    assert a.saliency == "grad_rollout" and a.saliency_class is None  # absent: the predicted class
    assert p.parse_args(base + ["--saliency", "grad_rollout", "--saliency_class", "1"]).saliency_class == 1
    assert p.parse_args(base).saliency_class is None
    for fam in ("timesformer", "swin", "resnet3d"):
        q = apps.build_parser(apps.FAMILIES[fam], inference=True)
        with pytest.raises(SystemExit):
            q.parse_args(base + ["--saliency", "grad_rollout"])
        with pytest.raises(SystemExit):
            q.parse_args(base + ["--saliency_class", "1"])
    with pytest.raises(SystemExit):
        apps.build_parser(apps.FAMILIES["lstm"], inference=True).parse_args(
            ["--videos_dir", "d", "--model_path", "m.pth", "--saliency", "grad_rollout"])
    with pytest.raises(SystemExit):  # inference flags: the ViViT train CLI does not get them
        apps.build_parser(apps.FAMILIES["vivit"], inference=False).parse_args(
            ["--data_dir", "d", "--saliency", "grad_rollout"])
