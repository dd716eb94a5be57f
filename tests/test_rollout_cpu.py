"""CPU-side checks of the ViViT saliency surface: the rollout entry point is declared, exported and has a
ctypes signature; `explain` refuses CPU tensors instead of falling back; `--saliency` exists for the ViViT
inference CLI only."""
import ctypes

import pytest
import torch

import vclip_amd._lib as L
from vclip_amd import apps, ops
from vclip_amd.build import LIB_PATH, build

TINY = dict(image_size=64, num_frames=4, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=128,
            num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)


def test_rollout_symbol_declared_exported_and_signed():
    build()
    assert "vc_attention_rollout_step" in L.header_functions()
    assert hasattr(ctypes.CDLL(LIB_PATH), "vc_attention_rollout_step")
    argtypes, restype = L.SIGNATURES["vc_attention_rollout_step"]
    assert restype is ctypes.c_int and len(argtypes) == 13 and argtypes[-1] is ctypes.c_void_p  # the stream last
    assert argtypes[8] is ctypes.c_float  # alpha


def test_rollout_entry_point_refuses_bad_arguments_before_any_hip_call():
    build()
    lib = L.load()
    p = ctypes.c_void_p(64)
    assert lib.vc_attention_rollout_step(None, 384, p, p, 1, 33, 2, 64, 0.5, p, 66, p, None) != 0
    assert "null" in lib.vc_last_error().decode()
    assert lib.vc_attention_rollout_step(p, 768, p, p, 1, 33, 2, 128, 0.5, p, 66, p, None) != 0
    assert "head_dim" in lib.vc_last_error().decode()
    assert lib.vc_attention_rollout_step(p, 384, p, p, 1, 33, 2, 64, 0.5, p, 65, p, None) != 0
    assert "work" in lib.vc_last_error().decode()
    assert lib.vc_attention_rollout_step(p, 384, p, p, 0, 33, 2, 64, 0.5, p, 66, p, None) != 0


def test_rollout_op_rejects_cpu_tensors():
    with pytest.raises(L.VclipError):
        ops.attention_rollout_step(torch.zeros(64, 384, dtype=torch.bfloat16), torch.zeros(66), torch.zeros(1, 33), 1,
                                   33, 2, 0.5, torch.zeros(66), torch.zeros(1, 33))


def test_explain_refuses_cpu_tensors():
    from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
    m = VivitForVideoClassification(VivitConfig(**TINY)).eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        m.explain(torch.zeros(1, 4, 3, 64, 64))
    with pytest.raises(ValueError, match="method"):
        m.explain(torch.zeros(1, 4, 3, 64, 64), method="gradcam")
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.explain(torch.zeros(1, 4, 3, 64, 64))


def test_saliency_flag_parses_for_vivit_only():
    base = ["--video_path", "v.npy", "--model_path", "m.pth"]
    p = apps.build_parser(apps.FAMILIES["vivit"], inference=True)
    assert p.parse_args(base).saliency is None  # absent by default
    for method in ("rollout", "cls_attention"):
        assert p.parse_args(base + ["--saliency", method]).saliency == method
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--saliency", "gradcam"])
    for fam in ("timesformer", "swin", "resnet3d"):
        with pytest.raises(SystemExit):
            apps.build_parser(apps.FAMILIES[fam], inference=True).parse_args(base + ["--saliency", "rollout"])
    with pytest.raises(SystemExit):
        apps.build_parser(apps.FAMILIES["lstm"], inference=True).parse_args(
            ["--videos_dir", "d", "--model_path", "m.pth", "--saliency", "rollout"])
    with pytest.raises(SystemExit):  # an inference flag: the ViViT train CLI does not get it
        apps.build_parser(apps.FAMILIES["vivit"], inference=False).parse_args(["--data_dir", "d", "--saliency", "rollout"])
