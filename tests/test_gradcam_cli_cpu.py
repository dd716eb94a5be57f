"""The ResNet3D inference parser's saliency flags (no GPU): present as run_inference builds the parser
(saliency=True), absent in the two-argument form, which keeps the reference's flag surface."""
import pytest

from vclip_amd.apps import FAMILIES, build_parser

BASE = ["--video_path", "x.npy", "--model_path", "y.pth"]


def test_resnet3d_saliency_flags_exist_under_saliency_true():
    p = build_parser(FAMILIES["resnet3d"], inference=True, saliency=True)
    a = p.parse_args(BASE)
    assert a.saliency is None and a.saliency_class is None and a.saliency_layer == "res5"
    a = p.parse_args(BASE + ["--saliency", "hirescam", "--saliency_class", "1", "--saliency_layer", "res4"])
    assert (a.saliency, a.saliency_class, a.saliency_layer) == ("hirescam", 1, "res4")
    assert p.parse_args(BASE + ["--saliency", "gradcam"]).saliency == "gradcam"
    for extra in (["--saliency", "rollout"], ["--saliency", "grad_rollout"], ["--saliency", "gradcam", "--saliency_layer", "res3"],
                  ["--saliency", "gradcam", "--saliency_layer", "res2"], ["--saliency_class", "one"]):
        with pytest.raises(SystemExit):
            p.parse_args(BASE + extra)


def test_resnet3d_two_argument_parser_keeps_todays_flags():
    p = build_parser(FAMILIES["resnet3d"], inference=True)
    a = p.parse_args(BASE)
    assert not any(hasattr(a, k) for k in ("saliency", "saliency_class", "saliency_layer"))
    for extra in (["--saliency", "gradcam"], ["--saliency_class", "1"], ["--saliency_layer", "res4"]):
        with pytest.raises(SystemExit):
            p.parse_args(BASE + extra)


@pytest.mark.parametrize("fam", ["timesformer", "swin"])
def test_other_families_get_no_class_or_layer_flag(fam):
    p = build_parser(FAMILIES[fam], inference=True, saliency=True)
    for extra in (["--saliency_class", "1"], ["--saliency_layer", "res4"], ["--saliency", "gradcam"]):
        with pytest.raises(SystemExit):
            p.parse_args(BASE + extra)

