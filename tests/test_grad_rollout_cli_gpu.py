"""cli/vivit_transformer/inference.py --saliency grad_rollout [--saliency_class N] on the GPU: a tiny ViViT
checkpoint (reference dict schema) and a raw uint8 .npy clip, as tests/test_rollout_cli_gpu.py makes them.  The
"saliency" object of the result JSON names the explained class for this method only."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(image_size=224, num_frames=8, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=128,
           num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, hidden_act="gelu_fast",
           layer_norm_eps=1e-6, qkv_bias=True)
FRAMES = 20
TODAY = {"video_path", "predicted_class", "class_id", "confidence", "class_mapping"}
SALIENCY_KEYS = {"method", "file", "shape", "temporal_importance", "tubelet_frame_indices"}
ID2LABEL = {0: "non-referral", 1: "referral"}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd.vivit import VivitConfig
    from vclip_amd.weights import make_vivit_weights
    root = tmp_path_factory.mktemp("grad_saliency_cli")
    config = VivitConfig(**CFG, id2label=ID2LABEL)
    sd = {k: torch.from_numpy(v) for k, v in make_vivit_weights(CFG, seed=0).items()}
    torch.save({"model_state_dict": sd, "config": config.to_dict(), "id2label": ID2LABEL,
                "label2id": {v: k for k, v in ID2LABEL.items()}, "num_frames": CFG["num_frames"]}, root / "ck.pth")
    np.save(root / "clip.npy", np.random.RandomState(0).randint(0, 256, (FRAMES, 224, 224, 3)).astype(np.uint8))
    return root


def _run(files, log, extra):
    from vclip_amd.apps import run_inference
    res = run_inference("vivit", ["--video_path", str(files / "clip.npy"), "--model_path", str(files / "ck.pth"),
                                  "--log_dir", str(files / log), "--num_frames", str(CFG["num_frames"])] + extra)
    (exp,) = sorted((files / log).iterdir())
    return res, exp / "inference_results"


def _map(out, s):
    sal = np.load(out / s["file"])
    assert sal.dtype == np.float32 and list(sal.shape) == [CFG["num_frames"] // 2, 14, 14] == s["shape"]
    assert (sal >= 0).all() and abs(float(sal.astype(np.float64).sum()) - 1) < 1e-5
    np.testing.assert_allclose(s["temporal_importance"], sal.sum(axis=(1, 2)), rtol=1e-5)
    return sal


def test_inference_grad_rollout_names_the_predicted_class(files):
    res, out = _run(files, "grad", ["--saliency", "grad_rollout"])
    saved = json.load(open(out / "clip_result.json"))
    assert set(saved) == TODAY | {"saliency"}
    s = saved["saliency"]
    assert set(s) == SALIENCY_KEYS | {"target_class", "target_label"}
    assert s["method"] == "grad_rollout" and s["file"] == "clip_saliency.npy"
    assert ID2LABEL[s["target_class"]] == s["target_label"] == res["predicted_class"]  # absent: the predicted class
    _map(out, s)


def test_inference_saliency_class_picks_the_map(files):
    maps = []
    for t in (0, 1):
        res, out = _run(files, f"class{t}", ["--saliency", "grad_rollout", "--saliency_class", str(t)])
        s = res["saliency"]
        assert s["target_class"] == t and s["target_label"] == ID2LABEL[t]
        maps.append(_map(out, s))
    assert not np.array_equal(maps[0], maps[1])


def test_inference_rollout_keeps_its_keys_and_saliency_class_needs_grad_rollout(files):
    res, out = _run(files, "plain", ["--saliency", "rollout"])
    assert set(res["saliency"]) == SALIENCY_KEYS
    assert set(json.load(open(out / "clip_result.json"))["saliency"]) == SALIENCY_KEYS
    for extra in (["--saliency_class", "1"], ["--saliency", "rollout", "--saliency_class", "1"]):
        with pytest.raises(SystemExit):
            _run(files, "refused", extra)
    with pytest.raises(SystemExit):  # not one of the checkpoint's two labels
        _run(files, "refused", ["--saliency", "grad_rollout", "--saliency_class", "2"])
