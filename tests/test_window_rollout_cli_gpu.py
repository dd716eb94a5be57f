"""cli/videoswintransformer/inference.py and cli/timesformer/inference.py --saliency on the GPU: a checkpoint with
synthetic weights (reference dict schema) and a raw uint8 .npy clip, as tests/test_rollout_cli_gpu.py makes them for
ViViT.  With the flag the saliency map is written beside the result JSON, which gains a "saliency" object whose
frame indices are grouped by the family's temporal patch (2 for Swin, 1 for TimeSformer); without it the output is
today's, and the label is the same either way."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TSF = dict(image_size=224, patch_size=16, num_frames=8, num_channels=3, hidden_size=128, num_hidden_layers=2,
           num_attention_heads=2, intermediate_size=256)
FRAMES, NUM_FRAMES = 20, 8
TODAY = {"video_path", "predicted_class", "class_id", "confidence", "class_mapping"}
ID2LABEL = {0: "non-referral", 1: "referral"}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd.swin3d import SWIN3D_CONFIGS
    from vclip_amd.timesformer import TimesformerConfig
    from vclip_amd.weights import make_swin3d_weights, make_timesformer_weights
    root = tmp_path_factory.mktemp("saliency_cli")
    sd = {k: torch.from_numpy(v) for k, v in make_timesformer_weights(TSF, seed=0).items()}
    torch.save({"model_state_dict": sd, "config": TimesformerConfig(**TSF, id2label=ID2LABEL).to_dict(),
                "id2label": ID2LABEL, "label2id": {v: k for k, v in ID2LABEL.items()}, "num_frames": NUM_FRAMES},
               root / "timesformer.pth")
    sd = {k: torch.from_numpy(v) for k, v in make_swin3d_weights(dict(SWIN3D_CONFIGS["tiny"], num_classes=2), seed=0).items()}
    torch.save({"model_state_dict": sd, "id2label": ID2LABEL}, root / "swin.pth")
    np.save(root / "clip.npy", np.random.RandomState(0).randint(0, 256, (FRAMES, 224, 224, 3)).astype(np.uint8))
    return root


def _run(files, fam, log, extra):
    from vclip_amd.apps import run_inference
    res = run_inference(fam, ["--video_path", str(files / "clip.npy"), "--model_path", str(files / f"{fam}.pth"),
                              "--log_dir", str(files / log), "--num_frames", str(NUM_FRAMES)] + extra)
    (exp,) = sorted((files / log).iterdir())
    return res, exp / "inference_results"


def _check(files, fam, method, grid, groups):
    res, out = _run(files, fam, f"{fam}_{method}", ["--saliency", method])
    plain, out0 = _run(files, fam, f"{fam}_{method}_plain", [])
    # without the flag: exactly today's keys and no map
    assert set(plain) == TODAY and set(json.load(open(out0 / "clip_result.json"))) == TODAY
    assert [p.name for p in out0.iterdir()] == ["clip_result.json"]
    # with it: the same label and confidence, plus the map and its description
    assert {k: res[k] for k in TODAY} == plain
    saved = json.load(open(out / "clip_result.json"))
    assert set(saved) == TODAY | {"saliency"}
    s = saved["saliency"]
    assert set(s) == {"method", "file", "shape", "temporal_importance", "tubelet_frame_indices"}
    assert s["method"] == method and s["file"] == "clip_saliency.npy" and s["shape"] == grid
    sal = np.load(out / s["file"])
    assert sal.dtype == np.float32 and list(sal.shape) == grid
    assert (sal >= 0).all() and abs(float(sal.astype(np.float64).sum()) - 1) < 1e-5
    assert len(s["temporal_importance"]) == grid[0]
    np.testing.assert_allclose(s["temporal_importance"], sal.sum(axis=(1, 2)), rtol=1e-5)
    assert s["tubelet_frame_indices"] == groups


def test_swin_inference_with_saliency_writes_map_and_json(files):
    from vclip_amd import preprocess, sampling
    idx = sampling.swin_inference_sampling_indices(str(files / "clip.npy"), FRAMES, NUM_FRAMES, "uniform", None,
                                                   fps_of=lambda p: 30.0)
    idx = idx[0] if isinstance(idx, tuple) else idx
    lo, hi = int(min(idx)), int(max(idx))
    kept = [lo + int(i) for i in preprocess.uniform_temporal_subsample_indices(hi - lo + 1, NUM_FRAMES)]
    assert len(kept) == NUM_FRAMES
    _check(files, "swin", "rollout", [NUM_FRAMES // 2, 56, 56], [kept[i:i + 2] for i in range(0, NUM_FRAMES, 2)])


@pytest.mark.parametrize("method", ["rollout", "cls_attention"])
def test_timesformer_inference_with_saliency_writes_map_and_json(files, method):
    from vclip_amd import sampling
    idx = sampling.VivitSampler(NUM_FRAMES, "uniform").get_sampling_indices(str(files / "clip.npy"), FRAMES)
    idx = [int(i) for i in (idx[0] if isinstance(idx, tuple) else idx)]
    _check(files, "timesformer", method, [NUM_FRAMES, 14, 14], [[i] for i in idx])


@pytest.mark.parametrize("fam", ["swin", "timesformer"])
def test_class_specific_flags_are_rejected_by_the_parser(fam):
    from vclip_amd.apps import FAMILIES, build_parser
    base = ["--video_path", "x.npy", "--model_path", "y.pth"]
    p = build_parser(FAMILIES[fam], inference=True, saliency=True)  # the parser run_inference builds
    assert p.parse_args(base).saliency is None
    assert p.parse_args(base + ["--saliency", "rollout"]).saliency == "rollout"
    for extra in (["--saliency", "grad_rollout"], ["--saliency", "rollout", "--saliency_class", "1"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + extra)
    if fam == "swin":  # no CLS token, so no CLS attention row
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--saliency", "cls_attention"])
