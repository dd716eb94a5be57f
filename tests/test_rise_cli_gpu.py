"""cli/timesformer/inference.py and cli/videoswintransformer/inference.py --saliency rise on the GPU: a checkpoint with
synthetic weights (reference dict schema) and a raw uint8 .npy clip, as tests/test_window_rollout_cli_gpu.py makes them.
The map is written at pixel resolution [T, H, W] beside the result JSON, whose "saliency" object names the class the
map explains (--saliency_class, the flag these two families have for `rise` only) and the mask setup; the frame indices
are one per time step for every family.  No value of the map is asserted to be good: the weights are synthetic."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TSF = dict(image_size=224, patch_size=16, num_frames=8, num_channels=3, hidden_size=128, num_hidden_layers=2,
           num_attention_heads=2, intermediate_size=256)
FRAMES, NUM_FRAMES, MASKS = 20, 8, 32
TODAY = {"video_path", "predicted_class", "class_id", "confidence", "class_mapping"}
ID2LABEL = {0: "non-referral", 1: "referral"}
KEYS = {"method", "file", "shape", "temporal_importance", "tubelet_frame_indices", "target_class", "target_label", "masks",
        "cells", "keep", "seed"}
RISE = ["--saliency", "rise", "--rise_masks", str(MASKS), "--saliency_class", "1"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd.swin3d import SWIN3D_CONFIGS
    from vclip_amd.timesformer import TimesformerConfig
    from vclip_amd.weights import make_swin3d_weights, make_timesformer_weights
    root = tmp_path_factory.mktemp("rise_cli")
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


def _check_rise(res, out, check=None):
    saved = json.load(open(out / "clip_result.json"))
    assert set(saved) == TODAY | {"saliency"} and saved["saliency"] == res["saliency"]
    s = saved["saliency"]
    assert set(s) == KEYS | ({"faithfulness"} if check else set())
    grid = [NUM_FRAMES, 224, 224]
    assert s["method"] == "rise" and s["file"] == "clip_saliency.npy" and s["shape"] == grid
    assert (s["target_class"], s["target_label"]) == (1, ID2LABEL[1])  # the asked class, whatever the prediction
    assert (s["masks"], s["cells"], s["keep"], s["seed"]) == (MASKS, [1, 7, 7], 0.5, 0)
    sal = np.load(out / s["file"])
    assert sal.dtype == np.float32 and list(sal.shape) == grid
    assert (sal >= 0).all() and abs(float(sal.astype(np.float64).sum()) - 1) < 1e-5
    np.testing.assert_allclose(s["temporal_importance"], sal.sum(axis=(1, 2)), rtol=1e-5)
    assert len(s["tubelet_frame_indices"]) == NUM_FRAMES and all(len(g) == 1 for g in s["tubelet_frame_indices"])
    return s


@pytest.mark.parametrize("fam", ["swin", "timesformer"])
def test_inference_with_rise_writes_the_pixel_map_and_json(files, fam):
    res, out = _run(files, fam, f"{fam}_rise", RISE)
    plain, _ = _run(files, fam, f"{fam}_plain", [])
    assert {k: res[k] for k in TODAY} == plain  # the label and confidence are the ordinary forward's
    s = _check_rise(res, out)
    kept = [g[0] for g in s["tubelet_frame_indices"]]
    assert kept == sorted(kept) and 0 <= kept[0] and kept[-1] < FRAMES
    if fam == "swin":  # the seeding is the same code for every family: checked once, on the smaller checkpoint
        return
    again, out2 = _run(files, fam, f"{fam}_rise_again", RISE)  # seeded: the same map
    assert np.array_equal(np.load(out2 / "clip_saliency.npy"), np.load(out / "clip_saliency.npy"))
    other, out3 = _run(files, fam, f"{fam}_rise_seed", RISE + ["--rise_seed", "5"])
    assert other["saliency"]["seed"] == 5
    assert not np.array_equal(np.load(out3 / "clip_saliency.npy"), np.load(out / "clip_saliency.npy"))


def test_rise_with_saliency_check(files):
    res, out = _run(files, "timesformer", "timesformer_check", RISE + ["--saliency_check", "4"])
    f = _check_rise(res, out, check=True)["faithfulness"]
    assert f["steps"] == 4 and f["target_class"] == 1 and f["baseline"] == "zero"
    N = NUM_FRAMES * 224 * 224  # the faithfulness grid is the pixel grid
    assert f["fractions"] == [(i * N // 4) / N for i in range(5)]
    for k in ("deletion", "insertion", "random_deletion"):
        assert len(f[k]) == 5 and all(0.0 <= v <= 1.0 for v in f[k])


@pytest.mark.parametrize("fam", ["swin", "timesformer"])
def test_saliency_class_still_needs_a_class_specific_method(files, fam):
    with pytest.raises(SystemExit):
        _run(files, fam, f"{fam}_bad", ["--saliency", "rollout", "--saliency_class", "1"])
    with pytest.raises(SystemExit):
        _run(files, fam, f"{fam}_bad2", RISE[:-1] + ["2"])  # not one of the checkpoint's labels
