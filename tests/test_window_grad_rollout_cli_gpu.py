"""cli/videoswintransformer/inference.py --saliency class_rollout [--saliency_class N] on the GPU: a Swin-T checkpoint
with synthetic weights (reference dict schema) and a raw uint8 .npy clip, as tests/test_window_rollout_cli_gpu.py makes
them.  The map is Swin3d.explain_class's: the result JSON's "saliency" object names the class it explains, the asked
one or the predicted one, two classes give two maps, a class the checkpoint does not have is refused, and
--saliency_check scores the map.  The CLI resizes every clip to 224 x 224, so the map is [T/2, 56, 56]."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAMES, NUM_FRAMES = 20, 8
TODAY = {"video_path", "predicted_class", "class_id", "confidence", "class_mapping"}
ID2LABEL = {0: "non-referral", 1: "referral"}
GRID = [NUM_FRAMES // 2, 56, 56]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd.swin3d import SWIN3D_CONFIGS
    from vclip_amd.weights import make_swin3d_weights
    root = tmp_path_factory.mktemp("class_rollout_cli")
    sd = {k: torch.from_numpy(v) for k, v in make_swin3d_weights(dict(SWIN3D_CONFIGS["tiny"], num_classes=2), seed=0).items()}
    torch.save({"model_state_dict": sd, "id2label": ID2LABEL}, root / "swin.pth")
    np.save(root / "clip.npy", np.random.RandomState(0).randint(0, 256, (FRAMES, 224, 224, 3)).astype(np.uint8))
    return root


def _run(files, log, extra):
    from vclip_amd.apps import run_inference
    res = run_inference("swin", ["--video_path", str(files / "clip.npy"), "--model_path", str(files / "swin.pth"),
                                 "--log_dir", str(files / log), "--num_frames", str(NUM_FRAMES)] + extra)
    (exp,) = sorted((files / log).iterdir())
    return res, exp / "inference_results"


def _map(out, s):
    sal = np.load(out / s["file"])
    assert s["file"] == "clip_saliency.npy" and s["shape"] == GRID
    assert sal.dtype == np.float32 and list(sal.shape) == GRID
    assert (sal >= 0).all() and abs(float(sal.astype(np.float64).sum()) - 1) < 1e-5
    np.testing.assert_allclose(s["temporal_importance"], sal.sum(axis=(1, 2)), rtol=1e-5)
    assert len(s["tubelet_frame_indices"]) == GRID[0] and all(len(g) == 2 for g in s["tubelet_frame_indices"])
    return sal


@pytest.fixture(scope="module")
def runs(files):
    """the CLI once without --saliency_class and once per class"""
    return {c: _run(files, f"class_{c}", ["--saliency", "class_rollout"] + ([] if c is None else ["--saliency_class", str(c)]))
            for c in (None, 0, 1)}


def test_class_rollout_names_the_predicted_class(files, runs):
    res, out = runs[None]
    saved = json.load(open(out / "clip_result.json"))
    assert set(saved) == TODAY | {"saliency"}
    s = saved["saliency"]
    assert set(s) == {"method", "file", "shape", "temporal_importance", "tubelet_frame_indices", "target_class", "target_label"}
    assert s["method"] == "class_rollout"
    pred = {v: k for k, v in ID2LABEL.items()}[saved["predicted_class"]]
    assert s["target_class"] == pred and s["target_label"] == saved["predicted_class"]
    sal = _map(out, s)
    # the same map as asking for that class by number
    res_c, out_c = runs[pred]
    np.testing.assert_array_equal(sal, np.load(out_c / "clip_saliency.npy"))


def test_saliency_class_picks_the_class_and_the_maps_differ(files, runs):
    maps = {}
    for c in (0, 1):
        res, out = runs[c]
        s = json.load(open(out / "clip_result.json"))["saliency"]
        assert s["method"] == "class_rollout" and s["target_class"] == c and s["target_label"] == ID2LABEL[c]
        maps[c] = _map(out, s)
        assert {k: res[k] for k in TODAY} == {k: runs[None][0][k] for k in TODAY}  # the label does not depend on the flag
    e = float(np.abs(maps[1].astype(np.float64) - maps[0]).max() / maps[0].max())  # E of the model tests
    print(f"E between the class-0 and class-1 maps of the Swin-T checkpoint: {e:.3f}")
    assert e > 0.15  # measured 0.343 on this checkpoint and clip; a class-blind map would give 0


def test_a_class_the_checkpoint_lacks_is_refused(files):
    with pytest.raises(SystemExit):
        _run(files, "class_2", ["--saliency", "class_rollout", "--saliency_class", "2"])


def test_saliency_check_scores_the_class_map(files):
    res, out = _run(files, "check", ["--saliency", "class_rollout", "--saliency_class", "1", "--saliency_check", "4"])
    s = json.load(open(out / "clip_result.json"))["saliency"]
    f = s["faithfulness"]
    assert f["steps"] == 4 and f["target_class"] == 1 and len(f["deletion"]) == 5 and len(f["insertion"]) == 5
    assert all(np.isfinite(f[k]) for k in ("deletion_auc", "insertion_auc", "random_deletion_auc", "deletion_gain"))
