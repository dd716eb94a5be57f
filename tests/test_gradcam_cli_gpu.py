"""cli/resnet50-3d-video/inference.py --saliency on the GPU: a checkpoint with synthetic ResNet3D-50 weights (reference
dict schema) and a raw uint8 .npy clip, as tests/test_window_rollout_cli_gpu.py makes them for Swin.  With the flag the
map is written beside the result JSON, which gains a "saliency" object (one source-frame index per time step, the
layer, the explained class and its label); without it the output is today's, and the label is the same either way."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAMES, NUM_FRAMES = 20, 8
TODAY = {"video_path", "predicted_class", "class_id", "confidence", "class_mapping"}
ID2LABEL = {0: "non-referral", 1: "referral"}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd.resnet3d import RESNET3D_50
    from vclip_amd.weights import make_resnet3d_weights
    root = tmp_path_factory.mktemp("gradcam_cli")
    sd = {k: torch.from_numpy(v) for k, v in make_resnet3d_weights(RESNET3D_50, seed=0).items()}
    torch.save({"model_state_dict": sd, "id2label": ID2LABEL}, root / "resnet3d.pth")
    np.save(root / "clip.npy", np.random.RandomState(0).randint(0, 256, (FRAMES, 224, 224, 3)).astype(np.uint8))
    return root


def _run(files, log, extra):
    """(the result dict, the output directory, the two lines the CLI prints: the prediction and its confidence)"""
    from vclip_amd.apps import run_inference
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        res = run_inference("resnet3d", ["--video_path", str(files / "clip.npy"), "--model_path",
                                         str(files / "resnet3d.pth"), "--log_dir", str(files / log), "--num_frames",
                                         str(NUM_FRAMES)] + extra)
    (exp,) = sorted((files / log).iterdir())
    lines = [ln for ln in printed.getvalue().splitlines() if ln.startswith(("Predicted class:", "Confidence:"))]
    return res, exp / "inference_results", lines


@pytest.fixture(scope="module")
def plain(files):
    res, out, printed = _run(files, "plain", [])
    # without the flag: exactly today's keys and no map
    assert set(res) == TODAY and set(json.load(open(out / "clip_result.json"))) == TODAY
    assert [p.name for p in out.iterdir()] == ["clip_result.json"]
    assert len(printed) == 2 and printed[0] == f"Predicted class: {res['predicted_class']}"
    return res, printed


def _kept_frames(files):
    from vclip_amd import preprocess, sampling
    idx = sampling.Resnet3dInferenceSampler(NUM_FRAMES, "uniform", None, fps_of=lambda p: 30.0).get_sampling_indices(
        str(files / "clip.npy"), FRAMES)[0]
    lo, hi = int(min(idx)), int(max(idx))
    return [[lo + int(i)] for i in preprocess.uniform_temporal_subsample_indices(hi - lo + 1, NUM_FRAMES)]


@pytest.mark.parametrize("extra,method,layer,grid,target", [
    (["--saliency", "hirescam", "--saliency_layer", "res4", "--saliency_class", "1"], "hirescam", "res4", [8, 14, 14], 1),
    (["--saliency", "gradcam"], "gradcam", "res5", [8, 7, 7], None)], ids=["hirescam-res4-class1", "gradcam"])
def test_resnet3d_inference_with_saliency_writes_map_and_json(files, plain, extra, method, layer, grid, target):
    plain, plain_printed = plain
    res, out, printed = _run(files, f"{method}_{layer}", extra)
    assert printed == plain_printed  # the printed prediction is unchanged by the flag
    assert {k: res[k] for k in TODAY} == plain  # the same label and confidence
    saved = json.load(open(out / "clip_result.json"))
    assert set(saved) == TODAY | {"saliency"}
    s = saved["saliency"]
    pred = [k for k, v in ID2LABEL.items() if v == plain["predicted_class"]][0]
    want = pred if target is None else target
    assert s["method"] == method and s["file"] == "clip_saliency.npy" and s["shape"] == grid and s["layer"] == layer
    assert s["target_class"] == want and s["target_label"] == ID2LABEL[want]
    sal = np.load(out / s["file"])
    assert sal.dtype == np.float32 and list(sal.shape) == grid and (sal >= 0).all()
    total = float(sal.astype(np.float64).sum())
    if s.get("empty"):  # the map has nothing positive: documented, and flagged
        assert s["empty"] is True and total == 0.0
        assert set(s) == {"method", "file", "shape", "temporal_importance", "tubelet_frame_indices", "target_class",
                          "target_label", "layer", "empty"}
    else:
        assert abs(total - 1) < 1e-5
        assert set(s) == {"method", "file", "shape", "temporal_importance", "tubelet_frame_indices", "target_class",
                          "target_label", "layer"}
    assert len(s["temporal_importance"]) == grid[0]
    np.testing.assert_allclose(s["temporal_importance"], sal.sum(axis=(1, 2)), rtol=1e-5, atol=1e-12)
    assert s["tubelet_frame_indices"] == _kept_frames(files)


def test_saliency_class_without_saliency_is_a_parser_error(files):
    with pytest.raises(SystemExit):
        _run(files, "bad", ["--saliency_class", "1"])
    with pytest.raises(SystemExit):
        _run(files, "bad2", ["--saliency", "gradcam", "--saliency_class", "2"])  # not one of the checkpoint's labels
