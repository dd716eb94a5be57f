"""inference.py --saliency <method> --saliency_check STEPS on the GPU, for ViViT and ResNet3D-50: a checkpoint with
synthetic weights (reference dict schema) and a raw uint8 .npy clip, as tests/test_rollout_cli_gpu.py and
tests/test_gradcam_cli_gpu.py make them.  With the flag the result JSON's "saliency" object gains a "faithfulness" object
whose curves and areas are those of vclip_amd.faithfulness.faithfulness driven by hand on the same clip and map; without
it the JSON has no such key.  No value of a curve is asserted to be good: the weights are synthetic."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VIVIT = dict(image_size=224, num_frames=8, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=128,
             num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, hidden_act="gelu_fast",
             layer_norm_eps=1e-6, qkv_bias=True)
FRAMES, NUM_FRAMES, STEPS = 20, 8, 4
ID2LABEL = {0: "non-referral", 1: "referral"}
SALIENCY = {"vivit": ["--saliency", "grad_rollout"], "resnet3d": ["--saliency", "hirescam", "--saliency_layer", "res4"]}
KEYS = {"steps", "baseline", "target_class", "deletion_auc", "insertion_auc", "random_deletion_auc", "deletion_gain",
        "fractions", "deletion", "insertion", "random_deletion"}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd.resnet3d import RESNET3D_50
    from vclip_amd.vivit import VivitConfig
    from vclip_amd.weights import make_resnet3d_weights, make_vivit_weights
    root = tmp_path_factory.mktemp("faithfulness_cli")
    sd = {k: torch.from_numpy(v) for k, v in make_vivit_weights(VIVIT, seed=0).items()}
    torch.save({"model_state_dict": sd, "config": VivitConfig(**VIVIT, id2label=ID2LABEL).to_dict(), "id2label": ID2LABEL,
                "label2id": {v: k for k, v in ID2LABEL.items()}, "num_frames": NUM_FRAMES}, root / "vivit.pth")
    sd = {k: torch.from_numpy(v) for k, v in make_resnet3d_weights(RESNET3D_50, seed=0).items()}
    torch.save({"model_state_dict": sd, "id2label": ID2LABEL}, root / "resnet3d.pth")
    np.save(root / "clip.npy", np.random.RandomState(0).randint(0, 256, (FRAMES, 224, 224, 3)).astype(np.uint8))
    return root


def _run(files, fam, log, extra):
    from vclip_amd.apps import run_inference
    res = run_inference(fam, ["--video_path", str(files / "clip.npy"), "--model_path", str(files / f"{fam}.pth"),
                              "--log_dir", str(files / log), "--num_frames", str(NUM_FRAMES)] + extra)
    (exp,) = sorted((files / log).iterdir())
    return res, json.load(open(exp / "inference_results" / "clip_result.json"))


def _by_hand(files, fam, saliency):
    """the model, its input and the map as run_inference makes them, then faithfulness() called directly"""
    from vclip_amd import sampling, video_io
    from vclip_amd.apps import FAMILIES
    from vclip_amd.checkpoint import load_reference_checkpoint
    from vclip_amd.faithfulness import faithfulness
    f = FAMILIES[fam]
    ck, sd = load_reference_checkpoint(str(files / f"{fam}.pth"), vivit_keys=fam == "vivit")
    src = video_io.open_video(str(files / "clip.npy"))
    if fam == "vivit":
        from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
        model = VivitForVideoClassification(VivitConfig.from_dict(dict(ck["config"]))).cuda()
        sampler = sampling.VivitSampler(NUM_FRAMES, "uniform")
    else:
        from vclip_amd.resnet3d import create_model
        model = create_model(None, device="cuda")
        sampler = sampling.Resnet3dInferenceSampler(NUM_FRAMES, "uniform", None, fps_of=lambda p: src.fps)
    model.load_state_dict(sd)
    model.eval()
    clip = f.load_clip(src, sampler, str(files / "clip.npy"), NUM_FRAMES)
    x = f.to_model_input(torch.from_numpy(clip).cuda().unsqueeze(0), NUM_FRAMES, div255=True)
    pred = int(f.logits(model, x).argmax(1))
    ex = model.explain(x, method=saliency[1], target=pred, **({"layer": "res4"} if fam == "resnet3d" else {}))
    return pred, faithfulness(model, x, ex, steps=STEPS, target=pred)


@pytest.mark.parametrize("fam", sorted(SALIENCY))
def test_saliency_check_writes_the_faithfulness_object(files, fam):
    res, saved = _run(files, fam, f"{fam}_check", SALIENCY[fam] + ["--saliency_check", str(STEPS)])
    plain, plain_saved = _run(files, fam, f"{fam}_plain", SALIENCY[fam])
    assert "faithfulness" not in plain["saliency"] and "faithfulness" not in plain_saved["saliency"]
    assert {k: v for k, v in saved["saliency"].items() if k != "faithfulness"} == plain_saved["saliency"]
    assert {k: v for k, v in saved.items() if k != "saliency"} == {k: v for k, v in plain_saved.items() if k != "saliency"}
    f = saved["saliency"]["faithfulness"]
    assert f == res["saliency"]["faithfulness"] and set(f) == KEYS
    assert f["steps"] == STEPS and f["baseline"] == "zero" and f["target_class"] == saved["saliency"]["target_class"]
    N = int(np.prod(saved["saliency"]["shape"]))
    assert f["fractions"] == [(i * N // STEPS) / N for i in range(STEPS + 1)]
    for k in ("deletion", "insertion", "random_deletion"):
        assert len(f[k]) == STEPS + 1 and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in f[k])
        trap = sum((f["fractions"][i + 1] - f["fractions"][i]) * (f[k][i + 1] + f[k][i]) / 2.0 for i in range(STEPS))
        assert abs(trap - f[f"{k}_auc"]) < 1e-12
    assert f["deletion_gain"] == f["random_deletion_auc"] - f["deletion_auc"]
    # nothing deleted = everything inserted = the clip itself: the confidence the CLI printed for that class
    if ID2LABEL[f["target_class"]] == saved["predicted_class"]:
        assert abs(f["deletion"][0] - saved["confidence"]) < 1e-2 and abs(f["insertion"][-1] - saved["confidence"]) < 1e-2
    pred, hand = _by_hand(files, fam, SALIENCY[fam])
    assert pred == f["target_class"]
    assert f["deletion_auc"] == float(hand["deletion_auc"][0])
    for k in ("deletion", "insertion", "random_deletion"):
        assert f[k] == [float(v) for v in hand[k].score[0]] and f[f"{k}_auc"] == float(hand[f"{k}_auc"][0])


def test_saliency_check_without_saliency_is_a_parser_error(files):
    for fam in sorted(SALIENCY):
        with pytest.raises(SystemExit):
            _run(files, fam, "bad", ["--saliency_check", "4"])
        with pytest.raises(SystemExit):
            _run(files, fam, "bad0", SALIENCY[fam] + ["--saliency_check", "0"])
