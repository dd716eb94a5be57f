"""The resnet50-2d-lstm CLI pair end to end on the GPU (vclip_amd.apps run_main("lstm") /
run_inference("lstm")), on a tiny synthetic dataset of raw uint8 clips (.npy) in the reference's
<root>/{train,val,test}/{non_referral,referral}/ layout, 64 x 64 frames:

  main.py       one epoch of the reference loop (BCEWithLogitsLoss(pos_weight), Adam, ReduceLROnPlateau,
                composite selection), the files it writes, a plain state_dict checkpoint;
  main.py       --skip_train --checkpoint_path: evaluation only;
  inference.py  --batch_mode over the test directory with one unreadable clip added, three videos per
                forward_ragged call: one CSV row per good video, the failure row, the summary, and each
                probability against model(clip) of that video run alone (1e-2 on the logit, the model's
                own bound in tests/test_lstm_gpu.py).
"""
import csv
import json
import math
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HISTORY_KEYS = ("train_loss", "val_loss", "train_acc", "val_acc", "train_auroc", "val_auroc")
METRIC_KEYS = ("auroc", "f1_score", "accuracy", "precision", "recall", "confusion_matrix", "class_metrics")
SEQ = 8
# frames per test video: the 20-frame one is shorter than the default 32, the 6-frame one shorter than SEQ
TEST_FRAMES = {"non_referral": (20, 12), "referral": (6, 10)}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd import _lib as L
    L.load()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("lstm_clips")
    rng = np.random.RandomState(0)
    for split, n in (("train", 2), ("val", 1), ("test", 2)):
        for c in ("non_referral", "referral"):
            d = root / split / c
            d.mkdir(parents=True)
            for k in range(n):
                F = TEST_FRAMES[c][k] if split == "test" else 12
                np.save(d / f"{c}_{split}_{k}.npy", rng.randint(0, 256, (F, 64, 64, 3)).astype(np.uint8))
    return root


@pytest.fixture(scope="module")
def trained(dataset, tmp_path_factory):
    """run_main("lstm") once: (metrics, history, experiment dir, model dir)."""
    from vclip_amd.apps import run_main
    out = tmp_path_factory.mktemp("lstm_run")
    m, history, exp = run_main("lstm", ["--data_dir", str(dataset), "--log_dir", str(out / "logs"), "--model_dir",
                                        str(out / "models"), "--epochs", "1", "--batch_size", "2", "--sequence_length",
                                        str(SEQ), "--hidden_size", "32", "--num_layers", "2", "--num_workers", "0"])
    return m, history, Path(exp), out / "models"


def _checkpoint(model_dir):
    cks = sorted(Path(model_dir).glob("model_*.pth"))
    assert len(cks) == 1, cks
    return cks[0]


def test_main_trains_and_writes_the_reference_files(trained):
    m, history, exp, model_dir = trained
    assert exp.parent.name == "logs" and exp.name.startswith("resnet50_lstm_enhanced_")
    assert set(history) == set(HISTORY_KEYS)
    for k in HISTORY_KEYS:
        assert len(history[k]) == 1 and math.isfinite(history[k][0]), (k, history[k])
    saved = json.load(open(exp / "training_history.json"))
    assert saved == history
    cfg = json.load(open(exp / "training_config.json"))
    for k in ("data_dir", "test_dir", "log_dir", "model_dir", "train_sampling", "val_sampling", "test_sampling",
              "loss_weight", "learning_rate", "batch_size", "epochs", "patience", "hidden_size", "num_layers", "dropout",
              "sequence_length"):
        assert k in cfg, k
    assert cfg["hidden_size"] == 32 and cfg["sequence_length"] == SEQ and cfg["loss_weight"] == 0.3
    metrics = json.load(open(exp / "test_metrics.json"))
    assert set(metrics) == set(METRIC_KEYS) and metrics == m
    assert set(metrics["class_metrics"]) == {"non_referral", "referral"}
    assert np.asarray(metrics["confusion_matrix"]).sum() == 4  # the four test videos, none dropped
    # a plain state_dict that a fresh model of the same shape loads strictly
    from vclip_amd.resnet50_lstm import VideoResNet50LSTM
    sd = torch.load(_checkpoint(model_dir), weights_only=True)
    assert all(isinstance(v, torch.Tensor) for v in sd.values()) and "lstm.weight_hh_l1" in sd
    fresh = VideoResNet50LSTM(32, 2, 0.5)
    missing, unexpected = fresh.load_state_dict(sd, strict=True)
    assert not missing and not unexpected


def test_main_skip_train_evaluates_a_checkpoint(dataset, trained, tmp_path):
    from vclip_amd.apps import run_main
    m, history, exp = run_main("lstm", ["--data_dir", str(dataset), "--log_dir", str(tmp_path / "logs"), "--model_dir",
                                        str(tmp_path / "models"), "--skip_train", "--checkpoint_path",
                                        str(_checkpoint(trained[3])), "--batch_size", "2", "--sequence_length", str(SEQ),
                                        "--hidden_size", "32", "--num_workers", "0"])
    assert all(history[k] == [] for k in HISTORY_KEYS)
    assert not (Path(exp) / "training_history.json").exists() and not list((tmp_path / "models").glob("*.pth"))
    assert set(json.load(open(Path(exp) / "test_metrics.json"))) == set(METRIC_KEYS)
    # the same weights on the same deterministic eval clips: the metrics of the training run's evaluation
    assert m == trained[0]


def test_inference_batches_ragged_videos(dataset, trained, tmp_path):
    from vclip_amd import preprocess as pp
    from vclip_amd import sampling
    from vclip_amd.apps import run_inference
    from vclip_amd.resnet50_lstm import VideoResNet50LSTM
    videos = tmp_path / "videos"
    shutil.copytree(dataset / "test", videos)
    (videos / "referral" / "zz_broken.npy").write_bytes(b"\x00 not a clip")
    ck = _checkpoint(trained[3])
    summary = run_inference("lstm", ["--videos_dir", str(videos), "--model_path", str(ck), "--output_dir",
                                     str(tmp_path / "out"), "--batch_mode", "--videos_per_batch", "3",
                                     "--sequence_length", str(SEQ)])
    out = Path(summary["output_dir"])
    assert out.parent == tmp_path / "out" and out.name.startswith("inference_")
    rows = list(csv.DictReader(open(out / "inference_results.csv")))
    assert list(rows[0].keys()) == ["video_path", "prediction", "probability", "sampled_frames", "total_frames",
                                    "frame_indices", "status"]
    assert len(rows) == 4 and all(r["status"] == "success" for r in rows)
    failures = list(csv.DictReader(open(out / "inference_failures.csv")))
    assert len(failures) == 1 and failures[0]["video_path"].endswith("zz_broken.npy")
    assert failures[0]["status"].startswith("error: ")
    saved = json.load(open(out / "inference_summary.json"))
    assert list(saved) == ["total_videos", "successful_predictions", "failed_predictions", "referral_cases",
                           "non_referral_cases", "sampling_method", "sequence_length", "model_path"]
    assert saved["total_videos"] == 5 and saved["successful_predictions"] == 4 and saved["failed_predictions"] == 1
    assert saved["referral_cases"] + saved["non_referral_cases"] == 4
    assert saved["referral_cases"] == sum(r["prediction"] == "referral" for r in rows)
    assert len(list(csv.DictReader(open(out / "inference_summary.csv")))) == 1
    # each probability against the model on that video alone
    model = VideoResNet50LSTM(32, 2, 0.5)
    model.load_state_dict(torch.load(ck, weights_only=True))
    model = model.cuda().eval()
    mean, std = 0.45, 0.225
    for r in rows:
        frames = np.load(r["video_path"])
        total = frames.shape[0]
        idx = sampling.lstm_uniform_sampling(total, SEQ)
        assert int(r["total_frames"]) == total and int(r["sampled_frames"]) == min(SEQ, total) == len(idx)
        assert json.loads(r["frame_indices"]) == [int(i) for i in idx]
        fr = pp.cv2_resize_u8(torch.from_numpy(frames[idx]).cuda(), (224, 224)).float()
        clip = ((fr / 255.0 - mean) / std).permute(3, 0, 1, 2).unsqueeze(0).contiguous()
        logit = float(model(clip)[0, 0])
        p = float(r["probability"])
        got = math.log(p / (1.0 - p))
        print(f"{Path(r['video_path']).name}: {total} frames, logit {got:.5f} in the batch, {logit:.5f} alone")
        assert abs(got - logit) < 1e-2
        assert r["prediction"] == ("referral" if p >= 0.5 else "non_referral")
    short = [r for r in rows if int(r["total_frames"]) == 6]
    assert len(short) == 1 and int(short[0]["sampled_frames"]) == 6
