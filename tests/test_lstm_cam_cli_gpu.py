"""The ResNet50-LSTM inference CLI's --saliency / --saliency_class / --saliency_layer on the GPU: three .npy videos of
5, 2 and 7 frames plus an unreadable one, --videos_per_batch 2, with and without --stream_chunk 3.  The saliency files,
their shapes and sums, the new row fields and CSV columns, and predictions and probabilities identical to the runs
without --saliency."""
import csv
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from vclip_amd.weights import make_resnet50_lstm_weights

pytestmark = pytest.mark.gpu
FRAMES = (5, 2, 7)
SEQ = 4
CHUNK = 3
PLAIN_KEYS = ["video_path", "prediction", "probability", "sampled_frames", "total_frames", "frame_indices", "status"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """{run name: output directory} of the five runs over one directory of videos"""
    from vclip_amd.apps import run_inference
    root = tmp_path_factory.mktemp("lstm_cam_cli")
    videos = root / "videos"
    videos.mkdir()
    rng = np.random.RandomState(7)
    for k, n in enumerate(FRAMES):
        np.save(videos / f"v{k}.npy", rng.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8))
    (videos / "zz_broken.npy").write_bytes(b"\x00 not a clip")
    ck = root / "model.pth"
    torch.save({k: torch.from_numpy(v) for k, v in make_resnet50_lstm_weights(seed=3, hidden=32).items()}, ck)
    runs = {"plain": [], "gradcam": ["--saliency", "gradcam"],
            "res4": ["--saliency", "hirescam", "--saliency_class", "0", "--saliency_layer", "res4"],
            "stream": ["--stream_chunk", str(CHUNK)], "stream_sal": ["--stream_chunk", str(CHUNK), "--saliency", "gradcam"]}
    out = {}
    for name, extra in runs.items():
        s = run_inference("lstm", ["--videos_dir", str(videos), "--model_path", str(ck), "--output_dir", str(root / name),
                                   "--batch_mode", "--videos_per_batch", "2", "--sequence_length", str(SEQ)] + extra)
        assert s["total_videos"] == 4 and s["successful_predictions"] == 3 and s["failed_predictions"] == 1, name
        out[name] = Path(s["output_dir"])
    return out


def rows_of(d):
    return list(csv.DictReader(open(d / "inference_results.csv")))


def same_predictions(a, b):
    assert [(r["video_path"], r["prediction"], r["probability"], r["frame_indices"]) for r in a] == \
           [(r["video_path"], r["prediction"], r["probability"], r["frame_indices"]) for r in b]


@pytest.mark.parametrize("run,hw,cls", [("gradcam", 7, None), ("res4", 14, 0)])
def test_cli_saliency_files_and_rows(cli, run, hw, cls):
    plain, rows = rows_of(cli["plain"]), rows_of(cli[run])
    assert list(plain[0].keys()) == PLAIN_KEYS and not (cli["plain"] / "saliency").exists()
    assert list(rows[0].keys()) == PLAIN_KEYS + ["saliency_file", "saliency_target", "frame_importance"]
    same_predictions(plain, rows)  # explain's logits are forward_ragged's, bit for bit
    assert len(list((cli[run] / "saliency").glob("*.npy"))) == 3
    for r in rows:
        T = min(SEQ, int(r["total_frames"]))
        assert r["saliency_file"] == f"saliency/{Path(r['video_path']).name}.npy"
        sal = np.load(cli[run] / r["saliency_file"])
        assert sal.dtype == np.float32 and sal.shape == (T, hw, hw) and np.isfinite(sal).all() and (sal >= 0).all()
        total = float(sal.astype(np.float64).sum())
        assert abs(total - 1) < 1e-5 or not sal.any(), total  # normalised, or nothing positive at all
        want = cls if cls is not None else int(r["prediction"] == "referral")  # absent: the predicted class
        assert int(r["saliency_target"]) == want
        imp = json.loads(r["frame_importance"])
        assert len(imp) == T == len(json.loads(r["frame_indices"]))
        assert np.allclose(imp, sal.sum(axis=(1, 2)), rtol=0, atol=1e-6)
    failures = list(csv.DictReader(open(cli[run] / "inference_failures.csv")))
    assert len(failures) == 1 and failures[0]["video_path"].endswith("zz_broken.npy") and failures[0]["status"].startswith("error: ")


def test_cli_stream_saliency_columns(cli):
    plain, rows = rows_of(cli["stream"]), rows_of(cli["stream_sal"])
    assert list(plain[0].keys()) == PLAIN_KEYS
    assert list(rows[0].keys()) == PLAIN_KEYS + ["saliency_target"]
    same_predictions(plain, rows)  # the session's push is forward_stream's launches
    assert not (cli["stream_sal"] / "saliency").exists()  # no spatial maps in this mode
    for r in rows:
        name = f"{Path(r['video_path']).name}.csv"
        base = list(csv.DictReader(open(cli["stream"] / "frame_probabilities" / name)))
        per = list(csv.DictReader(open(cli["stream_sal"] / "frame_probabilities" / name)))
        assert list(base[0].keys()) == ["frame", "probability"]
        assert list(per[0].keys()) == ["frame", "probability", "relevance", "importance"]
        assert [(q["frame"], q["probability"]) for q in per] == [(q["frame"], q["probability"]) for q in base]
        assert len(per) == int(r["total_frames"])
        rel = np.array([float(q["relevance"]) for q in per])
        imp = np.array([float(q["importance"]) for q in per])
        assert np.isfinite(rel).all() and rel.any() and (imp >= 0).all()
        pos = np.clip(rel, 0, None)
        want = pos / pos.sum() if pos.sum() > 0 else np.zeros_like(pos)
        assert np.allclose(imp, want, rtol=1e-5, atol=1e-7)
        assert int(r["saliency_target"]) == int(r["prediction"] == "referral")
