"""Whole-video streaming inference on the GPU: VideoResNet50LSTM.forward_stream / init_state and the
inference CLI's --stream_chunk.

Model, 64 x 64 frames, three recordings of 5 / 2 / 8 frames fed in rounds of at most 3 frames each
((3, 2, 3), (2, 0, 3), (0, 0, 2)): final and per-frame logits against a CPU fp32 replay of the rounds'
bf16 features (model.last_features, concatenated per recording) through nn.LSTM and the head, and the final
logits against one forward_ragged over all 15 frames, both within 1e-2 (the bound of this model's logits
in tests/test_lstm_gpu.py; equality with forward_ragged is not promised, the GEMM pick depends on the row
count).  Bit for bit: a recording's last frame logit and its returned logit, state=None and init_state, a
recording given length 0 and its previous logit and state, a round replayed from a kept state.

CLI: four .npy videos of 5, 2, 8 and 11 frames plus an unreadable one, --stream_chunk 4 --videos_per_batch 3.
"""
import csv
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from vclip_amd.weights import make_resnet50_lstm_weights, make_synthetic_video

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENGTHS = [5, 2, 8]
CHUNK = 3
TOL = 1e-2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd import _lib
    _lib.load()


@pytest.fixture(scope="module")
def weights():
    return {k: torch.from_numpy(v) for k, v in make_resnet50_lstm_weights(seed=0).items()}


@pytest.fixture(scope="module")
def model(weights):
    from vclip_amd.resnet50_lstm import VideoResNet50LSTM
    m = VideoResNet50LSTM(256, 2, 0.5)
    m.load_state_dict(weights)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def videos():
    return [torch.from_numpy(make_synthetic_video(1, n, 64, seed=11 + i)) for i, n in enumerate(LENGTHS)]


def _rounds(lengths, chunk):
    pos, out = [0] * len(lengths), []
    while any(p < n for p, n in zip(pos, lengths)):
        lens = [min(chunk, n - p) for p, n in zip(pos, lengths)]
        out.append((list(pos), lens))
        pos = [p + k for p, k in zip(pos, lens)]
    return out


@pytest.fixture(scope="module")
def streamed(model, videos):
    """The rounds run once: per round (lens, logits, state, frame logits, bf16 features), all kept."""
    out, state = [], None
    for pos, lens in _rounds(LENGTHS, CHUNK):
        x = torch.cat([v[:, :, p:p + n] for v, p, n in zip(videos, pos, lens) if n], dim=2).to(DEV)
        logits, state, frames = model.forward_stream(x, lens, state, frame_logits=True)
        out.append(dict(x=x, lens=lens, logits=logits, state=state, frames=frames, feats=model.last_features.clone()))
    torch.cuda.synchronize()
    return out


def _per_video(rounds, key):
    """the rows of a per-frame result, regrouped per recording in time order"""
    parts = [[] for _ in LENGTHS]
    for r in rounds:
        at = 0
        for b, n in enumerate(r["lens"]):
            parts[b].append(r[key][at:at + n].cpu())
            at += n
    return [torch.cat(p) for p in parts]


def test_round_shapes_and_state(model, streamed):
    assert [r["lens"] for r in streamed] == [[3, 2, 3], [2, 0, 3], [0, 0, 2]]
    for r in streamed:
        assert tuple(r["logits"].shape) == (3, 1) and r["logits"].dtype == torch.float32
        assert tuple(r["frames"].shape) == (sum(r["lens"]), 1) and r["frames"].dtype == torch.float32
        for t in (r["state"].h, r["state"].c):
            assert tuple(t.shape) == (2, 3, 256) and t.dtype == torch.float32 and t.is_cuda
            assert bool(torch.isfinite(t).all())
    assert len(model.forward_stream(streamed[0]["x"], streamed[0]["lens"])) == 2  # frame_logits off: (logits, state)


def test_stream_matches_fp32_replay_and_forward_ragged(weights, model, videos, streamed):
    lstm = torch.nn.LSTM(2048, 256, num_layers=2, batch_first=True)
    lstm.load_state_dict({k[len("lstm."):]: v for k, v in weights.items() if k.startswith("lstm.")})
    lstm.eval()
    feats = _per_video(streamed, "feats")
    frames = _per_video(streamed, "frames")
    final = streamed[-1]["logits"].cpu()
    e_final = e_frames = 0.0
    with torch.no_grad():
        for b, f in enumerate(feats):
            assert f.shape[0] == LENGTHS[b]
            y, _ = lstm(f.float()[None])
            y = torch.relu(y[0] @ weights["classifier.0.weight"].T + weights["classifier.0.bias"])
            want = y @ weights["classifier.3.weight"].T + weights["classifier.3.bias"]  # [T, 1]: the head on every step
            e_frames = max(e_frames, float((frames[b] - want).abs().max()))
            e_final = max(e_final, float((final[b] - want[-1]).abs().max()))
    ragged = model.forward_ragged(torch.cat(videos, dim=2).to(DEV), LENGTHS).cpu()
    e_ragged = float((final - ragged).abs().max())
    print(f"forward_stream lengths {LENGTHS} chunk {CHUNK} 64^2: final logits vs the fp32 replay {e_final:.2e}, per-frame "
          f"logits vs the replay {e_frames:.2e}, final logits vs one-shot forward_ragged {e_ragged:.2e}")
    assert e_final < TOL and e_frames < TOL
    assert e_ragged < TOL, (final, ragged)


def test_last_frame_logit_is_the_returned_logit(streamed):
    for k, r in enumerate(streamed):
        at = 0
        for b, n in enumerate(r["lens"]):
            at += n
            if n:
                assert torch.equal(r["frames"][at - 1], r["logits"][b]), (k, b)


def test_length_zero_keeps_logit_and_state(streamed):
    for k in (1, 2):
        prev, cur = streamed[k - 1], streamed[k]
        for b, n in enumerate(cur["lens"]):
            same = torch.equal(cur["logits"][b], prev["logits"][b]) and \
                torch.equal(cur["state"].h[:, b], prev["state"].h[:, b]) and torch.equal(cur["state"].c[:, b], prev["state"].c[:, b])
            assert same == (n == 0), (k, b)


def test_none_state_is_init_state_and_a_kept_state_replays(model, streamed):
    first, second = streamed[0], streamed[1]
    st0 = model.init_state(len(LENGTHS))
    logits, state, frames = model.forward_stream(first["x"], first["lens"], st0, frame_logits=True)
    assert torch.equal(logits, first["logits"]) and torch.equal(frames, first["frames"])
    assert torch.equal(state.h, first["state"].h) and torch.equal(state.c, first["state"].c)
    assert not st0.h.any() and not st0.c.any()  # the caller's state is not written
    # round 2 again from the state round 1 returned, after round 3 has run from round 2's
    logits, state, frames = model.forward_stream(second["x"], second["lens"], first["state"], frame_logits=True)
    assert torch.equal(logits, second["logits"]) and torch.equal(frames, second["frames"])
    assert torch.equal(state.h, second["state"].h) and torch.equal(state.c, second["state"].c)
    with pytest.raises(ValueError, match="state"):
        model.forward_stream(first["x"], first["lens"], model.init_state(2))


# ---- the CLI ------------------------------------------------------------------------------------------
CLI_FRAMES = (5, 2, 8, 11)
CLI_CHUNK, CLI_BATCH = 4, 3


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """(videos dir, checkpoint, summary of the --stream_chunk run)"""
    from vclip_amd.apps import run_inference
    root = tmp_path_factory.mktemp("lstm_stream")
    videos = root / "videos"
    videos.mkdir()
    rng = np.random.RandomState(5)
    for k, n in enumerate(CLI_FRAMES):
        np.save(videos / f"v{k}.npy", rng.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8))
    (videos / "zz_broken.npy").write_bytes(b"\x00 not a clip")
    ck = root / "model.pth"
    torch.save({k: torch.from_numpy(v) for k, v in make_resnet50_lstm_weights(seed=3, hidden=32).items()}, ck)
    summary = run_inference("lstm", ["--videos_dir", str(videos), "--model_path", str(ck), "--output_dir", str(root / "out"),
                                     "--batch_mode", "--videos_per_batch", str(CLI_BATCH), "--stream_chunk", str(CLI_CHUNK)])
    return videos, ck, summary


def test_cli_stream_chunk(cli):
    from vclip_amd import apps
    from vclip_amd import preprocess as pp
    videos, ck, summary = cli
    out = Path(summary["output_dir"])
    assert summary["stream_chunk"] == CLI_CHUNK and json.load(open(out / "inference_summary.json"))["stream_chunk"] == CLI_CHUNK
    assert summary["total_videos"] == 5 and summary["successful_predictions"] == 4 and summary["failed_predictions"] == 1
    rows = list(csv.DictReader(open(out / "inference_results.csv")))
    assert list(rows[0].keys()) == ["video_path", "prediction", "probability", "sampled_frames", "total_frames",
                                    "frame_indices", "status"]
    assert len(rows) == 4 and all(r["status"] == "success" and r["frame_indices"] == "all" for r in rows)
    failures = list(csv.DictReader(open(out / "inference_failures.csv")))
    assert len(failures) == 1 and failures[0]["video_path"].endswith("zz_broken.npy")
    assert failures[0]["status"].startswith("error: ")
    # forward_stream by hand over the same groups of videos, in the order the CLI lists them
    listed = apps.lstm_inference_videos(type("A", (), dict(videos_dir=str(videos), single_video=None, batch_mode=True)))
    good = [p for p in listed if not p.endswith("zz_broken.npy")]
    assert [r["video_path"] for r in rows] == good
    model = apps.lstm_model_from_checkpoint(str(ck), torch.device(DEV))
    by_path = {r["video_path"]: r for r in rows}
    for g0 in range(0, len(good), CLI_BATCH):
        group = good[g0:g0 + CLI_BATCH]
        clips = [np.load(p) for p in group]
        state, logits, frame_p = None, None, [[] for _ in group]
        for pos, lens in _rounds([c.shape[0] for c in clips], CLI_CHUNK):
            u8 = np.concatenate([c[p:p + n] for c, p, n in zip(clips, pos, lens) if n])
            x = pp.lstm_inference_preprocess(pp.cv2_resize_u8(torch.from_numpy(u8).to(DEV), (224, 224)))
            logits, state, fl = model.forward_stream(x, lens, state, frame_logits=True)
            fp, at = torch.sigmoid(fl).reshape(-1).tolist(), 0
            for b, n in enumerate(lens):
                frame_p[b].extend(fp[at:at + n])
                at += n
        probs = torch.sigmoid(logits).reshape(-1).tolist()
        for path, clip, p, fp in zip(group, clips, probs, frame_p):
            r = by_path[path]
            total = clip.shape[0]
            assert int(r["total_frames"]) == total == int(r["sampled_frames"])
            assert float(r["probability"]) == p, (path, r["probability"], p)
            assert r["prediction"] == ("referral" if p >= 0.5 else "non_referral")
            per = list(csv.DictReader(open(out / "frame_probabilities" / f"{Path(path).name}.csv")))
            assert list(per[0].keys()) == ["frame", "probability"]
            assert [int(q["frame"]) for q in per] == list(range(total))
            assert [float(q["probability"]) for q in per] == fp
            assert float(per[-1]["probability"]) == float(r["probability"])
            assert all(math.isfinite(float(q["probability"])) for q in per)
    assert len(list((out / "frame_probabilities").glob("*.csv"))) == 4


def test_cli_without_the_flag_writes_no_frame_probabilities(cli, tmp_path):
    from vclip_amd.apps import run_inference
    videos, ck, _ = cli
    summary = run_inference("lstm", ["--videos_dir", str(videos), "--model_path", str(ck), "--output_dir", str(tmp_path / "out"),
                                     "--batch_mode", "--videos_per_batch", str(CLI_BATCH), "--sequence_length", "4"])
    out = Path(summary["output_dir"])
    assert "stream_chunk" not in summary and "stream_chunk" not in json.load(open(out / "inference_summary.json"))
    assert not (out / "frame_probabilities").exists()
    rows = list(csv.DictReader(open(out / "inference_results.csv")))
    assert len(rows) == 4 and all(json.loads(r["frame_indices"]) for r in rows)
