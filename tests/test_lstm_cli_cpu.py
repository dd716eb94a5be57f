"""The ResNet50-LSTM application's host pieces (vclip_amd.apps `lstm` family, data_config.lstm): the
parsers against the reference's flags (tests/golden/cli_flags_lstm.json, extracted by
tools/make_cli_flags.py), the ragged entry point's declaration, the dataset scan and sampler, and the
trainer's pos_weight, model selection and learning-rate schedule."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from vclip_amd import apps, sampling

TYPES = {"str": str, "int": int, "float": float}


@pytest.fixture(scope="module")
def ref_flags(golden_dir):
    with open(os.path.join(golden_dir, "cli_flags_lstm.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("script", ["resnet50-2d-lstm/main.py", "resnet50-2d-lstm/inference.py"])
def test_cli_flags_match_reference(ref_flags, script):
    parser = apps.build_parser(apps.FAMILIES["lstm"], inference=script.endswith("inference.py"))
    acts = {a.option_strings[0]: a for a in parser._actions if a.option_strings}
    assert len(ref_flags[script]) == (19 if script.endswith("main.py") else 8)  # main.py:22-62, inference.py:207-223
    for flag, spec in ref_flags[script].items():
        assert flag in acts, (script, flag)
        a = acts[flag]
        if spec.get("action") == "store_true":
            assert a.const is True and a.default is False, (script, flag)
            continue
        if "type" in spec:
            assert a.type is TYPES[spec["type"]], (script, flag)
        assert bool(a.required) == bool(spec.get("required", False)), (script, flag)
        if "default" in spec:
            assert a.default == spec["default"], (script, flag, a.default, spec["default"])
        if "choices" in spec:
            assert sorted(a.choices) == sorted(spec["choices"]), (script, flag)
    if script.endswith("inference.py"):  # the one flag of our own
        assert acts["--videos_per_batch"].type is int and acts["--videos_per_batch"].default >= 1


def test_ragged_entry_point_declared_and_bound():
    import vclip_amd._lib as L
    assert "vc_lstm_seq_fwd_ragged" in L.header_functions()
    argtypes, restype = L.SIGNATURES["vc_lstm_seq_fwd_ragged"]
    assert len(argtypes) == 12 and restype is L.SIGNATURES["vc_lstm_seq_fwd"][1]
    assert len(L.SIGNATURES["vc_lstm_seq_fwd"][0]) == 15  # the dense entry point keeps its signature


def test_ragged_entry_point_validates_before_any_hip_call():
    """Bad shapes return non-zero with a vc_last_error message; the pointers are never dereferenced."""
    import ctypes

    import vclip_amd._lib as L
    from vclip_amd.build import build
    build()
    lib = L.load()
    p = ctypes.c_void_p(64)
    good = dict(pre=p, ldpre=1024, B=3, row0=p, len=p, max_len=8, hidden=256, w=p, hseq=p, ldh=256, hlast=p)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vc_lstm_seq_fwd_ragged(a["pre"], a["ldpre"], a["B"], a["row0"], a["len"], a["max_len"], a["hidden"], a["w"],
                                        a["hseq"], a["ldh"], a["hlast"], None)
        return rc, lib.vc_last_error().decode()

    for name in ("pre", "row0", "len", "w", "hseq", "hlast"):
        rc, msg = call(**{name: None})
        assert rc != 0 and "null" in msg, name
    for kw, word in ((dict(B=0), ">= 1"), (dict(max_len=0), ">= 1"), (dict(hidden=30), "hidden"), (dict(hidden=1028), "hidden"),
                     (dict(ldpre=1023), "stride"), (dict(ldh=255), "stride")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "vc_lstm_seq_fwd_ragged" in msg, (kw, msg)


@pytest.fixture()
def npy_tree(tmp_path):
    """{train,val,test}/{non_referral,referral} of small .npy clips: 3 referral and 5 non_referral train videos."""
    rng = np.random.RandomState(0)
    counts = {"train": (5, 3), "val": (1, 1), "test": (2, 1)}
    for split, (n0, n1) in counts.items():
        for name, n in (("referral", n1), ("non_referral", n0)):  # created referral first: the order is the code's
            d = tmp_path / split / name
            d.mkdir(parents=True)
            for k in range(n):
                np.save(d / f"v{k}.npy", rng.randint(0, 256, (6 + 9 * k, 8, 8, 3)).astype(np.uint8))
    return tmp_path


def test_dataset_scan_order_and_sampler(npy_tree):
    from vclip_amd.data_config import FOLDERS, lstm
    assert FOLDERS["lstm"] is lstm
    log = logging.getLogger("t")
    ds = lstm.VideoDataset(str(npy_tree), split="train", sampling_method="random_window", sequence_length=8, logger=log)
    assert ds.labels == [0] * 5 + [1] * 3 and all(type(v) is int for v in ds.labels)  # dataset.py:41-51
    assert [os.path.basename(os.path.dirname(p)) for p in ds.video_paths] == ["non_referral"] * 5 + ["referral"] * 3
    assert len(ds) == 8 and ds.fps == 30 and ds.sequence_length == 8
    for method in ("uniform", "random", "random_window"):
        ds = lstm.VideoDataset(str(npy_tree), "test", method, 8, logger=log)
        ref = sampling.LstmSampler(8, method, log)
        for total in (6, 8, 33):  # the short branch, the exact length, a long video
            assert ds.get_sampling_indices("x.npy", total) == ref.get_sampling_indices("x.npy", total)
    # the decoded span: [max(0, t0 - 0.01), min(duration, tN + 0.1)] with timestamps index / 30 (dataset.py:192-202)
    from vclip_amd import video_io
    src = video_io.open_video(ds.video_paths[1])  # 15 frames at 30 fps
    assert src.total_frames == 15
    lo, hi = ds._clip_window(src, [3, 5, 9])
    assert lo == pytest.approx(3 / 30 - 0.01) and hi == pytest.approx(9 / 30 + 0.1)
    lo, hi = ds._clip_window(src, [0, 14])
    assert lo == 0 and hi == pytest.approx(15 / 30)
    frames, label = ds.load_span(1)  # host half only: no GPU
    assert frames.dtype == np.uint8 and frames.shape[1:] == (8, 8, 3) and label == 0


def test_pos_weight_formula():
    labels = [0] * 5 + [1] * 3
    n, n1, n0 = 8, 3, 5
    assert apps.lstm_pos_weight(labels) == pytest.approx((n / (2 * n1)) / (n / (2 * n0)) * 1.5)
    assert apps.lstm_pos_weight(labels) == pytest.approx(2.5)
    with pytest.raises(ValueError, match="referral"):
        apps.lstm_pos_weight([0, 0, 0])


def test_composite_model_selection():
    """trainer.py:109-122 with loss_weight 0.3 (AUROC weight 0.7); score = 0.3 * min(best_loss, loss) / loss +
    0.7 * auroc, saved when it exceeds the best score, and best_loss is the loss of the last SAVED epoch:

      epoch  loss  auroc  best_loss before  normalised  score                  best score before  save
      1      1.0   0.60   inf               1.0         0.3 + 0.42  = 0.72     -inf               yes
      2      0.5   0.60   1.0               1.0         0.3 + 0.42  = 0.72     0.72               no (not greater)
      3      2.0   0.90   1.0               0.5         0.15 + 0.63 = 0.78     0.72               yes (best_loss := 2.0)
      4      1.0   0.80   2.0               1.0         0.3 + 0.56  = 0.86     0.78               yes (best_loss := 1.0)
      5      4.0   0.85   1.0               0.25        0.075+0.595 = 0.67     0.86               no
      6      1.0   0.80   1.0               1.0         0.86                   0.86               no

    The early-stopping counter resets on a save and stops at `patience` = 2 consecutive misses (epoch 6)."""
    sel = apps.LstmModelSelector(loss_weight=0.3, patience=2)
    seq = [(1.0, 0.60), (0.5, 0.60), (2.0, 0.90), (1.0, 0.80), (4.0, 0.85), (1.0, 0.80)]
    saves, counters, stops = [], [], []
    for loss, auroc in seq:
        saves.append(sel.update(loss, auroc))
        counters.append(sel.counter)
        stops.append(sel.early_stop)
    assert saves == [True, False, True, True, False, False]
    assert counters == [0, 1, 0, 0, 1, 2]
    assert stops == [False] * 5 + [True]
    assert sel.best_val_loss == 1.0 and sel.best_val_auroc == 0.80
    assert sel.best_composite_score == pytest.approx(0.86)


def test_reduce_lr_on_plateau_halves_project_adamw():
    from vclip_amd.optim import AdamW
    opt = AdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max", factor=0.5, patience=5)
    sched.step(0.7)
    for _ in range(5):  # five non-improving epochs: within the patience
        sched.step(0.6)
        assert opt.param_groups[0]["lr"] == 1e-3
    sched.step(0.6)  # the sixth
    assert opt.param_groups[0]["lr"] == pytest.approx(5e-4)


def test_test_metrics_keys_and_values():
    labels = [0, 0, 1, 1, 1]
    probs = [0.2, 0.7, 0.9, 0.4, 0.6]
    preds = [int(p >= 0.5) for p in probs]
    m = apps.lstm_test_metrics(labels, preds, probs, apps.LSTM_CLASS_NAMES, logging.getLogger("t"))
    assert set(m) == {"auroc", "f1_score", "accuracy", "precision", "recall", "confusion_matrix", "class_metrics"}
    assert m["confusion_matrix"] == [[1, 1], [1, 2]] and m["accuracy"] == pytest.approx(0.6)
    assert m["auroc"] == pytest.approx(4 / 6)  # 4 of the 6 (negative, positive) pairs are ordered
    assert set(m["class_metrics"]) == {"non_referral", "referral"}
    assert m["class_metrics"]["referral"]["recall"] == pytest.approx(2 / 3)
    json.dumps(m)


def test_inference_video_listing(tmp_path):
    for d in ("referral", "non_referral", "other/deep"):
        (tmp_path / d).mkdir(parents=True)
        (tmp_path / d / "a.npy").write_bytes(b"x")
    ns = lambda **k: type("A", (), dict(dict(videos_dir=str(tmp_path), single_video=None, batch_mode=False), **k))  # noqa: E731
    assert len(apps.lstm_inference_videos(ns())) == 2  # the two class folders (inference.py:263-267)
    assert len(apps.lstm_inference_videos(ns(batch_mode=True))) == 3  # recursive (inference.py:257-261)
    assert apps.lstm_inference_videos(ns(single_video=str(tmp_path / "referral" / "a.npy"))) == \
        [str(tmp_path / "referral" / "a.npy")]
    assert apps.lstm_inference_videos(ns(single_video=str(tmp_path / "nope.mp4"))) is None
