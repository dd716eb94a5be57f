"""CPU-side checks of bench.py's command line and of what a plain run writes: --full and
--dump-outputs exist, the plain record carries the headline fields, and --dump-outputs writes
float32 / float64 .npy files bounded by DUMP_LIMIT_BYTES with a sample that repeats from run to run."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_headline_record_fields():
    a = argparse.Namespace(batch=8, steps=4, warmup=1)
    rec = bench.headline_record(a, 1, "clips/sec fwd ViViT-B 32x224^2 bf16", 0.032, "synthetic", {"streams": 2})
    assert rec["value"] == 1000.0 and rec["ms_per_step"] == 8.0 and rec["steps"] == 4 and rec["warmup"] == 1
    assert rec["unit"] == "clips/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["metric"] == "clips/sec fwd ViViT-B 32x224^2 bf16" and rec["n_gpus"] == 1
    assert rec["build"] == bench._build_id()


def test_dump_outputs_dtypes_and_names(tmp_path):
    logits = torch.arange(16, dtype=torch.float32).reshape(8, 2)
    bench.dump_outputs(str(tmp_path / "d"), {"logits": logits, "half": logits.to(torch.bfloat16).to(torch.float16),
                                             "wide": logits.double()})
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in ("logits", "half", "wide")}
    assert got["logits"].dtype == np.float32 and got["half"].dtype == np.float32 and got["wide"].dtype == np.float64
    for v in got.values():
        assert v.shape == (8, 2) and np.array_equal(v, logits.numpy())
    bench.dump_outputs(str(tmp_path / "r"), {"logits": logits}, rank=1, world=2)
    assert os.listdir(tmp_path / "r") == ["logits_rank1.npy"]


def test_dump_outputs_bounded_repeatable_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = np.arange(5000, dtype=np.float32)
    small = np.arange(10, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(a, b) and a.size == 512 and np.all(np.diff(a) > 0)  # a sorted subset, the same twice
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 4096 + 2 * 128
