"""Timing of batched ragged ResNet50-LSTM inference against one video per forward (16 synthetic videos at
224 x 224, hidden 256, two layers).

  python tools/lstm_infer_time.py [--out profiles/lstm_infer_time.json] [--reps 7] [--kernel-reps 50]

Two sets of lengths: all 32 frames, and a mixed set (32 / 20 / 9 in turn).  For each set:

  baseline        `model(video)` one video at a time (B = 1): the path before forward_ragged existed;
  ragged k        `model.forward_ragged` over k videos per call, k = 2, 4, 8, 16;

each a pass over all 16 videos between device events after warm-up, the median of `--reps` passes, reported
as videos/s.  The recurrence kernel's own time is measured apart, on one layer's buffers: the dense kernel at
B = 1 per video summed over the 16 videos, and the ragged kernel per call summed over the calls of a pass
(median of `--kernel-reps` each).  `default_videos_per_batch` is the smallest k within 5 % of the best
measured rate (1 when no k beats the baseline).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, NV, HW = 256, 16, 224
KS = (2, 4, 8, 16)
DEV = "cuda"


def _time(fn) -> float:
    """one call between device events, in microseconds"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def _median(fn, reps: int, warmup: int = 2) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(_time(fn) for _ in range(reps))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_infer_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=50)
    a = ap.parse_args()

    from vclip_amd import ops
    from vclip_amd.build import source_hash
    from vclip_amd.resnet50_lstm import create_model
    from vclip_amd.weights import make_synthetic_video

    model = create_model(H, 2, 0.5, device=DEV).eval()
    frames = torch.from_numpy(make_synthetic_video(1, 32, HW, seed=1)).to(DEV)  # [1, 3, 32, HW, HW]
    w_hh_t = model._pack(torch.device(DEV, 0))["layers"][0]["w_hh_t"]
    res = {"videos": NV, "hidden": H, "frame": HW, "reps": a.reps, "kernel_reps": a.kernel_reps, "build": source_hash(),
           "device": torch.cuda.get_device_name(0), "sets": {}}
    for name, cycle in (("all32", (32,)), ("mixed", (32, 20, 9))):
        lengths = [cycle[i % len(cycle)] for i in range(NV)]
        # every video reuses the same synthetic frames (the timing does not depend on the pixels)
        videos = [frames[:, :, :n].contiguous() for n in lengths]
        groups = {k: [(torch.cat(videos[i:i + k], dim=2), lengths[i:i + k]) for i in range(0, NV, k)] for k in KS}

        def baseline():
            for v in videos:
                model(v)

        def ragged(k):
            for v, ls in groups[k]:
                model.forward_ragged(v, ls)

        # the recurrence kernel alone, on one layer's buffers
        N = sum(lengths)
        pre = torch.randn(N, 4 * H, device=DEV)
        hseq, hlast = torch.empty(N, H, dtype=torch.bfloat16, device=DEV), torch.empty(NV, H, device=DEV)

        def kernel_dense():
            r = 0
            for n in lengths:
                ops.lstm_seq_fwd(pre[r:r + n], 1, n, H, w_hh_t, hseq[r:r + n], hlast)
                r += n

        def kernel_ragged(k):
            r = 0
            for i in range(0, NV, k):
                ls = lengths[i:i + k]
                ops.lstm_seq_fwd_ragged(pre[r:r + sum(ls)], ls, H, w_hh_t, hseq[r:r + sum(ls)], hlast)
                r += sum(ls)

        base_us = _median(baseline, a.reps)
        s = {"lengths": lengths, "frames": N,
             "baseline": {"pass_ms": base_us / 1e3, "videos_per_s": NV / (base_us * 1e-6),
                          "recurrence_us_per_layer": _median(kernel_dense, a.kernel_reps, warmup=5)},
             "ragged": {}}
        for k in KS:
            us = _median(lambda: ragged(k), a.reps)
            s["ragged"][str(k)] = {"pass_ms": us / 1e3, "videos_per_s": NV / (us * 1e-6),
                                   "recurrence_us_per_layer": _median(lambda: kernel_ragged(k), a.kernel_reps, warmup=5)}
        base_end_us = _median(baseline, a.reps)  # the baseline again after the loop: its drift is the margin
        s["baseline"]["pass_ms_after"] = base_end_us / 1e3
        res["sets"][name] = s
        print(f"{name}: baseline {s['baseline']['videos_per_s']:.1f} videos/s ({base_us / 1e3:.2f} ms, after "
              f"{base_end_us / 1e3:.2f} ms; recurrence {s['baseline']['recurrence_us_per_layer']:.0f} us/layer); " +
              "; ".join(f"k={k}: {v['videos_per_s']:.1f} videos/s (recurrence {v['recurrence_us_per_layer']:.0f} us/layer)"
                        for k, v in s["ragged"].items()), flush=True)
    # the smallest batch within 5 % of the best rate, on the set with mixed lengths (what a directory yields)
    m = res["sets"]["mixed"]
    rates = {1: m["baseline"]["videos_per_s"], **{int(k): v["videos_per_s"] for k, v in m["ragged"].items()}}
    best = max(rates.values())
    res["default_videos_per_batch"] = min(k for k, r in rates.items() if r >= 0.95 * best)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"default_videos_per_batch": res["default_videos_per_batch"], "out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
