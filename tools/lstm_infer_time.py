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

Every run also times the stateful recurrence kernel (vc_lstm_seq_fwd_state) against the plain kernels at
B = 4, T = 32 (`state_kernel`).  With --stream the batched sets are replaced by the whole-video leg: 4 videos
of 256 frames through one forward_ragged against forward_stream at chunks 16 .. 256, frames/s and peak
memory (the peak includes each call's contiguous copy of its input slice); `default_stream_chunk` is the
smallest chunk within 5 % of the best streaming rate.
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


def state_kernel_leg(ops, w_hh_t, reps: int) -> dict:
    """The stateful recurrence kernel against the plain ones at B = 4, T = 32, hidden 256 on one layer's
    buffers (medians in us): dense and ragged layout, from the zero state (no W_hh product at step 0, like
    the plain kernels) and with a state carried in place (one more step's W_hh stream), with and without
    the f32 h_all rows."""
    B, T = 4, 32
    pre = torch.randn(B * T, 4 * H, device=DEV)
    hseq, hall = torch.empty(B * T, H, dtype=torch.bfloat16, device=DEV), torch.empty(B * T, H, device=DEV)
    hlast, h, c = torch.empty(B, H, device=DEV), torch.zeros(B, H, device=DEV), torch.zeros(B, H, device=DEV)
    lens = [T] * B
    legs = {
        "plain_dense_us": lambda: ops.lstm_seq_fwd(pre, B, T, H, w_hh_t, hseq, hlast),
        "plain_ragged_us": lambda: ops.lstm_seq_fwd_ragged(pre, lens, H, w_hh_t, hseq, hlast),
        "state_dense_zero_us": lambda: ops.lstm_seq_fwd_state(pre, None, H, w_hh_t, hseq, h, c, T=T),
        "state_ragged_zero_us": lambda: ops.lstm_seq_fwd_state(pre, lens, H, w_hh_t, hseq, h, c),
        "state_dense_carried_us": lambda: ops.lstm_seq_fwd_state(pre, None, H, w_hh_t, hseq, h, c, h0=h, c0=c, T=T),
        "state_ragged_carried_us": lambda: ops.lstm_seq_fwd_state(pre, lens, H, w_hh_t, hseq, h, c, h0=h, c0=c),
        "state_ragged_carried_h_all_us": lambda: ops.lstm_seq_fwd_state(pre, lens, H, w_hh_t, hseq, h, c, h0=h, c0=c,
                                                                        h_all=hall),
    }
    r = {"shape": dict(B=B, T=T, hidden=H), "reps": reps}
    for k, fn in legs.items():
        r[k] = _median(fn, reps, warmup=5)
    r["plain_dense_after_us"] = _median(legs["plain_dense_us"], reps, warmup=5)  # again: its drift is the margin
    print("state kernel B=4 T=32 H=256: " + ", ".join(f"{k[:-3]} {v:.1f} us" for k, v in r.items() if k.endswith("_us")),
          flush=True)
    return r


STREAM_VIDEOS, STREAM_FRAMES = 4, 256
STREAM_CHUNKS = (16, 32, 64, 128, 256)


def stream_leg(model, frames, reps: int) -> dict:
    """Whole-video inference over 4 synthetic videos of 256 frames at 224 x 224: one forward_ragged over all
    1024 frames (the only whole-video path before forward_stream; timed again after the loop) against
    forward_stream in lockstep at each chunk size, with the per-frame logits on.  Frames/s from the median
    pass; torch.cuda.max_memory_allocated per leg (reset before it, the model's workspace dropped)."""
    n, lengths = STREAM_VIDEOS * STREAM_FRAMES, [STREAM_FRAMES] * STREAM_VIDEOS
    # every chunk reuses the same 32 synthetic frames (the timing does not depend on the pixels)
    whole = frames.repeat(1, 1, n // frames.shape[2], 1, 1)

    def leg(fn):
        model._ws, model.backbone._ws, model.backbone._ws_used = {}, {}, []  # the cached workspaces of the leg before
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        us = _median(fn, reps, warmup=1)
        return {"pass_ms": us / 1e3, "frames_per_s": n / (us * 1e-6), "max_memory_allocated_MB": torch.cuda.max_memory_allocated() / 2 ** 20}

    def stream(chunk):
        x = whole[:, :, : STREAM_VIDEOS * chunk]
        state = None
        for _ in range(STREAM_FRAMES // chunk):
            _, state, _ = model.forward_stream(x, [chunk] * STREAM_VIDEOS, state, frame_logits=True)

    r = {"videos": STREAM_VIDEOS, "frames_per_video": STREAM_FRAMES, "reps": reps,
         "resident_MB": torch.cuda.memory_allocated() / 2 ** 20, "one_shot_forward_ragged": leg(lambda: model.forward_ragged(whole, lengths)),
         "forward_stream": {str(c): leg(lambda c=c: stream(c)) for c in STREAM_CHUNKS}}
    r["one_shot_forward_ragged_after"] = leg(lambda: model.forward_ragged(whole, lengths))
    best = max(v["frames_per_s"] for v in r["forward_stream"].values())
    r["default_stream_chunk"] = min(int(c) for c, v in r["forward_stream"].items() if v["frames_per_s"] >= 0.95 * best)
    print(f"stream 4 x 256 frames: one shot {r['one_shot_forward_ragged']['frames_per_s']:.0f} frames/s "
          f"({r['one_shot_forward_ragged']['max_memory_allocated_MB']:.0f} MB peak; after "
          f"{r['one_shot_forward_ragged_after']['frames_per_s']:.0f}); " +
          "; ".join(f"chunk {c}: {v['frames_per_s']:.0f} frames/s ({v['max_memory_allocated_MB']:.0f} MB)"
                    for c, v in r["forward_stream"].items()), flush=True)
    return r


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_infer_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--stream", action="store_true",
                    help="the streaming leg instead of the batched sets (default --out profiles/lstm_stream_time.json)")
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
    res["state_kernel"] = state_kernel_leg(ops, w_hh_t, a.kernel_reps)
    if a.stream:
        res["stream"] = stream_leg(model, frames, a.reps)
        del res["sets"], res["videos"]
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "lstm_stream_time.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"default_stream_chunk": res["stream"]["default_stream_chunk"], "out": out}))
        return 0
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
