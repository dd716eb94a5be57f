"""Timing of RISE saliency (vclip_amd.rise.rise_map) for each family at its benchmark shape, B = 1, synthetic weights
and clips: ViViT-B/16x2 32 x 224^2, TimeSformer-B 8 x 224^2, Swin-T 32 x 224^2, ResNet3D-50 32 x 224^2, ResNet50-LSTM
32 x 224^2.

  python tools/rise_time.py [--family all|vivit|timesformer|swin|resnet3d|lstm] [--masks 4000] [--sweep_masks 512]
                            [--chunks 4,8,16,32,64] [--reps 15] [--warmup 3] [--out profiles/rise_time.json]

Per family:

  sweep            for each `chunk` of --chunks: forward_ms, the median of --reps ordinary eval forwards of `chunk` clips
                   between device events (forward_clips_per_s is the family's own rate at that batch), and rise_ms, the
                   wall time of one rise_map(masks=--sweep_masks, chunk=chunk) after a warm-up call of the same shapes,
                   ending in its copy of the map to the host; masks_per_s from it, and over_forward_rate = masks_per_s /
                   forward_clips_per_s;
  chunk            the smallest swept value whose masks_per_s is within 5 % of the best: the project's rule for a default
                   (the LSTM's --videos_per_batch); vclip_amd.rise.DEFAULT_CHUNK is set from this table;
  rise_map_ms      the wall time of rise_map(masks=--masks, chunk=that chunk);
  outside_forward  1 - (masks / chunk) * forward_ms(chunk) / rise_map_ms: the share of the total not spent in the model's
                   forward (the two kernels, the logits to the host, the host scores, the weights' upload);
  apply_ms         ops.rise_apply alone on `chunk` masks (median), with the bytes it moves (one read of the clip, chunk
                   writes) and the rate they give;
  accumulate_ms    ops.rise_accumulate alone on `chunk` masks (median), and per 4000 masks.

A GPU is required: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
FAMILIES = ("vivit", "timesformer", "swin", "resnet3d", "lstm")


def _time(fn) -> float:
    """one call between device events, in milliseconds"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median(fn, reps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(_time(fn) for _ in range(reps))


def _wall(fn) -> float:
    """one call on the host clock, in milliseconds; fn ends in a copy to the host"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def make(family: str):
    """(name, model in eval mode, clip on the device, layout) at the family's benchmark shape, B = 1"""
    from vclip_amd.weights import make_synthetic_clips, make_synthetic_video
    if family == "vivit":
        from vclip_amd.vivit import create_model
        name, model, clip = "ViViT-B/16x2 32 x 224^2", create_model(num_frames=32, device=DEV), make_synthetic_clips(1, 32, 224, seed=1)
    elif family == "timesformer":
        from vclip_amd.timesformer import create_model
        name, model, clip = "TimeSformer-B 8 x 224^2", create_model(num_frames=8, device=DEV), make_synthetic_clips(1, 8, 224, seed=1)
    elif family == "swin":
        from vclip_amd.swin3d import create_model
        name, model, clip = "Swin-T 32 x 224^2", create_model(None, "tiny", num_classes=2, device=DEV), make_synthetic_video(1, 32, 224, seed=1)
    elif family == "resnet3d":
        from vclip_amd.resnet3d import create_model
        name, model, clip = "ResNet3D-50 32 x 224^2", create_model(None, device=DEV), make_synthetic_video(1, 32, 224, seed=1)
    else:
        from vclip_amd.resnet50_lstm import create_model
        name, model, clip = "ResNet50-LSTM 32 x 224^2", create_model(device=DEV), make_synthetic_video(1, 32, 224, seed=1)
    return name, model.eval(), torch.from_numpy(clip).to(DEV), "btchw" if family in ("vivit", "timesformer") else "bcthw"


def family(a, fam: str) -> dict:
    from vclip_amd import ops
    from vclip_amd.rise import rise_map, rise_masks

    name, model, clip, layout = make(fam)
    T = clip.shape[1] if layout == "btchw" else clip.shape[2]
    H, W = clip.shape[3], clip.shape[4]
    r = {"model": name, "masks": a.masks, "sweep_masks": a.sweep_masks, "sweep": {}}
    with torch.no_grad():
        for chunk in a.chunks:
            batch = clip.expand((chunk,) + tuple(clip.shape[1:])).contiguous()

            def forward():
                model(pixel_values=batch) if layout == "btchw" else model(batch)

            fwd = _median(forward, a.reps, a.warmup)
            del batch
            rise_map(model, clip, target=0, masks=2 * chunk, chunk=chunk)  # the shapes of the timed call, once
            ms = _wall(lambda: rise_map(model, clip, target=0, masks=a.sweep_masks, chunk=chunk))
            s = {"forward_ms": fwd, "forward_clips_per_s": chunk / (fwd * 1e-3), "rise_ms": ms,
                 "masks_per_s": a.sweep_masks / (ms * 1e-3)}
            s["over_forward_rate"] = s["masks_per_s"] / s["forward_clips_per_s"]
            r["sweep"][str(chunk)] = s
            print(f"{name} chunk {chunk}: forward of {chunk} clips {fwd:.2f} ms ({s['forward_clips_per_s']:.0f} clips/s), "
                  f"rise_map({a.sweep_masks} masks) {ms:.0f} ms ({s['masks_per_s']:.0f} masks/s, "
                  f"{s['over_forward_rate']:.2f} of the forward's rate)", flush=True)
            torch.cuda.empty_cache()
        best = max(s["masks_per_s"] for s in r["sweep"].values())
        chunk = min(c for c in a.chunks if r["sweep"][str(c)]["masks_per_s"] >= 0.95 * best)
        r["chunk"] = chunk
        ex = None

        def whole():
            nonlocal ex
            ex = rise_map(model, clip, target=0, masks=a.masks, chunk=chunk)

        r["rise_map_ms"] = _wall(whole)
        fwd = r["sweep"][str(chunk)]["forward_ms"]
        r["outside_forward"] = 1.0 - (a.masks / chunk) * fwd / r["rise_map_ms"]
        r["cells"] = list(ex.cells)
        bits, shifts = (t.to(DEV) for t in rise_masks(T, H, W, ex.cells, 0.5, chunk, 0))
        out = torch.empty((chunk,) + tuple(clip.shape), device=DEV)
        acc = torch.zeros((1, T, H, W), device=DEV)
        w = torch.rand(chunk, 1, device=DEV)
        r["apply_ms"] = _median(lambda: ops.rise_apply(clip, bits, shifts, ex.cells, layout, out=out), a.reps, a.warmup)
        r["accumulate_ms"] = _median(lambda: ops.rise_accumulate(acc, bits, shifts, w, ex.cells), a.reps, a.warmup)
        r["apply_bytes"] = clip.numel() * 4 * (chunk + 1)
        r["apply_gb_per_s"] = r["apply_bytes"] / (r["apply_ms"] * 1e-3) / 1e9
        r["apply_ms_per_4000"] = r["apply_ms"] * 4000 / chunk
        r["accumulate_ms_per_4000"] = r["accumulate_ms"] * 4000 / chunk
    print(f"{name}: chunk {chunk}; rise_map({a.masks} masks) {r['rise_map_ms']:.0f} ms, {r['outside_forward']:.1%} outside the "
          f"forward; rise_apply alone on {chunk} masks {r['apply_ms']:.3f} ms ({r['apply_gb_per_s']:.0f} GB/s), rise_accumulate "
          f"alone {r['accumulate_ms']:.3f} ms", flush=True)
    return r


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=("all",) + FAMILIES, default="all")
    ap.add_argument("--masks", type=int, default=4000)
    ap.add_argument("--sweep_masks", type=int, default=512)
    ap.add_argument("--chunks", type=lambda s: tuple(int(v) for v in s.split(",")), default=(4, 8, 16, 32, 64))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rise_time.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rise_time.py needs a GPU")
    from vclip_amd.build import source_hash
    res = {"reps": a.reps, "warmup": a.warmup, "build": source_hash(), "device": torch.cuda.get_device_name(0), "families": {}}
    for fam in FAMILIES if a.family == "all" else (a.family,):
        res["families"][fam] = family(a, fam)
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # after every family: a later one's failure keeps the earlier numbers
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({"out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
