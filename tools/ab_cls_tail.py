"""Interleaved A/B of the ViViT-B headline forward with the last layer run in full (A) and for the CLS
rows only (B, model.cls_only_last_layer; csrc/cls_tail.hip), in one process, in the style of
tools/ab_model_cfg.py: two captured hipGraphs (the attribute is part of the replay key), B = 8 over
2 streams 5 + 3, alternating --rounds times in alternating order.  Also prints max |logit difference|
between the two and each one's error against the HF golden of the same clips
(tests/golden/vivit_b8.json: the bench's clips and weights).

  python tools/ab_cls_tail.py [--rounds 8] [--captures 4] [--streams 2] [--graph 1] [--dtype bf16|fp16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vclip_amd.vivit import create_model  # noqa: E402
from vclip_amd.weights import make_synthetic_clips  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=8)
ap.add_argument("--streams", type=int, default=2)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--captures", type=int, default=1, help="re-capture both graphs this many times")
ap.add_argument("--graph", type=int, default=1)
ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
pix = torch.from_numpy(make_synthetic_clips(a.B, 32, 224, seed=1)).to(dev)
m = create_model(num_frames=32, device=dev)
m.concurrent_streams = a.streams
m.graph_replay = bool(a.graph)
if a.dtype == "fp16":
    m.compute_dtype = torch.float16
names = ("full last layer", "CLS-only last layer")

outs = []
for v in (False, True):
    m.cls_only_last_layer = v
    outs.append(m.forward_logits(pix).clone().cpu().numpy())
print(f"max |logit(CLS-only) - logit(full)| = {np.abs(outs[1] - outs[0]).max():.3e}", flush=True)
if a.B == 8:
    with open(os.path.join(ROOT, "tests", "golden", "vivit_b8.json")) as f:
        ref = np.array(json.load(f)["logits"])
    for n, o in zip(names, outs):
        print(f"{n}: max |logit - HF golden| = {np.abs(o - ref).max():.3e}", flush=True)

# every capture draws (tunes) its own stream set, and sets differ by a few per cent: with
# --captures n both graphs are dropped and captured again n times, and the gain is taken over all captures
caps = ([], [])
for cap in range(a.captures):
    if cap:
        m._graphs.clear()
    res = ([], [])
    for r in range(a.rounds):
        for i in ((0, 1) if r % 2 == 0 else (1, 0)):
            m.cls_only_last_layer = bool(i)
            for _ in range(3):
                m.forward_logits(pix)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                m.forward_logits(pix)
            torch.cuda.synchronize()
            res[i].append((time.perf_counter() - t0) / a.iters * 1e3)
    for i, (n, t) in enumerate(zip(names, res)):
        caps[i].append(float(np.median(t)))
        print(f"capture {cap} {n}: median {np.median(t):.3f} ms/step  min {min(t):.3f}  max {max(t):.3f}  "
              f"({a.B / np.median(t) * 1e3:.1f} clips/s)  rounds {[round(x, 3) for x in t]}", flush=True)
    print(f"capture {cap}: gain (median full / median CLS-only - 1) = {(np.median(res[0]) / np.median(res[1]) - 1.0) * 100:.2f} %; "
          f"spread of the full leg's rounds (max / min - 1) = {(max(res[0]) / min(res[0]) - 1.0) * 100:.2f} %", flush=True)
full, cls = np.array(caps[0]), np.array(caps[1])
print(f"over {a.captures} captures: full {full.mean():.3f} ms ({full.min():.3f}-{full.max():.3f}, {a.B / full.mean() * 1e3:.1f} clips/s), "
      f"CLS-only {cls.mean():.3f} ms ({cls.min():.3f}-{cls.max():.3f}, {a.B / cls.mean() * 1e3:.1f} clips/s); gain of the means "
      f"{(full.mean() / cls.mean() - 1.0) * 100:.2f} %, worst pairing (best full / worst CLS-only - 1) "
      f"{(full.min() / cls.max() - 1.0) * 100:.2f} %; the full leg's own spread across captures {(full.max() / full.min() - 1.0) * 100:.2f} %",
      flush=True)
