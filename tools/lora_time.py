"""What LoRA fine-tuning (vclip_amd.lora) gains over the full fine-tune step: ViViT-B/16x2 at 32 x 224^2, B = 4,
seeded synthetic weights and clips, the reference's train step (zero_grad, forward, CrossEntropyLoss, backward,
vclip_amd.optim.AdamW.step) in one process.

  python tools/lora_time.py [--batch 4] [--rank 8] [--rounds 8] [--seconds 1.5] [--out profiles/lora_time.json]

Legs: `full` (no adapters: every weight trains, the step of vivit_train.TrainEngine.backward), `lora_qv` (q, v on
every layer), `lora_all6` (q, k, v, o, fc1, fc2 on every layer), `lora_qv_last4` (q, v on the last 4 layers), all at
--rank.  Each leg is built and warmed up on its own (its peak of torch.cuda.max_memory_allocated over the build and
the warm-up steps, less what was allocated before, is recorded there); then the legs alternate for --rounds rounds,
each round timing a run of steps of each leg between device events, at least --seconds per leg in all.  ms_per_step is
the median over the rounds, with their min and max.  Last, each LoRA leg runs 3 steps under ops.OpRecorder: the
time of the two adapter-gradient kernels per step beside the time their algorithmic bytes take at the HBM peak
(8 TB/s).  Those launches run on the side stream beside the data-gradient chain, so their event times include what
they share with it.

A GPU is required: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
HBM_PEAK = 8e12
VIVIT_B = dict(image_size=224, num_frames=32, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=768,
               num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu_fast",
               layer_norm_eps=1e-6, qkv_bias=True)
ALL6 = ("q", "k", "v", "o", "fc1", "fc2")


def legs(rank: int) -> dict:
    return {"full": None,
            "lora_qv": dict(rank=rank, alpha=2.0 * rank, targets=("q", "v")),
            "lora_all6": dict(rank=rank, alpha=2.0 * rank, targets=ALL6),
            "lora_qv_last4": dict(rank=rank, alpha=2.0 * rank, targets=("q", "v"), layers=4)}


class Leg:
    def __init__(self, name, cfg, lora_kw, x, y, warmup):
        from vclip_amd import lora
        from vclip_amd.optim import AdamW
        from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
        from vclip_amd.weights import make_vivit_weights
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        model = VivitForVideoClassification(VivitConfig(**cfg, id2label={0: "non-referral", 1: "referral"}))
        model.load_state_dict(make_vivit_weights(cfg, seed=0))
        self.model = model.to(DEV).train()
        if lora_kw is not None:
            lora.attach(self.model, **lora_kw)
        self.name, self.x, self.y = name, x, y
        self.trainable = sum(p.numel() for p in self.model.parameters() if p.requires_grad)
        self.opt = AdamW([p for p in self.model.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.01)
        self.crit = torch.nn.CrossEntropyLoss()
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()
        self.peak_bytes = torch.cuda.max_memory_allocated() - before
        self.held_bytes = torch.cuda.memory_allocated() - before

    def step(self):
        self.opt.zero_grad()
        loss = self.crit(self.model(pixel_values=self.x).logits, self.y)
        loss.backward()
        self.opt.step()
        return loss

    def run(self, n: int) -> float:
        """n steps between device events: milliseconds per step"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            self.step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.5, help="timed seconds per leg, over all rounds (at least)")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--layers", type=int, default=12, help="encoder layers (12: ViViT-B; fewer for a rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_time.py needs a GPU")
    from vclip_amd import ops
    from vclip_amd.build import source_hash
    from vclip_amd.weights import make_synthetic_clips
    cfg = dict(VIVIT_B, num_hidden_layers=a.layers)
    x = torch.from_numpy(make_synthetic_clips(a.batch, cfg["num_frames"], cfg["image_size"], seed=1)).to(DEV)
    y = torch.arange(a.batch, device=DEV) % 2
    res = {"model": f"ViViT-B/16x2 32 x 224^2, {a.layers} layers", "batch": a.batch, "rank": a.rank, "rounds": a.rounds,
           "build": source_hash(), "device": torch.cuda.get_device_name(0), "legs": {}}
    built = {}
    for name, kw in legs(a.rank).items():
        if kw is not None and "layers" in kw:
            kw = dict(kw, layers=min(kw["layers"], a.layers))
        built[name] = Leg(name, cfg, kw, x, y, a.warmup)
        print(f"{name}: {built[name].trainable} trainable parameters, peak {built[name].peak_bytes / 2 ** 20:.0f} MiB",
              flush=True)
    # alternate the legs: every round times one run of each
    first = {n: leg.run(3) for n, leg in built.items()}
    per_round = {n: max(3, math.ceil(a.seconds * 1e3 / a.rounds / ms)) for n, ms in first.items()}
    times = {n: [] for n in built}
    for _ in range(a.rounds):
        for n, leg in built.items():
            times[n].append(leg.run(per_round[n]))
    full = statistics.median(times["full"])
    for n, leg in built.items():
        ms = statistics.median(times[n])
        res["legs"][n] = {"trainable_parameters": leg.trainable, "ms_per_step": ms, "ms_min": min(times[n]),
                          "ms_max": max(times[n]), "rounds_ms": times[n], "steps_per_round": per_round[n],
                          "timed_seconds": sum(times[n]) * per_round[n] * 1e-3, "clips_per_s": a.batch / (ms * 1e-3),
                          "speedup_over_full": full / ms, "peak_bytes": leg.peak_bytes, "held_bytes": leg.held_bytes}
        print(f"{n}: {ms:.2f} ms/step (min {min(times[n]):.2f}, max {max(times[n]):.2f} over {a.rounds} rounds of "
              f"{per_round[n]} steps), {full / ms:.3f}x the full step's rate", flush=True)
    # the adapter-gradient kernels under the op recorder (and where the rest of the step goes)
    for n, leg in built.items():
        if n == "full":
            continue
        rec = ops.OpRecorder()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with ops.recording(rec):
            e0.record()
            for _ in range(3):
                leg.step()
            e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        step_ms = e0.elapsed_time(e1) / 3
        byop = rec.summary_ops(3, step_ms)
        kern = {}
        for op in ("lora_down", "lora_wgrad"):
            nbytes = sum(w for _, o, _, _, w, _ in rec.entries if o == op) / 3
            kern[op] = dict(byop[op], bytes_per_step=nbytes, hbm_bound_ms_per_step=nbytes / HBM_PEAK * 1e3)
        res["legs"][n]["recorded_step_ms"] = step_ms
        res["legs"][n]["adapter_kernels"] = kern
        res["legs"][n]["recorded_ops"] = {k: {"ms_per_step": v["ms_per_step"], "launches_per_step": v["launches_per_step"]}
                                          for k, v in byop.items()}
        print(f"{n}: recorded step {step_ms:.2f} ms; " + "; ".join(
            f"{op} {k['ms_per_step']:.3f} ms/step in {k['launches_per_step']:.0f} launches (bytes at the HBM peak: "
            f"{k['hbm_bound_ms_per_step']:.3f} ms)" for op, k in kern.items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
