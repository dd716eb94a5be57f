"""Timing of ViViT saliency (VivitForVideoClassification.explain) against the plain forward: ViViT-B/16x2,
32 x 224^2, synthetic weights and clips, B = 1 and 4.

  python tools/saliency_time.py [--out profiles/saliency_time.json] [--reps 15] [--warmup 3]

Per batch size, each the median of `--reps` calls between device events after `--warmup` calls:

  forward_ms          the plain eager forward (`forward_logits`, one stream, no graph replay; the last layer
                      for the CLS rows only, as inference runs it);
  forward_full_ms     the same with every layer over every token (cls_only_last_layer = False), the arithmetic
                      explain's forward runs;
  explain_rollout_ms  explain("rollout"): that full forward with the lse-storing attention kernel, the twelve
                      rollout steps, the [B, S] copy to the host and the host normalisation;
  rollout_steps_ms    the twelve ops.attention_rollout_step calls alone, on the buffers explain kept;
  forward_after_ms    the plain forward again at the end: its drift is the margin of the comparison.

The class-specific method, in the same run:

  explain_grad_rollout_ms      explain("grad_rollout", target=0): the activation-keeping forward, the data-gradient
                               chain with a gradient-weighted rollout step per layer, the copy and the host part;
  grad_rollout_steps_ms        the twelve ops.attention_grad_rollout_step calls alone, on the buffers its engine
                               kept (dO is the last one the chain left: the work does not depend on its values);
  grad_rollout_extra_bytes     peak device memory of the first such call above what was allocated before it (the
                               engine's buffers and transposed weights included);
  train_fwd_bwd_ms             one forward plus backward of the train step (every weight gradient, its side
                               streams) on a second model, measured after everything else: what explain should undercut.

The steps' algorithmic work (2 S^2 64 flop and S^2 exp2 per clip, head and layer; twice the flop for the
gradient-weighted step) is recorded with the rate it gives.  A GPU is required: there is no CPU path.

  python tools/saliency_time.py --family timesformer [--out profiles/saliency_time_timesformer.json]

times TimesformerForVideoClassification.explain instead: TimeSformer-B, 8 x 224^2, B = 1, the same medians:
forward_ms, explain_rollout_ms, explain_cls_attention_ms, rollout_steps_ms (the 3 launches per layer alone: the
spatial step's two and the temporal step's one), temporal_steps_ms (the twelve ops.temporal_rollout_step calls
alone), forward_after_ms, and the size of the kept q|k|v and lse buffers.

  python tools/saliency_time.py --family swin [--out profiles/saliency_time_swin.json]

times Swin3d.explain: Swin-T, 32 x 224^2, B = 1, the same medians: forward_ms (the plain eager forward), explain_rollout_ms,
rollout_ms (the 12 ops.window_rollout_step calls and the 3 ops.merge_rollout_spread hops alone, on the q|k|v explain
kept), forward_after_ms, and the size of the kept q|k|v.

  python tools/saliency_time.py --family swin --class_rollout [--out profiles/swin_class_rollout_time.json]

times Swin3d.explain_class instead, at the same size, the same medians: forward_ms, explain_rollout_ms (the class-blind
map, for the ratio), explain_class_ms (the whole call: the train path's forward, the data-gradient chain, the 12
gradient-weighted steps and 3 hops, the copy and the host part), chain_ms (the forward and the chain alone, frozen
masters: no weight gradient formed), chain_with_weight_grads_ms (the same chain with every wgrad GEMM, bias sum and table
reduction run), class_rollout_ms (the 12 ops.window_grad_rollout_step calls, the 3 hops and the 3 adds alone, on the
q|k|v and dO of the last chain), plain_rollout_ms (the 12 ops.window_rollout_step calls and hops on the same q|k|v),
class_rollout_extra_bytes (peak device memory of the first call above what was allocated before it) and forward_after_ms.

  python tools/saliency_time.py --family resnet3d [--out profiles/saliency_time_resnet3d.json]

times ResNet3d.explain: ResNet3D-50, 32 x 224^2, B = 1, the same medians: forward_ms (the plain eager forward), then per
layer (res5, res4) and method (gradcam, hirescam) explain_ms and its ratio to forward_ms of the same process; for res4
also chain_ms (the data-gradient chain alone, on the activations explain kept), the chain's launches by kind (GEMM,
col2im, relu_bwd) with each kind's share of the chain's device time (ops.OpRecorder events around every launch), and
the bytes of the kept activations; forward_after_ms is the plain forward again at the end.

  python tools/saliency_time.py --family lstm [--out profiles/saliency_time_lstm.json]

times VideoResNet50LSTM.explain: ResNet50-LSTM (hidden 256, two layers), 32 x 224^2, B = 1, the same medians: forward_ms
(`model(video)`, the eager inference path), then per layer (res5, res4) and method explain_ms and its ratio to forward_ms of
the same process; bptt_ms (the head's and the recurrence's backward with the two lstm_dx GEMMs and the P = 1 vc_frame_cam,
alone, on what explain kept), for res4 chain_ms (the backbone's data-gradient chain alone), the bytes of the kept backbone
activations, and forward_after_ms.

  python tools/saliency_time.py --family <any of the five> --check [--out profiles/saliency_check_<family>.json]

times the perturbation test that scores such a map (vclip_amd.faithfulness) at the same full sizes, B = 1, the same medians:
forward_ms (`model(clip)`), explain_ms (rollout, or Grad-CAM at res5), faithfulness_zero_ms and faithfulness_blur_ms
(faithfulness(steps=10): 33 forwards, three ops.perturb_clips launches, host ranks and scores; with the blurred baseline
also three blurs), perturb_ms (the one launch that writes the 11 clips, with the bytes it moves) and blur_ms (the two
launches of ops.gaussian_blur_planes), and forward_after_ms.
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

BATCHES = (1, 4)
DEV = "cuda"


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


def timesformer(a) -> dict:
    """TimeSformer-B, 8 x 224^2, B = 1: the plain forward, explain("rollout") and ("cls_attention"), and the rollout's
    launches alone (per layer the spatial step's two and the temporal step's one) on the buffers explain kept"""
    from vclip_amd import ops
    from vclip_amd.build import source_hash
    from vclip_amd.timesformer import create_model
    from vclip_amd.weights import make_synthetic_clips

    model = create_model(num_frames=8, device=DEV).eval()
    c = model.config
    Hn, nl, B = c.num_attention_heads, c.num_hidden_layers, 1
    pix = torch.from_numpy(make_synthetic_clips(B, 8, 224, seed=1)).to(DEV)
    P, T, S, _, _ = model.geometry(B)

    def forward():
        model.forward_logits(pix)

    def explain():
        model.explain(pix, method="rollout")

    def explain_cls():
        model.explain(pix, method="cls_attention")

    r = {"S": S, "P": P, "T": T, "forward_ms": _median(forward, a.reps, a.warmup),
         "explain_rollout_ms": _median(explain, a.reps, a.warmup),
         "explain_cls_attention_ms": _median(explain_cls, a.reps, a.warmup)}
    buf = model._explain_buffers(B, pix.device)  # as the last explain left them
    fa, fb = buf["r_frame"]

    def steps():
        r_f = buf["seed"]
        for li in reversed(range(nl)):
            ops.attention_rollout_step(buf["QKV_s"][li], buf["LSE_s"][li], r_f, B * T, 1 + P, Hn, 0.5, buf["work"], fa)
            ops.temporal_rollout_step(buf["QKV_t"][li], fa, B, P, T, Hn, 0.5, buf["r_clip"], fb if li else None)
            r_f = fb

    def temporal_steps():
        for li in reversed(range(nl)):
            ops.temporal_rollout_step(buf["QKV_t"][li], fa, B, P, T, Hn, 0.5, buf["r_clip"], fb)

    r["rollout_steps_ms"] = _median(steps, a.reps, a.warmup)
    r["temporal_steps_ms"] = _median(temporal_steps, a.reps, a.warmup)
    r["forward_after_ms"] = _median(forward, a.reps, a.warmup)
    r["rollout_launches"] = 3 * nl
    r["kept_qkv_bytes"] = buf["QKV_t"].numel() * 2 + buf["QKV_s"].numel() * 2
    r["kept_lse_bytes"] = buf["LSE_s"].numel() * 4
    # per layer 2 (1+P)^2 64 flop per (frame, head) in the spatial step and 2 T^2 64 per (patch, head) in the temporal one
    r["rollout_steps_flop"] = 2.0 * 64 * Hn * nl * B * (T * (1 + P) ** 2 + P * T * T)
    r["explain_over_forward"] = r["explain_rollout_ms"] / r["forward_ms"]
    print(f"TimeSformer-B B = {B}: forward {r['forward_ms']:.2f} ms (after {r['forward_after_ms']:.2f}), explain(rollout) "
          f"{r['explain_rollout_ms']:.2f} ms, explain(cls_attention) {r['explain_cls_attention_ms']:.2f} ms, "
          f"{3 * nl} rollout launches {r['rollout_steps_ms']:.3f} ms of which {nl} temporal steps "
          f"{r['temporal_steps_ms']:.3f} ms; kept q|k|v {r['kept_qkv_bytes'] / 1e6:.0f} MB + lse "
          f"{r['kept_lse_bytes'] / 1e6:.1f} MB", flush=True)
    return {"model": "TimeSformer-B 8 x 224^2", "reps": a.reps, "warmup": a.warmup, "build": source_hash(),
            "device": torch.cuda.get_device_name(0), "batches": {str(B): r}}


def swin(a) -> dict:
    """Swin-T, 32 x 224^2, B = 1: the plain eager forward, explain("rollout"), and the rollout alone (the 12 block
    steps, three launches each, and the 3 PatchMerging hops) on the q|k|v explain kept"""
    from vclip_amd import ops
    from vclip_amd.build import source_hash
    from vclip_amd.swin3d import create_model
    from vclip_amd.weights import make_synthetic_video

    model = create_model(None, "tiny", num_classes=2, device=DEV).eval()
    c = model.cfg
    B = 1
    video = torch.from_numpy(make_synthetic_video(B, 32, 224, seed=1)).to(DEV)
    grids = model.geometry(B, 32, 224, 224)
    wins = model._block_windows(grids)
    full = tuple(c["window_size"])

    def forward():
        model.forward_logits(video)

    def explain():
        model.explain(video, method="rollout")

    r = {"grids": [list(g) for g in grids], "forward_ms": _median(forward, a.reps, a.warmup),
         "explain_rollout_ms": _median(explain, a.reps, a.warmup)}
    buf = model._explain_buffers(B, grids, video.device)  # as the last explain left them
    pk = model._packed

    def steps():
        r_in = buf["seed"]
        for s in reversed(range(len(grids))):
            blocks = pk["stages"][s]["blocks"]
            for i in reversed(range(len(blocks))):
                window, shift = wins[s][i]
                r_out = buf["r"][s][1] if r_in is buf["r"][s][0] else buf["r"][s][0]
                ops.window_rollout_step(buf["QKV"][s][i], blocks[i]["table"], r_in, B, grids[s], c["num_heads"][s],
                                        window, shift, full, 0.5, buf["work"][s], r_out)
                r_in = r_out
            if s > 0:
                r_in = ops.merge_rollout_spread(r_in, B, grids[s - 1], buf["r"][s - 1][0])

    r["rollout_ms"] = _median(steps, a.reps, a.warmup)
    r["forward_after_ms"] = _median(forward, a.reps, a.warmup)
    nsteps = sum(c["depths"])
    r["rollout_launches"] = 3 * nsteps + len(grids) - 1
    r["kept_qkv_bytes"] = sum(q.numel() * 2 for q in buf["QKV"])
    # per block and pass 2 * 32 flop per (token, key of its window, head); two passes (normaliser, then the column sums)
    flop = 0.0
    for s, (t, h, w) in enumerate(grids):
        for window, _ in wins[s]:
            flop += 2 * 2.0 * 32 * B * t * h * w * window[0] * window[1] * window[2] * c["num_heads"][s]
    r["rollout_flop"] = flop
    r["rollout_tflops"] = flop / (r["rollout_ms"] * 1e-3) / 1e12
    r["rollout_over_forward"] = r["rollout_ms"] / r["forward_ms"]
    r["explain_over_forward"] = r["explain_rollout_ms"] / r["forward_ms"]
    print(f"Swin-T B = {B}: forward {r['forward_ms']:.3f} ms (after {r['forward_after_ms']:.3f}), explain(rollout) "
          f"{r['explain_rollout_ms']:.3f} ms, the rollout alone ({nsteps} steps + {len(grids) - 1} hops, "
          f"{r['rollout_launches']} launches) {r['rollout_ms']:.3f} ms ({r['rollout_tflops']:.1f} TFLOP/s); "
          f"kept q|k|v {r['kept_qkv_bytes'] / 1e6:.0f} MB", flush=True)
    return {"model": "Swin-T 32 x 224^2", "reps": a.reps, "warmup": a.warmup, "build": source_hash(),
            "device": torch.cuda.get_device_name(0), "batches": {str(B): r}}


def swin_class(a) -> dict:
    """Swin-T, 32 x 224^2, B = 1: Swin3d.explain_class whole, its forward + data-gradient chain alone with and without
    the weight-gradient skips, and its 12 gradient-weighted steps alone beside the 12 plain steps on the same q|k|v"""
    from vclip_amd import ops
    from vclip_amd.build import source_hash
    from vclip_amd.swin3d import create_model
    from vclip_amd.weights import make_synthetic_video

    model = create_model(None, "tiny", num_classes=2, device=DEV).eval()
    c = model.cfg
    B = 1
    video = torch.from_numpy(make_synthetic_video(B, 32, 224, seed=1)).to(DEV)
    grids = model.geometry(B, 32, 224, 224)
    wins = model._block_windows(grids)
    full = tuple(c["window_size"])

    def forward():
        model.forward_logits(video)

    def explain():
        model.explain(video, method="rollout")

    def explain_class():
        model.explain_class(video, target=0)

    r = {"grids": [list(g) for g in grids], "forward_ms": _median(forward, a.reps, a.warmup),
         "explain_rollout_ms": _median(explain, a.reps, a.warmup)}
    model._explain_ws = {}  # explain's kept q|k|v must not count as already allocated
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    explain_class()
    torch.cuda.synchronize()
    r["class_rollout_extra_bytes"] = torch.cuda.max_memory_allocated() - base
    r["explain_class_ms"] = _median(explain_class, a.reps, a.warmup)
    kept = {}

    def chain(frozen=True):
        kept["logits"], kept["douts"], kept["qkv"] = model._class_chain(video, [0] * B, frozen=frozen)

    r["chain_ms"] = _median(chain, a.reps, a.warmup)
    r["chain_with_weight_grads_ms"] = _median(lambda: chain(False), a.reps, a.warmup)
    chain()
    buf, pk = model._explain_class_buffers(B, grids, video.device), model._packed

    def class_steps():
        model._class_rollout(buf, pk, kept["qkv"], kept["douts"], B, grids, wins)

    work = [ops.window_rollout_work(B, g, c["num_heads"][s], DEV) for s, g in enumerate(grids)]
    first = [sum(c["depths"][:s]) for s in range(len(grids))]

    def plain_steps():
        r_in = buf["base"][-1]
        for s in reversed(range(len(grids))):
            blocks = pk["stages"][s]["blocks"]
            for i in reversed(range(len(blocks))):
                window, shift = wins[s][i]
                r_out = buf["r"][s][1] if r_in is buf["r"][s][0] else buf["r"][s][0]
                ops.window_rollout_step(kept["qkv"][first[s] + i], blocks[i]["table"], r_in, B, grids[s], c["num_heads"][s],
                                        window, shift, full, 0.5, work[s], r_out)
                r_in = r_out
            if s > 0:
                r_in = ops.merge_rollout_spread(r_in, B, grids[s - 1], buf["r"][s - 1][0])

    r["class_rollout_ms"] = _median(class_steps, a.reps, a.warmup)
    r["plain_rollout_ms"] = _median(plain_steps, a.reps, a.warmup)
    r["forward_after_ms"] = _median(forward, a.reps, a.warmup)
    nsteps = sum(c["depths"])
    r["class_rollout_launches"] = 3 * nsteps + 2 * (len(grids) - 1)
    # per block 2 * 32 flop per (token, key of its window, head) and product: the normaliser's scores, then the column
    # kernel's scores and dP
    flop = 0.0
    for s, (t, h, w) in enumerate(grids):
        for window, _ in wins[s]:
            flop += 3 * 2.0 * 32 * B * t * h * w * window[0] * window[1] * window[2] * c["num_heads"][s]
    r["class_rollout_flop"] = flop
    r["class_rollout_tflops"] = flop / (r["class_rollout_ms"] * 1e-3) / 1e12
    r["grad_step_over_plain_step"] = r["class_rollout_ms"] / r["plain_rollout_ms"]
    r["chain_skip_gain"] = r["chain_with_weight_grads_ms"] / r["chain_ms"]
    r["explain_class_over_forward"] = r["explain_class_ms"] / r["forward_ms"]
    r["explain_class_over_explain_rollout"] = r["explain_class_ms"] / r["explain_rollout_ms"]
    print(f"Swin-T B = {B}: forward {r['forward_ms']:.3f} ms (after {r['forward_after_ms']:.3f}), explain(rollout) "
          f"{r['explain_rollout_ms']:.3f} ms, explain_class {r['explain_class_ms']:.3f} ms; forward + data-gradient chain "
          f"alone {r['chain_ms']:.3f} ms ({r['chain_with_weight_grads_ms']:.3f} ms with the weight gradients formed); the "
          f"{nsteps} gradient-weighted steps + {len(grids) - 1} hops alone {r['class_rollout_ms']:.3f} ms "
          f"({r['class_rollout_tflops']:.1f} TFLOP/s; the plain steps on the same q|k|v {r['plain_rollout_ms']:.3f} ms); peak "
          f"extra memory {r['class_rollout_extra_bytes'] / 1e6:.0f} MB", flush=True)
    return {"model": "Swin-T 32 x 224^2", "reps": a.reps, "warmup": a.warmup, "build": source_hash(),
            "device": torch.cuda.get_device_name(0), "batches": {str(B): r}}


def resnet3d(a) -> dict:
    """ResNet3D-50, 32 x 224^2, B = 1: the plain eager forward, explain at both layers with both methods, and for res4
    the data-gradient chain alone with its launches by kind"""
    from vclip_amd import ops
    from vclip_amd.build import source_hash
    from vclip_amd.resnet3d import create_model
    from vclip_amd.weights import make_synthetic_video

    model = create_model(None, device=DEV).eval()
    B = 1
    video = torch.from_numpy(make_synthetic_video(B, 32, 224, seed=1)).to(DEV)

    def forward():
        model.forward_logits(video)

    r = {"forward_ms": _median(forward, a.reps, a.warmup), "explain": {}}
    for layer in model.EXPLAIN_LAYERS:
        for method in model.EXPLAIN_METHODS:
            def explain():
                model.explain(video, method=method, target=0, layer=layer)

            ms = _median(explain, a.reps, a.warmup)
            r["explain"][f"{layer}.{method}"] = {"explain_ms": ms, "explain_over_forward": ms / r["forward_ms"]}
        buf = model._explain_buffers(B, 32, 224, 224, layer, video.device)  # as the last explain left them
        r["explain"][f"{layer}.kept_bytes"] = buf["kept_bytes"]
    buf = model._explain_buffers(B, 32, 224, 224, "res4", video.device)

    def chain():
        model._explain_chain(buf, B)

    r["res4_chain_ms"] = _median(chain, a.reps, a.warmup)
    rec = ops.OpRecorder()
    with ops.recording(rec):
        for _ in range(a.reps):
            chain()
    torch.cuda.synchronize()
    kinds = {}
    for _, op, e0, e1, _, _ in rec.entries:
        kind = "gemm" if op.startswith("cam.dgrad") else op.split(".", 1)[1]
        k = kinds.setdefault(kind, {"launches": 0, "ms": 0.0})
        k["launches"] += 1
        k["ms"] += e0.elapsed_time(e1)
    total = sum(k["ms"] for k in kinds.values())
    r["res4_chain_launches"] = {kind: {"launches": k["launches"] // a.reps, "ms": k["ms"] / a.reps,
                                       "share_of_chain": k["ms"] / total} for kind, k in kinds.items()}
    r["res4_chain_over_forward"] = r["res4_chain_ms"] / r["forward_ms"]
    r["forward_after_ms"] = _median(forward, a.reps, a.warmup)
    print(f"ResNet3D-50 B = {B}: forward {r['forward_ms']:.3f} ms (after {r['forward_after_ms']:.3f}); "
          + "; ".join(f"explain {k} {v['explain_ms']:.3f} ms ({v['explain_over_forward']:.2f}x)"
                      for k, v in r["explain"].items() if isinstance(v, dict))
          + f"; the res4 chain alone {r['res4_chain_ms']:.3f} ms: "
          + ", ".join(f"{v['launches']} {k} launches {v['share_of_chain']:.0%}" for k, v in r["res4_chain_launches"].items())
          + f"; kept activations {r['explain']['res4.kept_bytes'] / 1e6:.0f} MB (res4), "
          f"{r['explain']['res5.kept_bytes'] / 1e6:.0f} MB (res5)", flush=True)
    return {"model": "ResNet3D-50 32 x 224^2", "reps": a.reps, "warmup": a.warmup, "build": source_hash(),
            "device": torch.cuda.get_device_name(0), "batches": {str(B): r}}


def lstm(a) -> dict:
    """ResNet50-LSTM, 32 x 224^2, B = 1: model(video), explain at both layers with both methods, the recurrence's
    backward alone and, for res4, the backbone's data-gradient chain alone"""
    from vclip_amd import ops
    from vclip_amd.build import source_hash
    from vclip_amd.resnet50_lstm import create_model
    from vclip_amd.weights import make_synthetic_video

    model = create_model(device=DEV).eval()
    B, T = 1, 32
    video = torch.from_numpy(make_synthetic_video(B, T, 224, seed=1)).to(DEV)

    def forward():
        model(video)

    r = {"forward_ms": _median(forward, a.reps, a.warmup), "explain": {}}
    for layer in model.EXPLAIN_LAYERS:
        for method in model.EXPLAIN_METHODS:
            def explain():
                model.explain(video, method=method, target=1, layer=layer)

            ms = _median(explain, a.reps, a.warmup)
            r["explain"][f"{layer}.{method}"] = {"explain_ms": ms, "explain_over_forward": ms / r["forward_ms"]}
        buf = model.backbone._explain_buffers(B, T, 224, 224, layer, video.device)  # as the last explain left them
        r["explain"][f"{layer}.kept_bytes"] = buf["kept_bytes"]
    buf = model.backbone._explain_buffers(B, T, 224, 224, "res4", video.device)
    (ws,), pk, H = model._explain_ws.values(), model._packed, model.hidden  # the one workspace the last explain left

    def bptt():
        model._head_gradient(pk, ws["head"], ws["h_n"][model.layers - 1], [1] * B)
        dh_seq = None
        for l in range(model.layers - 1, -1, -1):
            L = pk["layers"][l]
            ops.lstm_seq_bwd_state(ws["gates"][l], ws["c_seq"][l], B, None, H, L["w_hh"], ws["dpre"], ws["dpb"], dh_seq=dh_seq,
                                   dh_n=ws["head"]["dh"] if dh_seq is None else None, T=T)
            dh_seq = model._lstm_dx(ws["dpb"], L["wt"], ws["g"] if l == 0 else ws["dxh"])
        ops.frame_cam(ws["feat"], ws["g"], B * T, 1, 2048, ws["frame_map"], ws["frame_rel"])

    def chain():
        model.backbone._explain_chain(buf, B)

    r["bptt_ms"] = _median(bptt, a.reps, a.warmup)
    r["res4_chain_ms"] = _median(chain, a.reps, a.warmup)
    r["res4_chain_over_forward"] = r["res4_chain_ms"] / r["forward_ms"]
    r["forward_after_ms"] = _median(forward, a.reps, a.warmup)
    print(f"ResNet50-LSTM B = {B}, T = {T}: forward {r['forward_ms']:.3f} ms (after {r['forward_after_ms']:.3f}); "
          + "; ".join(f"explain {k} {v['explain_ms']:.3f} ms ({v['explain_over_forward']:.2f}x)"
                      for k, v in r["explain"].items() if isinstance(v, dict))
          + f"; head + recurrence backward alone {r['bptt_ms']:.3f} ms, the res4 chain alone {r['res4_chain_ms']:.3f} ms; "
          f"kept activations {r['explain']['res4.kept_bytes'] / 1e6:.0f} MB (res4), "
          f"{r['explain']['res5.kept_bytes'] / 1e6:.0f} MB (res5)", flush=True)
    return {"model": "ResNet50-LSTM 32 x 224^2", "reps": a.reps, "warmup": a.warmup, "build": source_hash(),
            "device": torch.cuda.get_device_name(0), "batches": {str(B): r}}


def check(a) -> dict:
    """--check: the perturbation test of vclip_amd.faithfulness at the family's full size, B = 1, against the plain forward
    and explain of the same process: faithfulness(steps=10) with both baselines, and its two kernels alone"""
    from vclip_amd import ops
    from vclip_amd.build import source_hash
    from vclip_amd.faithfulness import BLUR_KSIZE, BLUR_SIGMA, cell_ranks, faithfulness, step_counts
    from vclip_amd.weights import make_synthetic_clips, make_synthetic_video

    steps, B = 10, 1
    if a.family == "vivit":
        from vclip_amd.vivit import create_model
        name, model, how = "ViViT-B/16x2 32 x 224^2", create_model(num_frames=32, device=DEV), dict(method="rollout")
        clip = make_synthetic_clips(B, 32, 224, seed=1)
    elif a.family == "timesformer":
        from vclip_amd.timesformer import create_model
        name, model, how = "TimeSformer-B 8 x 224^2", create_model(num_frames=8, device=DEV), dict(method="rollout")
        clip = make_synthetic_clips(B, 8, 224, seed=1)
    elif a.family == "swin":
        from vclip_amd.swin3d import create_model
        name, model, how = "Swin-T 32 x 224^2", create_model(None, "tiny", num_classes=2, device=DEV), dict(method="rollout")
        clip = make_synthetic_video(B, 32, 224, seed=1)
    elif a.family == "resnet3d":
        from vclip_amd.resnet3d import create_model
        name, model, how = "ResNet3D-50 32 x 224^2", create_model(None, device=DEV), dict(method="gradcam", layer="res5")
        clip = make_synthetic_video(B, 32, 224, seed=1)
    else:
        from vclip_amd.resnet50_lstm import create_model
        name, model, how = "ResNet50-LSTM 32 x 224^2", create_model(device=DEV), dict(method="gradcam", layer="res5")
        clip = make_synthetic_video(B, 32, 224, seed=1)
    model = model.eval()
    clip = torch.from_numpy(clip).to(DEV)
    layout = "btchw" if a.family in ("vivit", "timesformer") else "bcthw"

    def forward():
        model(pixel_values=clip) if layout == "btchw" else model(clip)

    def explain():
        return model.explain(clip, **how)

    r = {"forward_ms": _median(forward, a.reps, a.warmup), "explain": how, "explain_ms": _median(explain, a.reps, a.warmup)}
    ex = explain()
    grid = tuple(ex.saliency.shape[1:])
    for baseline in ("zero", "blur"):
        def faith():
            faithfulness(model, clip, ex, steps=steps, baseline=baseline)

        r[f"faithfulness_{baseline}_ms"] = _median(faith, a.reps, a.warmup)
    rank = cell_ranks(ex.saliency).to(DEV)
    k = torch.tensor(step_counts(rank.shape[1], steps), dtype=torch.int32, device=DEV)
    out, blurred, work = torch.empty((steps + 1,) + tuple(clip.shape), device=DEV), torch.empty_like(clip), torch.empty_like(clip)

    def perturb():
        ops.perturb_clips(clip, rank, k, grid, layout, "deletion", out=out)

    def blur():
        ops.gaussian_blur_planes(clip, BLUR_KSIZE, BLUR_SIGMA, out=blurred, work=work)

    r["perturb_ms"], r["blur_ms"] = _median(perturb, a.reps, a.warmup), _median(blur, a.reps, a.warmup)
    r["forward_after_ms"] = _median(forward, a.reps, a.warmup)
    r["steps"], r["grid"], r["forwards"] = steps, list(grid), 3 * (steps + 1)
    r["perturb_bytes"] = clip.numel() * 4 * (steps + 2) + rank.numel() * 4  # one read of the clip, steps + 1 writes
    r["perturb_gb_per_s"] = r["perturb_bytes"] / (r["perturb_ms"] * 1e-3) / 1e9
    r["blur_bytes"] = clip.numel() * 4 * 4  # rows: read + write, columns: read + write
    r["blur_gb_per_s"] = r["blur_bytes"] / (r["blur_ms"] * 1e-3) / 1e9
    r["faithfulness_over_forward"] = r["faithfulness_zero_ms"] / r["forward_ms"]
    r["faithfulness_over_explain"] = r["faithfulness_zero_ms"] / r["explain_ms"]
    print(f"{name} B = {B}: forward {r['forward_ms']:.3f} ms (after {r['forward_after_ms']:.3f}), explain({how}) "
          f"{r['explain_ms']:.3f} ms, faithfulness(steps={steps}) {r['faithfulness_zero_ms']:.2f} ms "
          f"({r['faithfulness_over_forward']:.1f} forwards' time for {r['forwards']} forwards), with the blurred baseline "
          f"{r['faithfulness_blur_ms']:.2f} ms; perturb_clips alone {r['perturb_ms']:.3f} ms "
          f"({r['perturb_gb_per_s']:.0f} GB/s), gaussian_blur_planes alone {r['blur_ms']:.3f} ms "
          f"({r['blur_gb_per_s']:.0f} GB/s)", flush=True)
    return {"model": name, "reps": a.reps, "warmup": a.warmup, "build": source_hash(),
            "device": torch.cuda.get_device_name(0), "batches": {str(B): r}}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=("vivit", "timesformer", "swin", "resnet3d", "lstm"), default="vivit")
    ap.add_argument("--check", action="store_true", help="time the perturbation test (vclip_amd.faithfulness) instead")
    ap.add_argument("--class_rollout", action="store_true", help="with --family swin: time Swin3d.explain_class instead")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", f"saliency_check_{a.family}.json" if a.check else
                             "saliency_time.json" if a.family == "vivit" else f"saliency_time_{a.family}.json")
    if a.class_rollout and (a.family != "swin" or a.check):
        ap.error("--class_rollout goes with --family swin, without --check")
    if a.class_rollout and a.out == os.path.join(ROOT, "profiles", "saliency_time_swin.json"):
        a.out = os.path.join(ROOT, "profiles", "swin_class_rollout_time.json")
    if not torch.cuda.is_available():
        raise SystemExit("saliency_time.py needs a GPU")
    if a.check or a.family in ("timesformer", "swin", "resnet3d", "lstm"):
        legs = {"timesformer": timesformer, "swin": swin, "resnet3d": resnet3d, "lstm": lstm}
        res = check(a) if a.check else swin_class(a) if a.class_rollout else legs[a.family](a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"out": a.out}))
        return 0

    from vclip_amd import ops
    from vclip_amd.build import source_hash
    from vclip_amd.vivit import create_model
    from vclip_amd.weights import make_synthetic_clips

    model = create_model(num_frames=32, device=DEV)
    c = model.config
    Hn, nl = c.num_attention_heads, c.num_hidden_layers
    res = {"model": "ViViT-B/16x2 32 x 224^2", "reps": a.reps, "warmup": a.warmup, "build": source_hash(),
           "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in BATCHES:
        pix = torch.from_numpy(make_synthetic_clips(B, 32, 224, seed=1)).to(DEV)
        _, S, _, _ = model.geometry(B)

        def forward():
            model.forward_logits(pix)

        def forward_full():
            model.cls_only_last_layer = False
            try:
                model.forward_logits(pix)
            finally:
                model.cls_only_last_layer = True

        def explain():
            model.explain(pix, method="rollout")

        r = {"S": S, "forward_ms": _median(forward, a.reps, a.warmup),
             "forward_full_ms": _median(forward_full, a.reps, a.warmup),
             "explain_rollout_ms": _median(explain, a.reps, a.warmup)}
        buf = model._explain_buffers(B, pix.device)  # as the last explain left them

        def steps():
            r_in = buf["seed"]
            for k, li in enumerate(reversed(range(nl))):
                r_out = buf["r"][k & 1]
                ops.attention_rollout_step(buf["QKV"][li], buf["LSE"][li], r_in, B, S, Hn, 0.5, buf["work"], r_out)
                r_in = r_out

        r["rollout_steps_ms"] = _median(steps, a.reps, a.warmup)
        r["forward_after_ms"] = _median(forward, a.reps, a.warmup)
        flop, exps = 2.0 * S * S * 64 * Hn * nl * B, 1.0 * S * S * Hn * nl * B
        r["rollout_steps_flop"], r["rollout_steps_exp2"] = flop, exps
        r["rollout_steps_tflops"] = flop / (r["rollout_steps_ms"] * 1e-3) / 1e12
        r["rollout_steps_gexp2_per_s"] = exps / (r["rollout_steps_ms"] * 1e-3) / 1e9
        r["explain_over_forward"] = r["explain_rollout_ms"] / r["forward_ms"]

        def explain_grad():
            model.explain(pix, method="grad_rollout", target=0)

        model._explain_grad = {}  # the other batch size's engine must not count as already allocated
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        explain_grad()
        torch.cuda.synchronize()
        r["grad_rollout_extra_bytes"] = torch.cuda.max_memory_allocated() - base
        r["explain_grad_rollout_ms"] = _median(explain_grad, a.reps, a.warmup)
        eng = model._explain_grad_engine(B, pix.device)  # as the last explain left it

        def grad_steps():
            r_in = eng.seed
            for k, li in enumerate(reversed(range(nl))):
                r_out = eng.r[k & 1]
                ops.attention_grad_rollout_step(eng.QKV[li], eng.dO, eng.LSE[li], r_in, B, S, Hn, 1.0, 1.0, eng.work,
                                                r_out)
                r_in = r_out

        r["grad_rollout_steps_ms"] = _median(grad_steps, a.reps, a.warmup)
        r["grad_rollout_steps_flop"] = 2 * flop
        r["grad_rollout_steps_tflops"] = 2 * flop / (r["grad_rollout_steps_ms"] * 1e-3) / 1e12
        r["grad_rollout_steps_gexp2_per_s"] = exps / (r["grad_rollout_steps_ms"] * 1e-3) / 1e9
        r["grad_step_over_plain_step"] = r["grad_rollout_steps_ms"] / r["rollout_steps_ms"]
        res["batches"][str(B)] = r
        print(f"B = {B}: forward {r['forward_ms']:.2f} ms (after {r['forward_after_ms']:.2f}), full forward "
              f"{r['forward_full_ms']:.2f} ms, explain(rollout) {r['explain_rollout_ms']:.2f} ms, {nl} rollout steps "
              f"{r['rollout_steps_ms']:.2f} ms ({r['rollout_steps_tflops']:.1f} TFLOP/s, "
              f"{r['rollout_steps_gexp2_per_s']:.0f} G exp2/s); explain(grad_rollout) "
              f"{r['explain_grad_rollout_ms']:.2f} ms, {nl} grad-rollout steps {r['grad_rollout_steps_ms']:.2f} ms "
              f"({r['grad_rollout_steps_tflops']:.1f} TFLOP/s), peak extra memory "
              f"{r['grad_rollout_extra_bytes'] / 1e6:.0f} MB", flush=True)
    # the train step's forward + backward, last: it moves its model's parameters into the flat training buffers
    model._explain_grad = {}
    trainee = create_model(num_frames=32, device=DEV).train()
    for B in BATCHES:
        pix = torch.from_numpy(make_synthetic_clips(B, 32, 224, seed=1)).to(DEV)

        def fwd_bwd():
            trainee(pixel_values=pix).logits[:, 0].sum().backward()

        r = res["batches"][str(B)]
        r["train_fwd_bwd_ms"] = _median(fwd_bwd, a.reps, a.warmup)
        r["explain_grad_over_train_fwd_bwd"] = r["explain_grad_rollout_ms"] / r["train_fwd_bwd_ms"]
        print(f"B = {B}: train forward + backward {r['train_fwd_bwd_ms']:.2f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
