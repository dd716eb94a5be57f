"""Timing of the ResNet50-LSTM recurrence kernels at the workload shape (B = 4, T = 32, hidden 256;
layer 0 with Din 2048, layer 1 with Din 256).

  python tools/lstm_time.py [--out profiles/lstm_time.json] [--reps 100] [--no-step]

Device events after warm-up, the median of `--reps` (>= 50) repetitions of each: the forward
(vc_lstm_seq_fwd of libvclip.so), its train variant, the backward kernel (vc_lstm_seq_bwd, full and
last-step-only), the stateful train pair (vc_lstm_seq_fwd_train_state / vc_lstm_seq_bwd_state, dense rows
from the zero state, dh0 / dc0 written) and, unless --no-step, the whole train step (forward, BCE-with-logits loss, backward,
AdamW) at B = 4, T = 32, 224 x 224.  A report without a bar: compare two builds by running it on each.
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

B, T, H = 4, 32, 256
DEV = "cuda"


def _time(fn) -> float:
    """one call between device events, in microseconds"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def _median(fn, reps: int, warmup: int = 10) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(_time(fn) for _ in range(reps))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_time.json"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--no-step", action="store_true", help="skip the whole train step")
    a = ap.parse_args()
    reps = max(50, a.reps)

    from vclip_amd import autograd_ops as A
    from vclip_amd import ops
    from vclip_amd.build import source_hash

    g = torch.Generator().manual_seed(0)
    M = B * T
    k = 1.0 / H ** 0.5
    res = {"shape": dict(B=B, T=T, hidden=H), "reps": reps, "build": source_hash(),
           "device": torch.cuda.get_device_name(0), "layers": {}}
    for name, din in (("l0", 2048), ("l1", 256)):
        w_ih = ((torch.rand(4 * H, din, generator=g) * 2 - 1) * k).to(DEV)
        w_hh = ((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).to(DEV)
        x = torch.randn(256, din, generator=g).bfloat16().to(DEV)  # rows >= M only pad the GEMM tile
        pk = A.pack_lstm_weights(w_ih, w_hh)
        pre = torch.empty(256, 4 * H, device=DEV)
        ops.gemm(x, pk["wb"], torch.zeros(4 * H, device=DEV), "bias_f32", pre)
        z = lambda r, c, dt=torch.float32: torch.zeros(r, c, dtype=dt, device=DEV)  # noqa: E731
        hseq, hlast = z(M, H, torch.bfloat16), z(B, H)
        gates, cseq, hprev = z(M, 4 * H), z(M, H), z(M, H, torch.bfloat16)
        fwd = lambda: ops.lstm_seq_fwd(pre, B, T, H, pk["w_hh_t"], hseq, hlast)  # noqa: E731
        fwd_train = lambda: ops.lstm_seq_fwd(pre, B, T, H, pk["w_hh_t"], hseq, hlast, gates=gates, c_seq=cseq,  # noqa: E731
                                             h_prev=hprev)
        fwd_train()  # the saved state the backward reads
        # the backward: full dh_seq (lower layers) and last step only (top layer)
        dh, dhl = torch.randn(M, H, generator=g).to(DEV), torch.randn(B, H, generator=g).to(DEV)
        dpre, dpb = z(M, 4 * H), z(M, 4 * H, torch.bfloat16)
        r = dict(din=din, fwd_us=_median(fwd, reps), fwd_train_us=_median(fwd_train, reps),
                 bwd_full_us=_median(lambda: ops.lstm_seq_bwd(gates, cseq, B, T, H, pk["w_hh"], dh, dpre, dpb), reps),
                 bwd_last_only_us=_median(lambda: ops.lstm_seq_bwd(gates, cseq, B, T, H, pk["w_hh"], dhl, dpre, dpb,
                                                                    last_only=True), reps))
        # the stateful train pair on the same rows from the zero state (dense layout), dh0 / dc0 asked for:
        # one W_hh product more than the pair above in the backward
        hn, cn, dh0, dc0 = z(B, H), z(B, H), z(B, H), z(B, H)
        r.update(fwd_train_state_us=_median(lambda: ops.lstm_seq_fwd_train_state(
                     pre, None, H, pk["w_hh_t"], hseq, hn, cn, gates, cseq, hprev, T=T), reps),
                 bwd_state_full_us=_median(lambda: ops.lstm_seq_bwd_state(
                     gates, cseq, B, None, H, pk["w_hh"], dpre, dpb, dh_seq=dh, dh0=dh0, dc0=dc0, T=T), reps),
                 bwd_state_last_only_us=_median(lambda: ops.lstm_seq_bwd_state(
                     gates, cseq, B, None, H, pk["w_hh"], dpre, dpb, dh_n=dhl, dh0=dh0, dc0=dc0, T=T), reps))
        res["layers"][name] = r
        print(f"{name} (Din {din}): fwd {r['fwd_us']:.1f} us, train fwd {r['fwd_train_us']:.1f} us, "
              f"bwd {r['bwd_full_us']:.1f} us, bwd last-only {r['bwd_last_only_us']:.1f} us; stateful train fwd "
              f"{r['fwd_train_state_us']:.1f} us, bwd {r['bwd_state_full_us']:.1f} us, bwd last-only "
              f"{r['bwd_state_last_only_us']:.1f} us", flush=True)

    if not a.no_step:
        import torch.nn.functional as F

        from vclip_amd.optim import AdamW
        from vclip_amd.resnet50_lstm import create_model
        from vclip_amd.weights import make_synthetic_video
        model = create_model(H, 2, 0.5, device=DEV).train()
        opt = AdamW([q for q in model.parameters() if q.requires_grad], lr=1e-3, weight_decay=0.0)
        video = torch.from_numpy(make_synthetic_video(B, T, 224, seed=1)).to(DEV)
        labels = torch.tensor([[1.0], [0.0], [1.0], [0.0]], device=DEV)
        pw = torch.tensor([1.5], device=DEV)

        def step():
            opt.zero_grad()
            F.binary_cross_entropy_with_logits(model(video), labels, pos_weight=pw).backward()
            opt.step()

        def tail():  # the same step without the frozen backbone: LSTM + head forward, backward, AdamW
            opt.zero_grad()
            F.binary_cross_entropy_with_logits(model._forward_tail(feats, B, T), labels, pos_weight=pw).backward()
            opt.step()

        res["train_step_ms"] = _median(step, 7, warmup=2) / 1e3
        feats = model.last_features
        res["train_step_lstm_head_ms"] = _median(tail, 20, warmup=3) / 1e3
        model.eval()
        res["eval_forward_ms"] = _median(lambda: model(video), 7, warmup=2) / 1e3
        print(f"train step B={B} T={T} 224^2: {res['train_step_ms']:.2f} ms (LSTM + head + AdamW part "
              f"{res['train_step_lstm_head_ms']:.2f} ms); eval forward {res['eval_forward_ms']:.2f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
