"""References for ResNet3d.explain (Grad-CAM / HiResCAM), CPU only:

  autograd_cam  the maps from plain autograd through oracle/resnet3d_ref.py (the yardstick of the GPU test, and with
                `rounding` the same graph at a bf16 implementation's storage precisions);
  chain_cam     the rules ResNet3d._explain_chain implements -- the closed-form seed of the head, the ReLU masks, the
                skip join, the transposed convolutions with BatchNorm folded -- written by hand in fp64 on the
                oracle's tensors, each rule switchable off (`drop`) so a test can show that a wrong rule is visible;
  E             max|x - ref| / max|ref| per clip on the signed maps.

Both return signed maps [B, T, H_l, W_l] (no ReLU)."""
import torch
import torch.nn.functional as F

from oracle import resnet3d_ref as ref

# every structural feature of the 50-layer net (tests/test_resnet3d_train_gpu.py's SMALL): branch1 on each stage,
# stride 2, (3,1,1) conv_a, an identity-skip block in res5
SMALL = dict(depths=(2, 1, 1, 2), stem_dim=64, conv_a_kernels=((1, 1, 1), (1, 1, 1), (3, 1, 1), (3, 1, 1)),
             spatial_strides=(1, 2, 2, 2), head_pool=(2, 2, 2), num_classes=2, bn_eps=1e-5)
FIXTURES = ((2, 8, 64, 2), (2, 6, 96, 3))  # make_synthetic_video(B, T, HW, seed); the second ends on a 3 x 3 map
LAYERS = {"res5": 4, "res4": 3}  # index into resnet3d_forward(..., return_stages=True)[1]
METHODS = ("gradcam", "hirescam")
DROPS = ("mask_out", "mask_b", "mask_a", "join", "cnt")
BF16 = {"act": lambda t: t.bfloat16().to(t.dtype), "weight": lambda t: t.bfloat16().to(t.dtype)}

# E(gpu) / E(bf16 oracle) of the signed maps, measured on an MI355X (tests/test_gradcam_gpu.py prints them), in the order
# of test_explain_matches_autograd's loops: fixture, layer (res5, res4), method, target, clip
MEASURED_RATIOS = (1.59, 1.07, 0.52, 0.97, 2.06, 1.23, 0.60, 0.97, 1.47, 0.68, 1.46, 0.76, 0.89, 0.67, 0.89, 1.16,
                   1.15, 1.51, 0.73, 1.01, 0.87, 2.94, 0.61, 0.84, 1.18, 1.68, 0.94, 0.90, 0.84, 0.82, 0.61, 1.02)
# the smallest power of two that is at least twice the largest measured ratio (2 x 2.94 = 5.9)
MODEL_FACTOR = 8
# Half of the smallest wrong-rule E of each case (fixture, layer, method, target, clip), rounded down to two digits;
# tests/test_gradcam_cpu.py recomputes and checks every entry.  MODEL_FACTOR x the bf16 yardstick alone exceeds it in
# every res4 case (the yardstick is 5e-3 to 5e-2 there and a dropped conv_b mask moves the map by only 0.05 to 0.3), so
# the GPU bound is the smaller of the two (bound()): no wrong rule of the CPU test is within it, and no case is left out.
HALF_WRONG = {
    (0, "res5", "gradcam", 0, 0): 0.16, (0, "res5", "gradcam", 0, 1): 0.13, (0, "res5", "hirescam", 0, 0): 0.14,
    (0, "res5", "hirescam", 0, 1): 0.11, (0, "res5", "gradcam", 1, 0): 0.13, (0, "res5", "gradcam", 1, 1): 0.19,
    (0, "res5", "hirescam", 1, 0): 0.12, (0, "res5", "hirescam", 1, 1): 0.16, (0, "res4", "gradcam", 0, 0): 0.029,
    (0, "res4", "gradcam", 0, 1): 0.024, (0, "res4", "hirescam", 0, 0): 0.071, (0, "res4", "hirescam", 0, 1): 0.043,
    (0, "res4", "gradcam", 1, 0): 0.04, (0, "res4", "gradcam", 1, 1): 0.05, (0, "res4", "hirescam", 1, 0): 0.081,
    (0, "res4", "hirescam", 1, 1): 0.11, (1, "res5", "gradcam", 0, 0): 0.67, (1, "res5", "gradcam", 0, 1): 0.7,
    (1, "res5", "hirescam", 0, 0): 0.31, (1, "res5", "hirescam", 0, 1): 0.31, (1, "res5", "gradcam", 1, 0): 0.76,
    (1, "res5", "gradcam", 1, 1): 0.8, (1, "res5", "hirescam", 1, 0): 0.31, (1, "res5", "hirescam", 1, 1): 0.31,
    (1, "res4", "gradcam", 0, 0): 0.024, (1, "res4", "gradcam", 0, 1): 0.037, (1, "res4", "hirescam", 0, 0): 0.06,
    (1, "res4", "hirescam", 0, 1): 0.05, (1, "res4", "gradcam", 1, 0): 0.041, (1, "res4", "gradcam", 1, 1): 0.05,
    (1, "res4", "hirescam", 1, 0): 0.13, (1, "res4", "hirescam", 1, 1): 0.13}


def bound(case, yard):
    """the GPU test's bound on E for a case: MODEL_FACTOR x its bf16 yardstick, capped at half its smallest wrong-rule E"""
    return min(MODEL_FACTOR * yard, HALF_WRONG[case])


def E(x, r):
    return float((x.double() - r.double()).abs().max() / r.double().abs().max())


def _targets(target, B):
    return [int(target)] * B if isinstance(target, int) else [int(t) for t in target]


def autograd_cam(sd, cfg, video, layer, target, rounding=None, dtype=torch.float32):
    """{"logits" [B, classes], "A" the layer's activations and "grad" d sum_b logit[b, target_b] / d A [B, C, T, H, W],
    "gradcam", "hirescam" [B, T, H, W]} by torch.autograd on the oracle's graph"""
    p = {k: v.to(dtype) for k, v in sd.items()}
    v = video.to(dtype).clone().requires_grad_(True)  # or nothing in the graph has a grad_fn
    logits, stages = ref.resnet3d_forward(p, cfg, v, return_stages=True, rounding=rounding)
    A = stages[LAYERS[layer]]
    B = video.shape[0]
    t = _targets(target, B)
    (g,) = torch.autograd.grad(logits[torch.arange(B), torch.tensor(t)].sum(), A)
    A = A.detach()
    return {"logits": logits.detach(), "A": A, "grad": g, "gradcam": (g.mean((2, 3, 4), keepdim=True) * A).sum(1),
            "hirescam": (g * A).sum(1)}


def _fold(p, conv, bn, eps):
    sc = p[bn + ".weight"] / torch.sqrt(p[bn + ".running_var"] + eps)
    return p[conv + ".weight"] * sc.view(-1, 1, 1, 1, 1), p[bn + ".bias"] - p[bn + ".running_mean"] * sc


def head_seed(wc, target, grid, pool, cnt=True, dtype=torch.float64):
    """d logit[target_b] / d x of AvgPool3d(pool, stride 1) -> Linear -> global mean: [B, C, T, H, W]; cnt=False: the
    position-independent Wc / N (a global-mean head's seed, the wrong rule)"""
    T, H, W = grid
    if cnt:
        ax = []
        for L, k in zip(grid, pool):
            i = torch.arange(L)
            ax.append((torch.minimum(i, torch.tensor(L - k)) - torch.clamp(i - k + 1, min=0) + 1).to(dtype))
        npos = (T - pool[0] + 1) * (H - pool[1] + 1) * (W - pool[2] + 1)
        w = ax[0].view(-1, 1, 1) * ax[1].view(1, -1, 1) * ax[2].view(1, 1, -1) / (npos * pool[0] * pool[1] * pool[2])
    else:
        w = torch.full((T, H, W), 1.0 / (T * H * W), dtype=dtype)
    return wc.to(dtype)[torch.tensor(target)][:, :, None, None, None] * w[None, None]


def chain_cam(sd, cfg, video, layer, target, drop=()):
    """The maps by the rules of ResNet3d._explain_chain in fp64: {"logits", "A", "grad", "gradcam", "hirescam"}.
    drop: rules switched off, of DROPS -- "mask_out" / "mask_b" / "mask_a" (the ReLU mask at a block's output / after
    conv_b / after conv_a), "join" (the skip gradient is not added), "cnt" (a position-independent seed)."""
    assert set(drop) <= set(DROPS), drop
    p = {k: v.double() for k, v in sd.items()}
    eps = cfg.get("bn_eps", 1e-5)
    with torch.no_grad():
        logits, stages = ref.resnet3d_forward(p, cfg, video.double(), return_stages=True)
        B = video.shape[0]
        t = _targets(target, B)
        last = stages[-1]
        g = head_seed(p["blocks.5.proj.weight"], t, tuple(last.shape[2:]), cfg["head_pool"], cnt="cnt" not in drop)
        A = stages[LAYERS[layer]]
        if layer == "res4":
            # res5 again, block by block, with BatchNorm folded, keeping what the backward reads
            s = len(cfg["depths"]) - 1
            ka, ss = tuple(cfg["conv_a_kernels"][s]), cfg["spatial_strides"][s]
            pa = tuple(k // 2 for k in ka)
            x, kept = A, []
            for i in range(cfg["depths"][s]):
                pre = f"blocks.{s + 1}.res_blocks.{i}."
                stride = (1, ss, ss) if i == 0 else (1, 1, 1)
                w1 = _fold(p, pre + "branch1_conv", pre + "branch1_norm", eps) if pre + "branch1_conv.weight" in p else None
                wa, wb, wc = (_fold(p, pre + f"branch2.conv_{n}", pre + f"branch2.norm_{n}", eps) for n in "abc")
                sc = x if w1 is None else F.conv3d(x, w1[0], w1[1], stride=stride)
                a = F.relu(F.conv3d(x, wa[0], wa[1], padding=pa))
                b = F.relu(F.conv3d(a, wb[0], wb[1], stride=stride, padding=(0, 1, 1)))
                out = F.relu(sc + F.conv3d(b, wc[0], wc[1]))
                kept.append((x.shape, a, b, out, w1, wa[0], wb[0], wc[0], stride))
                x = out
            assert float((x - last).abs().max()) <= 1e-9 * float(last.abs().max())  # the folded restatement is the oracle's
            d1, d2 = g, None
            for xs, a, b, out, w1, wa, wb, wc, stride in reversed(kept):
                d = d1 if d2 is None or "join" in drop else d1 + d2
                if "mask_out" not in drop:
                    d = d * (out > 0)
                dsk = d if w1 is None else torch.nn.grad.conv3d_input(xs, w1[0], d, stride=stride)
                dB = torch.nn.grad.conv3d_input(b.shape, wc, d)
                if "mask_b" not in drop:
                    dB = dB * (b > 0)
                dA = torch.nn.grad.conv3d_input(a.shape, wb, dB, stride=stride, padding=(0, 1, 1))
                if "mask_a" not in drop:
                    dA = dA * (a > 0)
                d1, d2 = torch.nn.grad.conv3d_input(xs, wa, dA, padding=pa), dsk
            g = d1 if "join" in drop else d1 + d2  # at the layer: joined, not masked by its activations
    return {"logits": logits, "A": A, "grad": g, "gradcam": (g.mean((2, 3, 4), keepdim=True) * A).sum(1),
            "hirescam": (g * A).sum(1)}
