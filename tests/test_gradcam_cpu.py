"""The rules of ResNet3d.explain (Grad-CAM / HiResCAM) on the CPU oracle, no GPU: the hand-written eval-mode chain of
tests/gradcam_ref.py (the closed-form head seed, the ReLU masks, the skip join, transposed convolutions with BatchNorm
folded) against plain autograd, the two exact identities at res5, and how visible each wrong rule is in
E = max|x - ref| / max|ref| (signed maps, per clip) -- which bounds the tolerance tests/test_gradcam_gpu.py may use.

Measured here (SMALL, seed-0 weights, both fixtures, target 0; the test prints every figure):
  other target >= 1.26, other method >= 0.237, position-independent seed (HiResCAM) >= 0.228, dropped output mask >=
  0.67, dropped join >= 0.98, dropped conv_a mask >= 0.12, dropped conv_b mask >= 0.049;
  bf16 yardstick (activations and weights rounded, tests/test_gradcam_gpu.py's) 2.9e-3 to 1.9e-2 (target 0), 6e-3 to
  5.2e-2 (target 1)."""
import pytest
import torch

import gradcam_ref as R
from vclip_amd.weights import make_resnet3d_weights, make_synthetic_video


@pytest.fixture(scope="module")
def sd():
    return {k: torch.from_numpy(v) for k, v in make_resnet3d_weights(R.SMALL, seed=0).items()}


@pytest.fixture(scope="module")
def table(sd):
    """per (fixture, layer, target): autograd fp32, autograd with bf16 storage, the chain in fp64"""
    out = {}
    for fi, (B, T, HW, seed) in enumerate(R.FIXTURES):
        video = torch.from_numpy(make_synthetic_video(B, T, HW, seed=seed))
        for layer in R.LAYERS:
            for t in (0, 1):
                out[(fi, layer, t)] = dict(video=video, ref=R.autograd_cam(sd, R.SMALL, video, layer, t),
                                           ref16=R.autograd_cam(sd, R.SMALL, video, layer, t, rounding=R.BF16),
                                           chain=R.chain_cam(sd, R.SMALL, video, layer, t))
    return out


def test_fixture_geometry(table):
    assert tuple(table[(0, "res5", 0)]["ref"]["A"].shape) == (2, 2048, 8, 2, 2)
    assert tuple(table[(0, "res4", 0)]["ref"]["A"].shape) == (2, 1024, 8, 4, 4)
    assert tuple(table[(1, "res5", 0)]["ref"]["A"].shape) == (2, 2048, 6, 3, 3)  # the pool has 2 x 2 spatial positions
    assert tuple(table[(1, "res4", 0)]["ref"]["A"].shape) == (2, 1024, 6, 6, 6)


def test_chain_equals_autograd(table):
    """the hand-written rules are the gradient: to fp32 rounding (the reference is fp32 autograd, the chain fp64)"""
    for (fi, layer, t), r in table.items():
        for m in R.METHODS:
            for b in range(2):
                e = R.E(r["chain"][m][b], r["ref"][m][b])
                print(f"fixture {fi} {layer} target {t} {m} clip {b}: E(chain, autograd) {e:.2e}")
                assert e <= 1e-5, (fi, layer, t, m, b, e)
        assert R.E(r["chain"]["grad"], r["ref"]["grad"]) <= 1e-5


def test_res5_identities(sd, table):
    """HiResCAM at res5 sums to logit - bias (the head is linear in res5), and Grad-CAM there is classic CAM,
    sum_c Wc[target, c] / N * A: the mean of the seed's pool-window weights over the grid is 1 / N"""
    wc, bc = sd["blocks.5.proj.weight"].double(), sd["blocks.5.proj.bias"].double()
    for fi in range(len(R.FIXTURES)):
        for t in (0, 1):
            r = table[(fi, "res5", t)]["chain"]
            total = r["hirescam"].sum(dim=(1, 2, 3))
            want = r["logits"][:, t] - bc[t]
            print(f"fixture {fi} target {t}: sum hirescam - (logit - bias) {(total - want).abs().max():.2e}")
            assert float((total - want).abs().max()) <= 1e-9
            ref32 = table[(fi, "res5", t)]["ref"]
            d32 = ref32["hirescam"].double().sum(dim=(1, 2, 3)) - (ref32["logits"][:, t].double() - bc[t])
            assert float(d32.abs().max()) <= 5e-6  # the fp32 autograd maps: 5e-7 measured
            A = r["A"]
            n = A.shape[2] * A.shape[3] * A.shape[4]
            cam = (wc[t].view(1, -1, 1, 1, 1) / n * A).sum(1)
            assert R.E(r["gradcam"], cam) <= 1e-12


def wrong_rules(sd, table, fi, layer, t, m):
    """{rule: [E per clip]} of every wrong rule that applies to the case"""
    r = table[(fi, layer, t)]
    ref = r["ref"][m]
    other_m = R.METHODS[1 - R.METHODS.index(m)]
    w = {"other target": [R.E(table[(fi, layer, 1 - t)]["ref"][m][b], ref[b]) for b in range(2)],
         "other method": [R.E(r["ref"][other_m][b], ref[b]) for b in range(2)]}
    drops = (["cnt"] if m == "hirescam" else []) + (["mask_out", "mask_b", "mask_a", "join"] if layer == "res4" else [])
    for d in drops:
        got = R.chain_cam(sd, R.SMALL, r["video"], layer, t, drop=(d,))[m]
        w[f"dropped {d}"] = [R.E(got[b], ref[b]) for b in range(2)]
    return w


def test_wrong_rules_are_visible(sd, table):
    """E of every wrong rule, per case, against the bf16 yardstick: the floors measured for target 0 hold, and the GPU
    test's bound stays at or below half the case's smallest wrong-rule E, for every case of both targets.
    MODEL_FACTOR x yardstick alone does not (printed as "smallest / 2 / yardstick" below MODEL_FACTOR = 8: 2.4 to 5.8
    in the sixteen res4 cases, where a dropped conv_b mask moves the map by only 0.05 to 0.3 against a yardstick of 5e-3
    to 5e-2), so the bound is capped at gradcam_ref.HALF_WRONG, whose entries are checked here."""
    floors = {"other target": 1.25, "other method": 0.23, "dropped cnt": 0.22}  # the measured minima, rounded down
    broken, uncapped = [], []
    for fi in range(len(R.FIXTURES)):
        for layer in R.LAYERS:
            for t in (0, 1):
                for m in R.METHODS:
                    w = wrong_rules(sd, table, fi, layer, t, m)
                    r = table[(fi, layer, t)]
                    for b in range(2):
                        yard = R.E(r["ref16"][m][b], r["ref"][m][b])
                        small = min(v[b] for v in w.values())
                        npos = int((r["ref"][m][b] > 0).sum())
                        print(f"fixture {fi} {layer} target {t} {m} clip {b}: yardstick {yard:.2e}, positive {npos}/"
                              f"{r['ref'][m][b].numel()}, " + ", ".join(f"{k} {v[b]:.3g}" for k, v in w.items())
                              + f"; smallest / 2 / yardstick = {small / 2 / yard:.2f}")
                        if t == 0:
                            for k, floor in floors.items():
                                assert k not in w or w[k][b] >= floor, (fi, layer, m, b, k, w[k][b])
                        case = (fi, layer, m, t, b)
                        # the table is the computed half, rounded down to two digits: never above it, never stale
                        assert 0.9 * small / 2 <= R.HALF_WRONG[case] <= small / 2, (case, small / 2)
                        if R.bound(case, yard) > small / 2:
                            broken.append((case, yard, small))
                        if R.MODEL_FACTOR * yard > small / 2:
                            uncapped.append(case)
    print(f"{len(uncapped)} cases where MODEL_FACTOR x yardstick alone exceeds half the smallest wrong-rule E:", uncapped)
    assert len(R.HALF_WRONG) == 32 and not broken, broken
