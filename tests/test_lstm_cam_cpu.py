"""VideoResNet50LSTM.explain on the CPU, no GPU: the autograd reference of tests/lstm_cam_ref.py (its forward against
oracle/lstm_ref.py, the conditions on the fixtures' seeds, the closed forms of the rule at res5), how visible each wrong
rule is in E = max|x - ref| / max|ref| (per video, signed) -- which caps the tolerance tests/test_lstm_cam_gpu.py may use --
and the parts of the feature that need no GPU: the two entry points of csrc/frame_cam.hip declared, bound and exported,
the inference parser's flags, Explanation.frame_relevance.

Measured here (seed-0 weights, the three fixtures, ten videos; the test prints every figure): BPTT with the cell path
dropped moves frame_relevance by >= 0.26 and the maps by >= 0.54; the top layer's chain through time skipped >= 0.20 and
>= 0.28; a missing 1/P is P - 1 = 3 at res5 and res4 alike; a per-video instead of a per-frame alpha moves res4 Grad-CAM by
>= 0.34; a dropped conv_b mask moves the res4 maps by >= 0.20.  The bf16 yardstick is 1.3e-2 to 2.3e-1.  A one-frame video
has no step through time and is its own clip: only the missing 1/P and the dropped mask apply to it, and nothing to its
frame relevance."""
import ctypes
import re

import pytest
import torch

import lstm_cam_ref as R
from vclip_amd import _lib
from vclip_amd.build import INCLUDE, LIB_PATH, build

ENTRIES = ("vc_frame_cam", "vc_frame_avgpool_bwd")


@pytest.fixture(scope="module")
def p():
    return R.weights()


@pytest.fixture(scope="module")
def table(p):
    """per (fixture, video): the fp32 autograd reference for both targets and with bf16 storage, computed once"""
    out = {}
    for name in R.FIXTURES:
        _, _, vids = R.fixture_video(name)
        for b, fr in enumerate(vids):
            out[(name, b)] = dict(frames=fr, ref={t: R.autograd_cam(p, fr, t) for t in (0, 1)},
                                  ref16=R.autograd_cam(p, fr, 1, rounding=R.BF16))
    return out


def test_fixture_geometry_and_forward_is_the_oracle(p, table):
    from oracle.lstm_ref import lstm_forward
    assert [len(R.fixture_video(n)[2]) for n in R.FIXTURES] == [2, 3, 5]
    r = table[("ragged3", 2)]["ref"][1]
    assert tuple(r["A"]["res5"].shape) == (6, 2048, 2, 2) and tuple(r["A"]["res4"].shape) == (6, 1024, 4, 4)
    assert tuple(r["g"].shape) == (6, 2048) and tuple(r[("res4", "gradcam")].shape) == (6, 4, 4)
    for (name, b), e in table.items():
        with torch.no_grad():
            want = lstm_forward(p, e["frames"].permute(1, 0, 2, 3)[None])  # torch's own nn.LSTM
        z = e["ref"][1]["logit"]
        print(f"{name} video {b}: logit {float(z):+.6f}, oracle {float(want):+.6f}")
        assert abs(float(z) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))


def test_seeds_give_live_maps(table):
    """every video's fp32 maps and frame relevance are non-zero for both targets and positive somewhere for at least one"""
    for (name, b), e in table.items():
        for q in R.quantities():
            m0, m1 = e["ref"][0][q], e["ref"][1][q]
            top = max(float(m0.abs().max()), float(m1.abs().max()))
            print(f"{name} video {b} {q}: max|map| {top:.3e}, positive entries target 0 {int((m0 > 0).sum())}, "
                  f"target 1 {int((m1 > 0).sum())} of {m1.numel()}")
            assert float(m0.abs().max()) > 0 and float(m1.abs().max()) > 0, (name, b, q)
            assert bool((m0 > 0).any()) or bool((m1 > 0).any()), (name, b, q)
        assert float(e["ref"][1]["g"].abs().max()) > 0


def test_closed_forms(table):
    """at res5 the gradient is g / P, uniform over the positions, so Grad-CAM equals HiResCAM; target 0 is minus target 1"""
    for (name, b), e in table.items():
        r = e["ref"][1]
        P = r["A"]["res5"].shape[2] * r["A"]["res5"].shape[3]
        assert R.E(r["G"]["res5"], (r["g"] / P)[:, :, None, None].expand_as(r["G"]["res5"])) <= 1e-6
        assert R.E(r[("res5", "gradcam")], r[("res5", "hirescam")]) <= 1e-6
        want = (r["g"][:, :, None, None] * r["A"]["res5"]).sum(1) / P
        assert R.E(r[("res5", "gradcam")], want) <= 1e-6
        assert R.E(r[("res5", "gradcam")].sum(dim=(1, 2)), r["frame"]) <= 1e-5  # the pool is linear: the map sums to g . f
        for q in R.quantities():
            assert R.E(e["ref"][0][q], -r[q]) <= 1e-6, (name, b, q)


def test_wrong_rules_are_visible(p, table):
    """E of every wrong rule per (video, quantity) against the bf16 yardstick; lstm_cam_ref.HALF_WRONG holds half of the
    smallest, rounded down, and the GPU test's bound never exceeds it"""
    floors = {"cell": 0.26, "l1_chain": 0.2, "no_p": 2.99, "clip_alpha": 0.34, "mask_b": 0.2}  # measured minima, rounded down
    stale, broken, cases = [], [], 0
    for (name, b), e in table.items():
        w = R.wrong_rule_E(p, e["frames"], e["ref"][1])
        for q in R.quantities():
            yard = R.E(e["ref16"][q], e["ref"][1][q])
            if not w[q]:  # the frame relevance of a one-frame video: no wrong rule touches it, no cap
                assert q == "frame" and e["frames"].shape[0] == 1 and (name, b, q) not in R.HALF_WRONG
                continue
            cases += 1
            small = min(w[q].values())
            print(f"{name} video {b} {q}: yardstick {yard:.2e}, " + ", ".join(f"{k} {v:.3g}" for k, v in w[q].items())
                  + f"; smallest / 2 = {small / 2:.3g}, / yardstick = {small / 2 / yard:.1f}")
            for k, v in w[q].items():
                assert v >= floors[k], (name, b, q, k, v)
            case = (name, b, q)
            if case not in R.HALF_WRONG or not 0.9 * small / 2 <= R.HALF_WRONG[case] <= small / 2:
                stale.append((case, round(small / 2, 4)))
            elif R.bound(case, yard) > small / 2:
                broken.append((case, yard, small))
    assert len(R.HALF_WRONG) == cases == 48 and not stale and not broken, (stale, broken)


def test_entry_points_declared_bound_and_exported():
    build()
    names = _lib.header_functions()
    raw = ctypes.CDLL(LIB_PATH)
    with open(f"{INCLUDE}/vclip.h") as f:
        header = f.read()
    for n in ENTRIES:
        assert n in names, f"{n} not declared in vclip.h"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(raw, n), f"{n} declared in vclip.h but not exported"
        decl = re.search(rf"\bint {n}\s*\(([^;]*)\);", header).group(1)
        params = [a.strip() for a in decl.split(",")]
        argtypes, restype = _lib.SIGNATURES[n]
        assert restype is _lib.c_int and len(argtypes) == len(params), (n, params)
        for a, t in zip(params, argtypes):  # pointers and the stream as void*, the extents as int64
            want = _lib.c_p if ("*" in a or "hipStream_t" in a) else _lib.c_i64 if a.startswith("int64_t") else _lib.c_int
            assert t is want, (n, a)


def _parser():
    from vclip_amd.apps import build_parser_lstm
    return build_parser_lstm(inference=True)


BASE = ["--videos_dir", "v", "--model_path", "m"]


def test_parser_flags():
    a = _parser().parse_args(BASE)
    assert a.saliency is None and a.saliency_class is None and a.saliency_layer == "res5"
    a = _parser().parse_args(BASE + ["--saliency", "hirescam", "--saliency_class", "0", "--saliency_layer", "res4"])
    assert (a.saliency, a.saliency_class, a.saliency_layer) == ("hirescam", 0, "res4")
    for bad in (["--saliency", "rollout"], ["--saliency", "gradcam", "--saliency_class", "2"],
                ["--saliency", "gradcam", "--saliency_layer", "res3"]):
        with pytest.raises(SystemExit):
            _parser().parse_args(BASE + bad)
    assert not any(o.startswith("--saliency") for act in __import__("vclip_amd.apps", fromlist=["x"]).build_parser_lstm(
        inference=False)._actions for o in act.option_strings)  # the training parser is untouched


@pytest.mark.parametrize("extra,msg", [(["--saliency_class", "1"], "--saliency_class needs --saliency"),
                                        (["--saliency_layer", "res4"], "--saliency_layer needs --saliency"),
                                        (["--saliency", "gradcam", "--saliency_layer", "res4", "--stream_chunk", "4"],
                                         "--saliency_layer does not apply with --stream_chunk")])
def test_parser_errors_before_any_work(extra, msg, tmp_path, capsys):
    """flag combinations that make no sense are parser errors, raised before the model or any output directory exists"""
    from vclip_amd.apps import run_inference
    with pytest.raises(SystemExit) as e:
        run_inference("lstm", BASE + ["--output_dir", str(tmp_path / "out")] + extra)
    assert e.value.code == 2 and msg in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_explanation_frame_relevance_defaults_to_none():
    from vclip_amd.vivit import Explanation
    ex = Explanation(None, None, None, None, "rollout")
    assert ex.frame_relevance is None and ex.target is None
    assert Explanation(None, None, None, None, "gradcam", target=[1], frame_relevance=[2]).frame_relevance == [2]
