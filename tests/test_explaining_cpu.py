"""The host-side scaffold the families' explain paths share (vclip_amd.explaining): target checks and their messages,
the refusals, the per-clip normalisation and the buffer cache.  No GPU needed."""
import numpy as np
import pytest
import torch

import vclip_amd
from vclip_amd import explaining
from vclip_amd.explaining import (Explanation, cached_explain, check_targets, expand_targets, normalise,
                                  require_explainable, require_method, require_residual)
from vclip_amd.hosting import FusedVideoModel


def test_explanation_has_one_home():
    from vclip_amd import rise, vivit
    assert vivit.Explanation is Explanation and issubclass(vclip_amd.RiseExplanation, Explanation)
    assert rise.Explanation is Explanation
    ex = Explanation(None, None, None, None, "rollout")
    assert ex.target is None and ex.frame_relevance is None and ex.method == "rollout"


def test_check_targets_values():
    assert check_targets(None, 2) == (None, False)
    assert check_targets(1, 2) == ([1], True)
    assert check_targets(np.int64(0), 2) == ([0], True)
    assert check_targets([0, 1], 2) == ([0, 1], False)
    assert check_targets((1,), 2) == ([1], False)
    assert check_targets(np.array([1, 0]), 2) == ([1, 0], False)
    assert check_targets(torch.tensor([1, 1, 0]), 2) == ([1, 1, 0], False)
    from vclip_amd.vivit import VivitForVideoClassification
    assert VivitForVideoClassification._check_targets([1], 2) == ([1], False)  # the alias the tests call


@pytest.mark.parametrize("who", ["explain", "explain_class"])
def test_check_targets_messages(who):
    kw = {} if who == "explain" else {"who": who}  # "explain" is the default prefix
    for bad in (torch.tensor([0.5]), torch.tensor([True])):
        with pytest.raises(ValueError) as e:
            check_targets(bad, 2, **kw)
        assert str(e.value) == f"{who}: target must hold integers"
    for bad in (True, 1.5, "a", [0, 1.5], [None]):
        with pytest.raises(ValueError) as e:
            check_targets(bad, 2, **kw)
        assert str(e.value) == f"{who}: target must be None, an int or a sequence of B ints"
    for bad, shown in ((2, [2]), (-1, [-1]), ([0, 3], [0, 3])):
        with pytest.raises(ValueError) as e:
            check_targets(bad, 2, **kw)
        assert str(e.value) == f"{who}: target {shown} out of range for 2 labels"


def test_expand_targets():
    assert expand_targets(None, False, 3) is None
    assert expand_targets([1], True, 3) == [1, 1, 1]
    assert expand_targets([0, 1, 1], False, 3) == [0, 1, 1]
    assert expand_targets([1], False, 1) == [1]  # a sequence of one is not a scalar: its length is checked
    with pytest.raises(ValueError) as e:
        expand_targets([1], False, 3)
    assert str(e.value) == "explain: target has 1 entries for 3 clips"
    with pytest.raises(ValueError) as e:
        expand_targets([0, 1], False, 3, who="explain_class")
    assert str(e.value) == "explain_class: target has 2 entries for 3 clips"
    with pytest.raises(ValueError) as e:
        expand_targets([0, 1], False, 1, what="videos")
    assert str(e.value) == "explain: target has 2 entries for 1 videos"
    with pytest.raises(ValueError) as e:
        expand_targets([0, 1], False, 1, who="")
    assert str(e.value) == "target has 2 entries for 1 clips"


def test_refusals_and_their_messages():
    model = torch.nn.Linear(1, 1)
    x = torch.zeros(1)
    with pytest.raises(RuntimeError) as e:
        require_explainable(model, x)  # a constructed module is in training mode
    assert str(e.value) == "explain: inference only; call model.eval() first"
    model.eval()
    for bad in (x, None, [1.0]):
        with pytest.raises(RuntimeError) as e:
            require_explainable(model, bad)
        assert str(e.value) == "explain runs on the GPU only: move the clip batch to cuda"
    with pytest.raises(RuntimeError) as e:
        require_explainable(model, x, what="pixel_values")
    assert str(e.value) == "explain runs on the GPU only: move pixel_values to cuda"
    with pytest.raises(RuntimeError) as e:
        require_explainable(model, x, who="explain_class")
    assert str(e.value) == "explain_class runs on the GPU only: move the clip batch to cuda"
    with pytest.raises(RuntimeError) as e:
        require_explainable(model.train(), x, who="explain_class")
    assert str(e.value) == "explain_class: inference only; call model.eval() first"

    require_method("rollout", ("rollout", "cls_attention"))
    with pytest.raises(ValueError) as e:
        require_method("gradcam", ("rollout",))
    assert str(e.value) == "explain: method must be one of ('rollout',), not 'gradcam'"
    for ok in (1e-9, 0.5, 1, 1.0):
        require_residual(ok)
    for bad in (0, 0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError) as e:
            require_residual(bad)
        assert str(e.value) == f"explain: residual must be in (0, 1], not {bad}"


def test_normalise_plain_is_the_division():
    g = torch.Generator().manual_seed(0)
    rel = torch.rand(3, 37, generator=g).double()
    got = normalise(rel, zero_ok=False)
    assert got.dtype == torch.float32 and got.shape == rel.shape
    assert torch.equal(got, (rel / rel.sum(dim=1, keepdim=True)).float())
    assert torch.equal(normalise(rel, zero_ok=True), got)  # positive sums: the same bits either way
    # every dimension after the first is the clip's: TimeSformer passes a transposed [B, T, P] view
    view = rel.reshape(3, 37, 1).expand(3, 37, 2).transpose(1, 2)
    assert torch.equal(normalise(view, zero_ok=False), (view / view.sum(dim=(1, 2), keepdim=True)).float())
    assert torch.isnan(normalise(torch.zeros(1, 4, dtype=torch.float64), zero_ok=False)).all()  # nothing is hidden


def test_normalise_zero_ok():
    rel = torch.tensor([[0.0, 0.0, 0.0], [1.0, 3.0, 0.0], [0.0, 0.0, 1e-40]], dtype=torch.float64)
    got = normalise(rel, zero_ok=True)
    assert got.dtype == torch.float32
    assert torch.equal(got, torch.tensor([[0.0, 0.0, 0.0], [0.25, 0.75, 0.0], [0.0, 0.0, 1.0]]))
    # ResNet3d's and Swin3d.explain_class's earlier expressions, bit for bit
    g = torch.Generator().manual_seed(1)
    pos = (torch.randn(4, 50, generator=g).double()).clamp_min(0)
    pos[2] = 0
    tot = pos.sum(dim=1, keepdim=True)
    cam = torch.where(tot > 0, pos / tot.clamp_min(1e-300), torch.zeros_like(pos)).float()
    swin = torch.where(tot > 0, pos / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(pos)).float()
    assert torch.equal(normalise(pos, zero_ok=True), cam) and torch.equal(cam, swin)
    assert not normalise(pos, zero_ok=True)[2].any()


def test_cache_builds_once_and_evicts_at_the_limit():
    built = []

    def build(tag):
        def f():
            built.append(tag)
            return {"tag": tag}
        return f

    cache = {}
    a = cached_explain(cache, "a", build("a"))
    assert cached_explain(cache, "a", build("a2")) is a and built == ["a"]
    b = cached_explain(cache, "b", build("b"))
    assert set(cache) == {"a", "b"} and cached_explain(cache, "a", build("a3")) is a
    c = cached_explain(cache, "c", build("c"))  # two entries are held: both go before the third is built
    assert set(cache) == {"c"} and cache["c"] is c and built == ["a", "b", "c"]
    assert cached_explain(cache, "b", build("b2")) is not b and set(cache) == {"c", "b"}

    one = {}
    cached_explain(one, 1, build(1), limit=1)
    first = cached_explain(one, 1, build(1), limit=1)
    cached_explain(one, 2, build(2), limit=1)  # the LSTM model's workspace: one key at a time
    assert set(one) == {2} and cached_explain(one, 1, build(1), limit=1) is not first


def test_fused_models_share_the_cache_helper():
    m = FusedVideoModel({"w": (1,)}, 2)
    assert m._explain_ws == {}
    buf = m._cached_explain(m._explain_ws, ("k",), lambda: [1])
    assert m._cached_explain(m._explain_ws, ("k",), lambda: [2]) is buf
    m._drop_device_state()
    assert m._explain_ws == {}
    assert explaining.cached_explain is FusedVideoModel._cached_explain
