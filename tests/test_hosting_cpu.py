"""The host-side base classes of the model families (vclip_amd.hosting): parameter store, pack and workspace
caches, the graph-replay key, and the per-thread capture state of vclip_amd.streams.  No GPU needed."""
import contextlib
import json
import os
import threading

import numpy as np
import pytest
import torch

from vclip_amd import streams, vivit_train
from vclip_amd.hosting import FusedVideoModel, round_up

GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = {"a.weight": (2, 3), "a.bias": (2,), "norm.weight": (3,), "norm.running_mean": (3,)}


class Toy(FusedVideoModel):
    def __init__(self):
        super().__init__(SHAPES, 2, frozen=lambda n: n.endswith("running_mean"))

    def _pack(self, device, extra=()):
        pk = self._cached_pack(device, extra)
        if pk is None:
            pk = self._packed = {"device": device, "version": self._weights_version(), "extra": extra}
        return pk


def _values(seed=0):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(s, generator=g) for n, s in SHAPES.items()}


def test_round_up():
    assert [round_up(x, 128) for x in (0, 1, 128, 129)] == [0, 128, 128, 256]


def test_param_store_round_trip():
    m = Toy()
    assert list(m.state_dict()) == list(SHAPES)
    assert [p.requires_grad for p in m._param_list()] == [True, True, True, False]
    sd = _values()
    sd["a.bias"] = sd["a.bias"].numpy()  # arrays load too
    assert m.load_state_dict(sd) == ([], [])
    got = m.state_dict()
    assert all(torch.equal(got[n], torch.as_tensor(sd[n])) for n in SHAPES)
    assert not any(v.requires_grad for v in got.values())
    m2 = Toy()
    m2.load_state_dict({"module." + n: v for n, v in got.items()})  # a DataParallel checkpoint
    assert all(torch.equal(m2.P(n), got[n]) for n in SHAPES)


def test_load_state_dict_strictness_and_pack_drop():
    m = Toy()
    sd = _values()
    del sd["a.bias"]
    sd["extra.weight"] = torch.zeros(1)
    with pytest.raises(KeyError) as e:
        m.load_state_dict(sd)
    assert "load_state_dict: missing=['a.bias'] unexpected=['extra.weight']" in str(e.value)
    pk = m._pack("cpu")
    assert m._packed is pk
    assert m.load_state_dict(sd, strict=False) == (["a.bias"], ["extra.weight"])
    assert m._packed is None  # a load drops the pack
    assert torch.equal(m.P("a.weight"), sd["a.weight"])


def test_cached_pack_validity():
    m = Toy()
    pk = m._pack("cpu")
    assert m._pack("cpu") is pk and m._cached_pack("cpu") is pk
    assert m._cached_pack("cpu", extra=(torch.float16,)) is None
    assert m._cached_pack("cuda:0") is None
    with torch.no_grad():
        m.P("a.weight").add_(1.0)
    assert m._cached_pack("cpu") is None
    pk = m._pack("cpu")
    vivit_train.MASTER_EPOCH[0] += 1  # what the fused AdamW does after writing the masters through raw pointers
    try:
        assert m._cached_pack("cpu") is None
    finally:
        vivit_train.MASTER_EPOCH[0] -= 1
    assert m._cached_pack("cpu") is pk


def test_cached_workspace():
    m = Toy()
    made = []

    def build():
        made.append(len(made))
        return {"id": made[-1]}

    ws = m._cached_workspace("k0", build, 3)
    assert m._cached_workspace("k0", build, 3) is ws and made == [0]
    assert len(m._ws_used) == 1 and m._ws_used[0] is ws  # appended once only
    m._ws_used = []  # what every forward starts with
    assert m._cached_workspace("k0", build, 3) is ws and m._ws_used == [ws]
    m._cached_workspace("k1", build, 3)
    m._cached_workspace("k2", build, 3)
    assert set(m._ws) == {"k0", "k1", "k2"}
    w3 = m._cached_workspace("k3", build, 3)  # the limit + 1-th distinct key empties the cache first
    assert set(m._ws) == {"k3"} and m._ws["k3"] is w3
    assert any(w is ws for w in m._ws_used)  # the running forward still lists what it addressed


def _vivit():
    from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
    cfg = json.loads(str(np.load(os.path.join(GD, "vivit_tiny.npz"))["config"]))
    m = VivitForVideoClassification(VivitConfig(**cfg, id2label={0: "non-referral", 1: "referral"})).eval()
    knobs = dict(compute_dtype=torch.float16, gemm_cfg={"qkv": 5}, rows="tight", precise_layers=1,
                 precise_ops=("embed_w",), stream_priorities=(0, -1), cls_only_last_layer=False)
    return m, (2, cfg["num_frames"], cfg["num_channels"], cfg["image_size"], cfg["image_size"]), knobs


def _timesformer():
    from vclip_amd.timesformer import TimesformerConfig, TimesformerForVideoClassification
    cfg = json.loads(str(np.load(os.path.join(GD, "timesformer_tiny.npz"))["config"]))
    m = TimesformerForVideoClassification(TimesformerConfig(**cfg, id2label={0: "non-referral", 1: "referral"}))
    return (m, (2, cfg["num_frames"], cfg["num_channels"], cfg["image_size"], cfg["image_size"]),
            dict(proj_cfg=None, gemm_cfg={"fc1": 8}))


def _swin():
    from vclip_amd.swin3d import Swin3d
    m = Swin3d(dict(patch_size=(2, 4, 4), embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=(2, 3, 3),
                    mlp_ratio=4.0, layer_norm_eps=1e-5), num_classes=2)
    return m, (2, 3, 8, 48, 48), {}


def _resnet3d():
    from oracle import resnet3d_ref as ref
    from vclip_amd.resnet3d import ResNet3d
    return (ResNet3d(ref.RESNET3D_50), (2, 3, 8, 32, 32),
            dict(implicit_conv=False, conv_ring={"s3": 3}, conv_cfg={"conv_a.s4": (4, 1)}))


@pytest.mark.parametrize("make", [_vivit, _timesformer, _swin, _resnet3d])
def test_graph_key(make):
    """Element 0 is the input address (GraphReplay.run serves new tensors of a captured configuration by
    key[1:]); everything that selects kernels moves key[1:]."""
    m, shape, knobs = make()
    x = torch.zeros(shape)
    m._check_input(x)
    with pytest.raises(ValueError):
        m._check_input(torch.zeros(shape[:1] + (shape[1] + 1,) + shape[2:]))
    key = m._graph_key(x)
    assert key[0] == x.data_ptr()
    assert m._graph_key(x) == key
    assert m._graph_key(torch.zeros(shape))[1:] == key[1:]
    seen = {key[1:]}
    for name, value in dict(concurrent_streams=2, split_sizes=[1, 1], **knobs).items():
        old = getattr(m, name)
        setattr(m, name, value)
        k = m._graph_key(x)
        assert k[0] == x.data_ptr() and k[1:] not in seen, name
        seen.add(k[1:])
        setattr(m, name, old)
        assert m._graph_key(x) == key, name
    with torch.no_grad():
        m._param_list()[0].add_(1.0)
    assert m._graph_key(x)[1:] not in seen  # the weights version
    assert m._graphs is not None and m._graph_keep()[:2] == (m._packed, ())


def test_capture_state_is_per_thread(monkeypatch):
    """While one thread holds GraphReplay's capture context, a split forward on another thread still runs its
    parts (and may tune); the holder's own fork_parts runs eagerly again after the context."""
    class FakeStream:
        def wait_stream(self, other):
            pass

    monkeypatch.setattr(torch.cuda, "stream", lambda st: contextlib.nullcontext())
    sts, cur = [FakeStream(), FakeStream()], FakeStream()
    parts, ran, seen = [], [], []

    def other():
        seen.append((streams._CAPTURE.parts, streams._CAPTURE.no_tune))
        streams.fork_parts(sts, cur, [lambda: ran.append(0), lambda: ran.append(1)])

    with streams._capturing(parts):
        assert streams._CAPTURE.parts is parts and streams._CAPTURE.no_tune
        t = threading.Thread(target=other)
        t.start()
        t.join()
    assert ran == [0, 1] and parts == [] and seen == [(None, False)]
    assert streams._CAPTURE.parts is None and not streams._CAPTURE.no_tune
    streams.fork_parts(sts, cur, [lambda: ran.append(2), lambda: ran.append(3)])
    assert ran == [0, 1, 2, 3] and parts == []
