"""vclip_amd.lora on the host: what `attach` builds (names, shapes, initialisation, requires_grad, layer selection),
its argument checks, the adapter state-dict round trip and the ViViT trainer's new flags.  No GPU: nothing here
launches a kernel."""
import json
import math
import os

import pytest
import torch

from vclip_amd import apps, lora
from vclip_amd.vivit import VivitConfig, VivitForVideoClassification
from vclip_amd.weights import make_vivit_weights

SMALL = dict(image_size=32, num_frames=4, tubelet_size=[2, 16, 16], num_channels=3, hidden_size=256,
             num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, hidden_act="gelu_fast",
             layer_norm_eps=1e-6, qkv_bias=True)
D, I = 256, 512
DIMS = {"q": (D, D), "k": (D, D), "v": (D, D), "o": (D, D), "fc1": (I, D), "fc2": (D, I)}
MODULE = {"q": "attention.q_proj", "k": "attention.k_proj", "v": "attention.v_proj", "o": "attention.o_proj",
          "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
HEAD_NUMEL = 2 * D + 2


def _model(cfg=SMALL):
    model = VivitForVideoClassification(VivitConfig(**cfg, id2label={0: "non-referral", 1: "referral"}))
    model.load_state_dict(make_vivit_weights(cfg, seed=0))
    return model


@pytest.mark.parametrize("rank,targets,train_head", [(8, ("q", "v"), True), (3, ("q", "k", "v", "o", "fc1", "fc2"), True),
                                                      (4, ("fc2", "o"), False)])
def test_attach_names_shapes_and_trainable_count(rank, targets, train_head):
    model = _model()
    base = {n: p.detach().clone() for n, p in model.hf_state_dict().items()}
    assert lora.attach(model, rank=rank, alpha=2.0 * rank, targets=targets, train_head=train_head) is model
    sd = lora.state_dict(model)
    want = {}
    for i in range(2):
        for t in targets:
            nout, nin = DIMS[t]
            want[f"vivit.layers.{i}.{MODULE[t]}.lora_A.weight"] = (rank, nin)
            want[f"vivit.layers.{i}.{MODULE[t]}.lora_B.weight"] = (nout, rank)
    got = {k: tuple(v.shape) for k, v in sd.items() if "lora_" in k and k != "lora_config"}
    assert got == want
    assert ("classifier.weight" in sd) == train_head and ("classifier.bias" in sd) == train_head
    count = sum(2 * 0 + rank * (DIMS[t][0] + DIMS[t][1]) for t in targets) * 2 + (HEAD_NUMEL if train_head else 0)
    assert lora.trainable_parameters(model) == count
    assert sum(p.numel() for p in model.parameters() if p.requires_grad) == count
    # model.parameters() yields the adapters; model.state_dict() is the base weights alone, unchanged
    ids = {id(p) for p in model.parameters()}
    assert all(id(model.lora_params[k.replace(".", "__")]) in ids for k in want)
    msd = model.state_dict()
    assert list(msd) == list(base) and all(torch.equal(msd[n], base[n]) for n in base)
    # requires_grad: adapters yes, the classifier pair when train_head, every other base parameter no
    for n, p in model.hf_state_dict().items():
        assert p.requires_grad == (train_head and n in ("classifier.weight", "classifier.bias")), n
    assert all(model.lora_params[k.replace(".", "__")].requires_grad for k in want)
    assert sd["lora_config"] == {"rank": rank, "alpha": 2.0 * rank, "layers": [0, 1], "train_head": train_head,
                                 "targets": [t for t in lora.TARGETS if t in targets]}


def test_initialisation_b_zero_a_seeded():
    a, b, c = _model(), _model(), _model()
    lora.attach(a, rank=8, seed=5)
    lora.attach(b, rank=8, seed=5)
    lora.attach(c, rank=8, seed=6)
    sa, sb, sc = lora.state_dict(a), lora.state_dict(b), lora.state_dict(c)
    for k, v in sa.items():
        if k.endswith("lora_B.weight"):
            assert not v.any(), k
        elif k.endswith("lora_A.weight"):
            assert torch.equal(v, sb[k]) and not torch.equal(v, sc[k]), k
            # kaiming_uniform_(a = sqrt 5): uniform in +-1 / sqrt(fan_in), filling the range
            bound = 1.0 / math.sqrt(v.shape[1])
            assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.9 * bound
            assert abs(float(v.mean())) < 0.1 * bound
    # adapters of one model differ from each other (one generator runs through them)
    ks = [k for k in sa if k.endswith("lora_A.weight")]
    assert not torch.equal(sa[ks[0]], sa[ks[1]])


def test_layers_int_and_list():
    four = dict(SMALL, num_hidden_layers=4)
    for layers, want in ((None, [0, 1, 2, 3]), (1, [3]), (3, [1, 2, 3]), ([2, 0], [0, 2]), ((1,), [1]), (range(1, 3), [1, 2])):
        model = VivitForVideoClassification(VivitConfig(**four))
        lora.attach(model, rank=2, targets=("q",), layers=layers)
        cfg = lora.state_dict(model)["lora_config"]
        assert cfg["layers"] == want, layers
        got = sorted({int(k.split(".")[2]) for k in lora.state_dict(model) if "lora_A" in k})
        assert got == want, layers


@pytest.mark.parametrize("kw", [dict(targets=("q", "w")), dict(targets=()), dict(targets=("q", "q")), dict(rank=0),
                                dict(rank=65), dict(rank=2.5), dict(rank=True), dict(layers=0), dict(layers=3),
                                dict(layers=[0, 2]), dict(layers=[-1]), dict(layers=[]), dict(alpha=0.0)])
def test_bad_arguments_raise(kw):
    with pytest.raises(ValueError):
        lora.attach(_model(), **kw)


def test_attach_twice_and_calls_without_adapters_raise():
    model = _model()
    for fn in (lora.state_dict, lora.merge, lora.merged_state_dict):
        with pytest.raises(RuntimeError):
            fn(model)
    lora.attach(model, rank=2)
    with pytest.raises(RuntimeError):
        lora.attach(model, rank=2)


def test_state_dict_round_trip_on_a_fresh_model():
    model = _model()
    lora.attach(model, rank=4, alpha=6.0, targets=("v", "fc1"), layers=1, seed=3)
    with torch.no_grad():
        for k, p in model.lora_params.items():
            if k.endswith("lora_B__weight"):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(1)) * 0.02)
        model.P("classifier.bias").add_(0.5)
    sd = lora.state_dict(model)
    fresh = _model()
    lora.load_state_dict(fresh, sd)  # attaches from sd["lora_config"]
    back = lora.state_dict(fresh)
    assert back["lora_config"] == sd["lora_config"] and list(back) == list(sd)
    for k in sd:
        if k != "lora_config":
            assert torch.equal(back[k], sd[k]), k
    # through torch.save / load as a checkpoint entry, onto a model that already has the same adapters
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    lora.load_state_dict(fresh, torch.load(buf, weights_only=True))
    assert all(torch.equal(lora.state_dict(fresh)[k], sd[k]) for k in sd if k != "lora_config")
    # a state for other adapters is refused
    other = _model()
    lora.attach(other, rank=2)
    with pytest.raises(ValueError):
        lora.load_state_dict(other, sd)


def test_exported_from_the_package():
    import vclip_amd
    assert vclip_amd.lora is lora and "lora" in vclip_amd.__all__


def test_cli_parser_takes_the_lora_flags(golden_dir):
    p = apps.build_parser(apps.FAMILIES["vivit"], inference=False)
    a = p.parse_args(["--data_dir", "x"])
    assert (a.lora_rank, a.lora_alpha, a.lora_targets, a.lora_layers) == (0, None, "q,v", 0)
    a = p.parse_args(["--data_dir", "x", "--lora_rank", "4", "--lora_alpha", "12", "--lora_targets", "q,k,fc2",
                      "--lora_layers", "1"])
    assert (a.lora_rank, a.lora_alpha, a.lora_targets, a.lora_layers) == (4, 12.0, "q,k,fc2", 1)
    # the reference's flags are all still there with their defaults (tests/golden/cli_flags.json)
    with open(os.path.join(golden_dir, "cli_flags.json")) as f:
        ref = json.load(f)["vivit_transformer/main.py"]
    acts = {x.option_strings[0]: x for x in p._actions if x.option_strings}
    for flag, spec in ref.items():
        assert flag in acts, flag
        if "default" in spec and spec.get("action") != "store_true":
            assert acts[flag].default == spec["default"], flag
    # the other families' trainers and ViViT's inference parser do not get them
    for fam, inference in (("timesformer", False), ("swin", False), ("resnet3d", False), ("vivit", True)):
        q = apps.build_parser(apps.FAMILIES[fam], inference=inference)
        assert not any(o.startswith("--lora") for x in q._actions for o in x.option_strings), fam
