"""ResNet50-LSTM (vclip_amd/resnet50_lstm.py), the parts that need no GPU: the state dict speaks the
reference's names (resnet50-2d-lstm/src/models/model.py), checkpoints round-trip, the trainable set
is the reference's (LSTM + classifier; frozen backbone), CPU tensors are refused, and the C entry
points of csrc/lstm.hip are declared and bound."""
import pytest
import torch

from vclip_amd import _lib
from vclip_amd.resnet50_lstm import VideoResNet50LSTM, create_model
from vclip_amd.weights import resnet50_lstm_param_shapes

LSTM_ENTRIES = ("vc_frame_avgpool", "vc_lstm_seq_fwd", "vc_lstm_seq_bwd", "vc_mlp_head_fwd", "vc_mlp_head_bwd",
                "vc_bn_apply_h16", "vc_video_to_cl_h16")


@pytest.fixture(scope="module")
def models():
    return {(h, l): create_model(h, l, 0.5, device=None, weights_seed=0) for h, l in ((256, 2), (64, 3))}


@pytest.mark.parametrize("hidden,layers", [(256, 2), (64, 3)])
def test_state_dict_matches_reference_names(models, hidden, layers):
    sd = models[(hidden, layers)].state_dict()
    want = resnet50_lstm_param_shapes(hidden, layers)
    assert list(sd.keys()) == list(want.keys())
    for n, shp in want.items():
        assert tuple(sd[n].shape) == tuple(shp), n
    assert any(float(v.abs().sum()) > 0 for n, v in sd.items() if n.startswith("lstm."))


def test_checkpoint_round_trip(models, tmp_path):
    m = models[(64, 3)]
    path = tmp_path / "ckpt.pt"
    torch.save({"module." + k: v for k, v in m.state_dict().items()}, path)  # a DataParallel-style checkpoint
    sd = torch.load(path)
    sd["module.resnet50.1.num_batches_tracked"] = torch.tensor(7)
    m2 = VideoResNet50LSTM(64, 3, 0.5)
    missing, unexpected = m2.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    a, b = m.state_dict(), m2.state_dict()
    assert list(a.keys()) == list(b.keys())
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_loads_torch_lstm_and_classifier_modules(models):
    """lstm.* / classifier.* straight from torch's own modules, as the reference builds them."""
    hidden, layers = 64, 3
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(2048, hidden, num_layers=layers, batch_first=True, dropout=0.5)
    cls = torch.nn.Sequential(torch.nn.Linear(hidden, 64), torch.nn.ReLU(), torch.nn.Dropout(0.5), torch.nn.Linear(64, 1))
    sd = {k: v for k, v in models[(hidden, layers)].state_dict().items() if k.startswith("resnet50.")}
    sd.update({"lstm." + k: v for k, v in lstm.state_dict().items()})
    sd.update({"classifier." + k: v for k, v in cls.state_dict().items()})
    m = VideoResNet50LSTM(hidden, layers, 0.5)
    m.load_state_dict(sd, strict=True)
    got = m.state_dict()
    assert torch.equal(got["lstm.weight_hh_l2"], lstm.weight_hh_l2.detach())
    assert torch.equal(got["classifier.3.bias"], cls[3].bias.detach())
    with pytest.raises(KeyError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "lstm.bias_hh_l1"}, strict=True)


def test_trainable_parameters_are_lstm_and_classifier(models):
    m = models[(256, 2)]
    trainable = [p for p in m.parameters() if p.requires_grad]
    frozen = [p for p in m.parameters() if not p.requires_grad]
    assert len(trainable) == 4 * 2 + 4  # per layer w_ih, w_hh, b_ih, b_hh; the head's two Linears
    assert sum(p.numel() for p in trainable) == sum(
        int(torch.tensor(s).prod()) for n, s in resnet50_lstm_param_shapes(256, 2).items() if not n.startswith("resnet50."))
    assert len(frozen) == len(list(m.backbone.parameters())) and all(not p.requires_grad for p in m.backbone.parameters())
    m.train()  # model.train() does not thaw the backbone
    assert all(not p.requires_grad for p in m.backbone.parameters())
    m.eval()


def test_cpu_tensor_is_refused(models):
    with pytest.raises(RuntimeError, match="GPU only"):
        models[(256, 2)](torch.zeros(1, 3, 2, 64, 64))


def test_unsupported_hidden_is_refused():
    for h in (0, 30, 1028):
        with pytest.raises(ValueError, match="hidden_size"):
            VideoResNet50LSTM(h, 1, 0.0)


def test_lstm_entry_points_declared_and_bound():
    names = _lib.header_functions()
    for n in LSTM_ENTRIES:
        assert n in names, f"{n} not declared in vclip.h"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
