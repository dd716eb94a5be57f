"""vivit_transformer/main.py --lora_rank end to end on the GPU, on tiny raw uint8 clips (.npy) in the reference's
<root>/{train,val,test}/{class}/ layout (as tests/test_cli_gpu.py): two epochs of LoRA fine-tuning on the last
layer, the checkpoint's three LoRA entries with the adapters folded into model_state_dict, inference.py on that
checkpoint, and a seeded rerun that reproduces the history and the adapters bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vclip_amd import _lib as L
    L.load()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("clips")
    rng = np.random.RandomState(0)
    for split, n in (("train", 2), ("val", 1), ("test", 1)):
        for c in ("non-referral", "referral"):
            d = root / split / c
            d.mkdir(parents=True)
            for k in range(n):
                np.save(d / f"{c}_{split}_{k}.npy", rng.randint(0, 256, (36, 224, 224, 3)).astype(np.uint8))
    return root


def _train(dataset, out):
    from vclip_amd.apps import run_main
    m, history, exp = run_main("vivit", ["--data_dir", str(dataset), "--log_dir", str(out / "logs"), "--model_dir",
                                         str(out / "models"), "--epochs", "2", "--batch_size", "2", "--num_workers", "0",
                                         "--lora_rank", "4", "--lora_layers", "1", "--seed", "7"])
    return history, torch.load(out / "models" / "best_model_uniform.pth", weights_only=True, map_location="cpu")


def test_lora_main_checkpoint_inference_and_rerun(dataset, tmp_path):
    from vclip_amd.apps import run_inference
    from vclip_amd.weights import vivit_param_shapes
    history, ck = _train(dataset, tmp_path / "a")
    assert len(history["train_loss"]) == 2 and all(np.isfinite(history["train_loss"] + history["val_loss"]))
    for k in ("model_state_dict", "lora_state_dict", "lora_config", "optimizer_state_dict", "config", "id2label"):
        assert k in ck
    assert ck["lora_config"] == {"rank": 4, "alpha": 8.0, "targets": ["q", "v"], "layers": [11], "train_head": True}
    lsd = ck["lora_state_dict"]
    assert lsd["lora_config"] == ck["lora_config"]
    assert sorted(k for k in lsd if "lora_" in k and k != "lora_config") == sorted(
        f"vivit.layers.11.attention.{p}_proj.lora_{ab}.weight" for p in "qv" for ab in "AB")
    assert lsd["vivit.layers.11.attention.v_proj.lora_B.weight"].abs().sum() > 0  # it trained
    # model_state_dict is an ordinary full ViViT state dict with the adapters folded in
    msd = ck["model_state_dict"]
    from vclip_amd.vivit import VivitConfig
    shapes = vivit_param_shapes(VivitConfig.from_dict(ck["config"]).as_shape_cfg())
    assert {k: tuple(v.shape) for k, v in msd.items()} == {k: tuple(v) for k, v in shapes.items()}
    from vclip_amd.weights import make_vivit_weights
    base = make_vivit_weights(VivitConfig.from_dict(ck["config"]).as_shape_cfg(), seed=0)
    s = ck["lora_config"]["alpha"] / ck["lora_config"]["rank"]
    for p in ("q_proj", "v_proj"):
        pre = f"vivit.layers.11.attention.{p}"
        delta = s * lsd[pre + ".lora_B.weight"].double() @ lsd[pre + ".lora_A.weight"].double()
        assert float(delta.abs().max()) > 0
        # create_model's seeded base weight plus the delta, to fp32 rounding
        err = (msd[pre + ".weight"].double() - (torch.from_numpy(base[pre + ".weight"]).double() + delta)).abs().max()
        assert float(err) < 1e-6, (p, float(err))
    for k in ("vivit.layers.0.attention.q_proj.weight", "vivit.layers.11.mlp.fc1.weight"):  # frozen: untouched
        assert torch.equal(msd[k], torch.from_numpy(base[k])), k
    # inference.py reads it as any checkpoint
    video = sorted((dataset / "test" / "referral").iterdir())[0]
    res = run_inference("vivit", ["--video_path", str(video), "--model_path", str(tmp_path / "a" / "models" /
                                                                                 "best_model_uniform.pth"),
                                  "--log_dir", str(tmp_path / "ilogs")])
    assert res["predicted_class"] in ("non-referral", "referral") and 0.5 <= res["confidence"] <= 1.0
    # a seeded rerun: the same history and adapters, bit for bit
    history2, ck2 = _train(dataset, tmp_path / "b")
    assert history2 == history
    for k, v in lsd.items():
        if k != "lora_config":
            assert torch.equal(v, ck2["lora_state_dict"][k]), k
    assert all(torch.equal(v, ck2["model_state_dict"][k]) for k, v in msd.items())
