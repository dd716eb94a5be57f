"""vclip_amd — MI355X-native video-clip classification hot path.

Frame sampling (host, bit-exact with the reference samplers) -> frame gather/normalise
-> tubelet embedding -> joint space-time attention encoder -> classifier head, with
every device op a hand-written HIP kernel for gfx950 behind the C-ABI in
include/vclip.h (libvclip.so).  See DESIGN.md.
"""
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(PKG_DIR)

__all__ = ["PKG_DIR", "REPO_ROOT", "faithfulness", "perturbation_curve", "PerturbationCurve", "rise_map",
           "RiseExplanation", "lora"]


def __getattr__(name):
    """The saliency faithfulness test (vclip_amd/faithfulness.py) and RISE saliency (vclip_amd/rise.py), imported on
    first use: importing the package itself loads neither torch nor the library."""
    if name in ("faithfulness", "perturbation_curve", "PerturbationCurve"):
        import importlib
        mod = importlib.import_module(".faithfulness", __name__)
        return mod if name == "faithfulness" else getattr(mod, name)
    if name in ("rise_map", "RiseExplanation"):
        import importlib
        return getattr(importlib.import_module(".rise", __name__), name)
    if name == "lora":  # LoRA fine-tuning of ViViT (vclip_amd/lora.py)
        import importlib
        return importlib.import_module(".lora", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
