"""Drop-in for the reference's `vivit_transformer/main.py` (same flags): runs on libvclip / MI355X.

    python cli/vivit_transformer/main.py <the reference's arguments>

Beyond the reference: `--lora_rank R [--lora_alpha A] [--lora_targets q,v] [--lora_layers N]` trains rank-R LoRA
adapters and the classifier on a frozen base (vclip_amd/lora.py); the checkpoint's `model_state_dict` has the
adapters folded in, and `lora_state_dict` / `lora_config` carry them on their own.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vclip_amd.apps import run_main  # noqa: E402

if __name__ == "__main__":
    run_main("vivit")
