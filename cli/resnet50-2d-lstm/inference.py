"""Drop-in for the reference's `resnet50-2d-lstm/inference.py` (same flags, plus `--videos_per_batch`, `--stream_chunk`
and `--saliency {gradcam,hirescam} [--saliency_class {0,1}] [--saliency_layer {res5,res4}]`): runs on libvclip / MI355X,
several videos per forward; with `--saliency` also which frames, and where in them, produced each prediction.

    python cli/resnet50-2d-lstm/inference.py <the reference's arguments>
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vclip_amd.apps import run_inference  # noqa: E402

if __name__ == "__main__":
    run_inference("lstm")
