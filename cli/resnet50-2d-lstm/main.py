"""Drop-in for the reference's `resnet50-2d-lstm/main.py` (same flags): runs on libvclip / MI355X.

    python cli/resnet50-2d-lstm/main.py <the reference's arguments>

Beyond the reference: `--tbptt_chunk N` trains and validates on every frame of every video, the videos of a
batch in lockstep rounds of <= N frames with the LSTM state carried (truncated backpropagation through time).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vclip_amd.apps import run_main  # noqa: E402

if __name__ == "__main__":
    run_main("lstm")
