"""Entrypoint with the reference's path (reference SingleModels/audio_nn.py): `python SingleModels/audio_nn.py --batch_size 8 --synthetic 16 --audio-seconds 3,8`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tav_amd  # noqa: E402,F401
from tav_amd.SingleModels.audio_nn import main, prepare_dataloader, runModel  # noqa: E402,F401

if __name__ == "__main__":
    main()
