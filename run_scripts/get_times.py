"""Entrypoint with the reference's file name (reference run_scripts/get_times.py): utterance times by CTC forced alignment on the device."""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import tav_amd  # noqa: E402,F401
from tav_amd.run_scripts.get_times import (LABELS, SAMPLE_RATE, Point, Segment, align_batch, backtrack, get_times, get_trellis,  # noqa: E402,F401
                                           merge_repeats, transcript_tokens)
