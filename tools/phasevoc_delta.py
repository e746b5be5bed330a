#!/usr/bin/env python3
"""How far the mean F0 of an utterance pitch-normalised with the phase vocoder lies from the target (DESIGN section
19; the bar of tests/test_phasevoc_gpu.py's end-to-end test): the fp64 restatement of tests/phasevoc_ref.py on the
CPU over the 16 utterances tools/pitch_norm_delta.py uses (4 batches of 4 of data.synthetic_gender_dataset, 1 s
each).  No phase seeds: the path draws no random numbers.  Prints each utterance, then one line with the worst
|mean - target|, the smallest voiced share and the largest phase distance between two summation orders of the
carried phase (the recurrence reduced mod 1 per step against one cumulative sum).

    python tools/phasevoc_delta.py [target_hz]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import phasevoc_ref as V  # noqa: E402


def main(argv):
    target = float(argv[0]) if argv else 170.0
    worst, low, spread = V.delta_cases(target, report=lambda line: print(line, flush=True))
    print(f"worst |mean - target| {worst:.4f} Hz over 16 utterances; smallest voiced share {low:.3f}; "
          f"phase spread between two summation orders {spread:.2e} turns")


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1:])
