#!/usr/bin/env python3
"""What the restatement of the WSOLA path (tests/wsola_ref.py) does to the pitch, on the CPU: the
figures the one measured bar is made of.  Nothing here runs a kernel; kernel and restatement are equal in every bit, so
the restatement's figures are the kernel's.

    python tools/wsola_delta.py [--out profiles/wsola_delta.json]

  f0       the worst |mean voiced F0(out) - mean voiced F0(in)| over the resonance rows of section 16 and harmonic rows
           at 95 to 300 Hz, at tempo 0.8 and 1.25, tracked with the tracker restatement (tests/pitch_ref.py).
  tracker  the worst distance of that tracker's voiced mean of the inputs from the fundamentals the rows were generated
           at: its own resolution there.
  The bar is twice their sum."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import wsola_ref as R  # noqa: E402


def measure():
    wav, fundamentals = R.f0_rows()
    mean_in = R.voiced_mean(wav)
    tracker = float((mean_in - torch.tensor(fundamentals, dtype=torch.float64)).abs().max())
    res = {"tempos": list(R.F0_TEMPOS), "fundamentals_hz": fundamentals, "f0_mean_in_hz": mean_in.tolist()}
    worst = 0.0
    for tempo in R.F0_TEMPOS:
        out, n_out = R.scaled(wav, tempo)
        mean_out = R.voiced_mean(out)
        rms = (out.double().pow(2).mean(1).sqrt() / wav.double().pow(2).mean(1).sqrt()).tolist()
        res[f"tempo_{tempo:g}"] = {"n_out": n_out, "f0_mean_out_hz": mean_out.tolist(), "rms_ratio": rms}
        worst = max(worst, float((mean_out - mean_in).abs().max()))
    res.update(f0_delta_hz=worst, tracker_delta_hz=tracker, f0_bar_hz=2.0 * (worst + tracker))
    return res


def main(argv):
    res = measure()
    text = json.dumps(res, indent=1) + "\n"
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1:])
