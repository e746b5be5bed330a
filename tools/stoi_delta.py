#!/usr/bin/env python3
"""The figures the STOI tests take their bar from, all measured on the fp64 restatement (tests/stoi_ref.py) on the
CPU, never on the kernel.  The kernel test's cases are re-evaluated with four perturbations:

  a   the resampled signals rounded to fp32
  b   the band magnitudes rounded to fp32
  c   the DFT as a direct sum in reverse order instead of numpy.fft
  d   the frame energies summed from the far end

and the worst |delta score| per measure is reported, with every case's own figures, the smallest distance of a frame
energy from its row's threshold, and the kept-frame counts.  The GPU test allows the kernel 16 x the worst value plus
2^-24 |ref|; the bar has to stay at or below 1e-4.

    python tools/stoi_delta.py          # one JSON line
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import speech_anonymization_amd  # noqa: E402,F401  (registers the package name)
from tests import stoi_ref as R  # noqa: E402

PERTURBATIONS = {"a": dict(x10_fp32=True), "b": dict(bands_fp32=True), "c": dict(direct_dft=True),
                 "d": dict(reverse_energy=True)}


def main():
    worst = {"stoi": 0.0, "estoi": 0.0}
    per_case, margin = {}, float("inf")
    for name, ref, deg, nv, _ in R.gpu_cases():
        base = R.case_ref(name)
        margin = min(margin, float(base.margin.min()))
        row = {"frames": base.frames.tolist(), "segments": base.segments.tolist(), "stoi": base.stoi.tolist(),
               "estoi": base.estoi.tolist()}
        for key, kw in PERTURBATIONS.items():
            p = R.stoi(ref, deg, nv, **kw)
            assert (p.frames == base.frames).all() and (p.segments == base.segments).all(), (name, key)
            for m in ("stoi", "estoi"):
                d = float(np.abs(getattr(p, m) - getattr(base, m)).max())
                row[f"{key}_{m}"] = d
                worst[m] = max(worst[m], d)
        per_case[name] = row
    bars = {m: R.BAR_FACTOR * worst[m] + R.U for m in worst}
    assert max(bars.values()) <= 1e-4, bars
    print(json.dumps({"worst": worst, "factor": R.BAR_FACTOR, "bar_at_score_1": bars, "smallest_margin": margin,
                      "per_case": per_case}))


if __name__ == "__main__":
    main()
