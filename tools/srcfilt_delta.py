#!/usr/bin/env python3
"""The figures the source-filter tests take their bars from, all measured on the integer / fp64 restatement
(tests/srcfilt_ref.py) on the CPU, never on the kernel:

  c        the restatement's overlap-added output on the synthesis test's own cases, re-run under three perturbations:
           the lag sums from the far end, the excitation energy Ee summed from the far end, and the all-pole filter's
           taps accumulated in the opposite order; per perturbation the worst |delta y| / max|y_row|, and "worst" over
           the three.  Two equally valid fp64 evaluations lie this far apart; the GPU test allows the kernel 16 x on
           top of the fp32 roundings, and 16 x worst must stay under u / 4 = 2^-26.
  near     per case, the frames near a decision, the share of samples they touch (the inputs leave out none), and the
           frames of each status.
  e2e      SourceFilter restated (tests/pitch_ref.py's YIN and ratio, seed 1) on the three 4800-sample voiced rows, at
           each row's own pitch ("own") and at 170 Hz ("170"): per row |voiced-mean F0 / wanted - 1| and the distance in
           Hz of the envelope peak near 1220 Hz from the input's; the worst of each.  The end-to-end test allows twice
           those.

    python tools/srcfilt_delta.py          # one JSON line, also written to profiles/srcfilt_delta.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speech_anonymization_amd  # noqa: E402,F401  (registers the package name)
from tests import srcfilt_ref as R  # noqa: E402


def near():
    out = {}
    for name, asp in R.SYNTH_CASES:
        ref = R.case_ref(name, asp)
        out[f"{name}_{asp:g}"] = {"near_frames": int(ref.near.sum()), "left_out_share": float(ref.left_out.mean()),
                                  "status": [int((ref.status == k).sum()) for k in range(4)]}
    return out


def e2e():
    out = {}
    for label, target in (("own", None), ("170", R.TARGET_HZ)):
        wav, y = R.e2e_restatement(target)
        f_rel, peak_hz, f_out, p_in, p_out = R.e2e_measure(wav, y, target)
        out[label] = {"f0_rel": [float(v) for v in f_rel], "peak_hz": [float(v) for v in peak_hz],
                      "f0_out_hz": [float(v) for v in f_out], "peak_in_hz": [float(v) for v in p_in],
                      "peak_out_hz": [float(v) for v in p_out], "f0_rel_worst": float(f_rel.max()),
                      "peak_hz_worst": float(peak_hz.max())}
    return out


def main():
    c = R.measure_c()
    c["worst"] = max(c.values())
    assert R.C_FACTOR * c["worst"] < R.U / 4.0, c
    res = {"c": c, "c_factor": R.C_FACTOR, "near": near(), "e2e": e2e()}
    line = json.dumps(res)
    with open(R.DELTA_FILE, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
