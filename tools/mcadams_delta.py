#!/usr/bin/env python3
"""The figures the McAdams tests take their bars from, all measured on the fp64 restatement (tests/mcadams_ref.py) on
the CPU, never on the kernel:

  C       the restatement re-run on the kernel test's cases with its own fp64 Aberth iteration in place of
          numpy.roots, and again with the autocorrelation summed from the far end: the worst |delta| / max|y| of
          the output.  Two equally valid fp64 evaluations lie this far apart; the GPU test allows the kernel 16 x.
  peaks   on tests/formant_ref.py's three-resonance rows at alpha = 0.8 and 0.6: how far the output's envelope peak
          lies from (16000 / 2 pi) phi^alpha, and its voiced-mean F0 from the input's, both relative.  The
          end-to-end test allows twice the worst.

    python tools/mcadams_delta.py          # one JSON line
"""
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import speech_anonymization_amd  # noqa: E402,F401  (registers the package name)
from tests import formant_ref as FR  # noqa: E402
from tests import mcadams_ref as M  # noqa: E402

END_TO_END_ALPHAS = (0.8, 0.6)


def conditioning():
    worst, iters, left_out, fallbacks = 0.0, 0, 0, 0
    per_case = {}
    for name, wav, alpha, nv in M.gpu_cases():
        for level in (True, False):
            ref = M.case_ref(name, level)
            ab = M.mcadams(wav, alpha, nv, level, roots=M.aberth)
            rv = M.mcadams(wav, alpha, nv, level, reverse_acf=True)
            assert (ab.status == ref.status).all() and (rv.status == ref.status).all(), name
            peak = np.abs(ref.out).max(1, keepdims=True)
            peak[peak == 0.0] = 1.0
            d = max(float((np.abs(ab.out - ref.out) / peak).max()), float((np.abs(rv.out - ref.out) / peak).max()))
            per_case[f"{name}/{int(level)}"] = d
            worst, iters = max(worst, d), max(iters, ab.iters)
            left_out += int(ref.left_out.sum())
            fallbacks += int((ref.status == M.FALLBACK).sum())
    return {"C": worst, "per_case": per_case, "aberth_iterations": iters, "left_out": left_out,
            "fallback_frames": fallbacks}


def end_to_end():
    rows = FR.resonance_rows().numpy()
    B, N = rows.shape
    f0_in = FR.voiced_f0(rows)[0].numpy()
    peak_rel, f0_rel, detail = 0.0, 0.0, []
    for alpha in END_TO_END_ALPHAS:
        out = M.mcadams(rows, np.full(B, alpha, np.float32), np.full(B, N, np.int32), True)
        assert (out.status == M.OK).all()
        want_all = np.array([M.expected_peak(F, alpha) for _, F in FR.ROWS])
        peaks = M.envelope_peak_near(out.out, want_all)
        glob = FR.envelope_peak(out.out).numpy()
        f0 = FR.voiced_f0(out.out)[0].numpy()
        for b, (_, F) in enumerate(FR.ROWS):
            want = float(want_all[b])
            peak_rel = max(peak_rel, abs(peaks[b] / want - 1.0))
            f0_rel = max(f0_rel, abs(f0[b] / f0_in[b] - 1.0))
            detail.append({"alpha": alpha, "F": F, "expected_hz": want, "peak_hz": float(peaks[b]), "highest_peak_hz": float(glob[b]),
                           "f0_in": float(f0_in[b]), "f0_out": float(f0[b])})
    return {"peak_rel": peak_rel, "f0_rel": f0_rel, "rows": detail}


def main():
    out = conditioning()
    out.update(end_to_end())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
