#!/usr/bin/env python3
"""The figures the mel-cepstral distortion tests take their bars from, all measured on the fp64 restatement
(tests/mcd_ref.py) on the CPU, never on the kernel.

The kernel test's cases (mcd_ref.gpu_cases()) are re-evaluated with four perturbations:

      cep32      the cepstra rounded to fp32
      cos32      the cosine table rounded to fp32
      sum32      the sum over the coefficients, the additions of the recurrence and the frame-synchronous sum in fp32
      reverse    the sum over the coefficients from the far end

and the worst |delta| per output is reported (``worst``); frames has to come out the same.  The waveform-level case
(mcd_ref.wave_case(), through mcd_ref.log_mel) is re-evaluated with the same four and with the log-Mel front end in
fp32 (``front32``: window, transform, power, Mel filters and logarithm), which gives ``worst_wave``.  The GPU tests
allow 16 x these plus 2^-24 |ref|.

    python tools/mcd_delta.py          # one line per case, then one JSON line
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import mcd_ref as R  # noqa: E402


def measure_cases(report=print):
    worst = {k: 0.0 for k in R.OUTPUTS}
    by = {key: {k: 0.0 for k in R.OUTPUTS} for key in R.PERTURBATIONS}
    for name, ref, deg, n_ref, n_deg, order, band in R.gpu_cases():
        base = R.case_ref(name)
        row = {}
        for key, kw in R.PERTURBATIONS.items():
            p = R.score(ref, deg, n_ref, n_deg, order, band, **kw)
            assert (p.frames == base.frames).all(), (name, key)
            for k in R.OUTPUTS:
                d = float(np.abs(getattr(p, k) - getattr(base, k)).max())
                row[f"{key}_{k}"] = d
                by[key][k] = max(by[key][k], d)
                worst[k] = max(worst[k], d)
        report(f"{name}: frames {base.frames.tolist()} " + " ".join(f"{k} {v:.3e}" for k, v in row.items()))
    return worst, by


def measure_wave(report=print):
    base = R.wave_ref()
    worst, by = {k: 0.0 for k in R.OUTPUTS}, {}
    variants = dict({key: (False, kw) for key, kw in R.PERTURBATIONS.items()}, front32=(True, {}))
    for key, (fp32, kw) in variants.items():
        p = R.wave_ref(fp32, **kw)
        assert (p.frames == base.frames).all(), key
        by[key] = {k: float(np.abs(getattr(p, k) - getattr(base, k)).max()) for k in R.OUTPUTS}
        for k in R.OUTPUTS:
            worst[k] = max(worst[k], by[key][k])
        report(f"wave {key}: " + " ".join(f"{k} {v:.3e}" for k, v in by[key].items()))
    return worst, by, {k: getattr(base, k).tolist() for k in R.OUTPUTS + ("frames",)}


def main():
    say = lambda line: print(line, flush=True)
    worst, by = measure_cases(say)
    worst_wave, by_wave, wave = measure_wave(say)
    print(json.dumps({"worst": worst, "worst_wave": worst_wave, "factor": R.BAR_FACTOR, "by_perturbation": by,
                      "by_perturbation_wave": by_wave, "wave": wave}))


if __name__ == "__main__":
    main()
