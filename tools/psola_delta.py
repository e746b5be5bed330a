#!/usr/bin/env python3
"""What the restatement of the TD-PSOLA path (tests/psola_ref.py) does, on the CPU: the figures the
tests' bars are made of.  Nothing here runs a kernel.

    python tools/psola_delta.py [--out profiles/psola_delta.json]

  ola       the largest difference between the fp32-accumulating and the fp64 overlap-add over the GPU test's inputs,
            relative to the row's largest |sample|.  The bar is 4 x that: the device's fp64 cos may round a weight the
            other way, a single-ulp effect on a sum of at most ~45 terms.
  identity  the largest |out - wav| at rho_q = 2^16 on the resonance rows and the row with an unvoiced gap (fp64).
  f0        the worst |voiced-mean F0 - target| of the output over the seven end-to-end rows and the gap row, three
            frames left out at either end; ``tracker``: the worst distance of the tracker's voiced mean from the
            fundamental the seven rows were generated at, its own resolution there.  The bar is their sum.
  peak      the worst displacement of the cepstral-envelope peak over the three resonance rows; the bar is twice that
            (section 16's margin: the measure is an argmax over bins and moves in steps).
  contour   the standard deviation of the output's F0 at contour_scale 0 on the glide and the vibrato row; the bar is
            twice the worst.  (Section 20's own bars carry four times their figures; no bar here may exceed twice its
            measured value, and the marks and the plan are exact, so the smaller factor holds.)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import contour_ref as CR  # noqa: E402
from tests import formant_ref as F  # noqa: E402
from tests import pitch_ref as P  # noqa: E402
from tests import psola_ref as R  # noqa: E402

TARGET = 170.0
E2E_F0 = (125.0, 230.0, 210.0, 95.0, 140.0, 210.0, 300.0)        # what psola_ref.end_to_end_rows are generated at


def ola_delta():
    worst = 0.0
    for wav, f0, rho_q, nv in R.kernel_cases().values():
        rows = R.tables(wav, f0, rho_q, nv)
        d = (R.psola(wav, f0, rho_q, nv, True, rows) - R.psola(wav, f0, rho_q, nv, False, rows)).abs()
        worst = max(worst, float((d / wav.abs().amax(1).double().clamp(min=1e-30)[:, None]).max()))
    return worst


def identity_delta():
    gap, gap_f0 = R.gap_row()
    res = F.resonance_rows()
    worst = 0.0
    for wav, f0 in ((res, P.yin(res.double())[0].float()), (gap, gap_f0)):
        B, N = wav.shape
        nv = torch.full((B,), N)
        out = R.psola(wav, f0, torch.full(f0.shape, R.RHO_ONE), nv)
        worst = max(worst, float((out - wav.double()).abs().max()))
    return worst


def end_to_end(target=TARGET):
    """-> (worst |mean F0 - target|, the tracker's worst distance from the generators' fundamentals, worst peak
    displacement, per-row lists of the output's mean F0 and of the peaks before and after)"""
    rows, (gap, _) = R.end_to_end_rows(), R.gap_row()
    wav = torch.cat([rows, gap])
    lens, N = torch.ones(wav.shape[0]), wav.shape[1]
    out, _, f0_in = R.normalize(wav, lens, target)
    mean_in = R.voiced_mean_f0(f0_in, lens, N)
    mean_out = R.voiced_mean_f0(P.yin(out)[0], lens, N)
    peak_in, peak_out = F.envelope_peak(wav[:3]), F.envelope_peak(out[:3])
    tracker = float((mean_in[:7] - torch.tensor(E2E_F0, dtype=torch.float64)).abs().max())
    return (float((mean_out - target).abs().max()), tracker, float((peak_out - peak_in).abs().max()),
            mean_out.tolist(), peak_in.tolist(), peak_out.tolist())


def contour(target=TARGET):
    """-> (std of the output's F0 at gamma 0 per row, std of the input's, |mean - target| per row)"""
    wav, lens = CR.case_rows(), torch.ones(2)
    N = wav.shape[1]
    out, _, f0_in = R.normalize(wav, lens, target, gamma=0.0)
    mean, std, _ = CR.f0_stats(P.yin(out)[0], lens, N)
    return std.tolist(), CR.f0_stats(f0_in, lens, N)[1].tolist(), (mean - target).abs().tolist()


def measure():
    f0_worst, tracker, peak_worst, mean_out, peak_in, peak_out = end_to_end()
    std_out, std_in, mean_err = contour()
    ola = ola_delta()
    return {"target_hz": TARGET,
            "ola_delta": ola, "ola_bar": 4.0 * ola,
            "identity_delta": identity_delta(),
            "f0_delta_hz": f0_worst, "tracker_delta_hz": tracker, "f0_bar_hz": f0_worst + tracker,
            "f0_mean_out_hz": mean_out,
            "peak_in_hz": peak_in, "peak_out_hz": peak_out, "peak_delta_hz": peak_worst, "peak_bar_hz": 2.0 * peak_worst,
            "contour_std_in_hz": std_in, "contour_std_out_hz": std_out, "contour_mean_err_hz": mean_err,
            "contour_bar_hz": 2.0 * max(std_out)}


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
