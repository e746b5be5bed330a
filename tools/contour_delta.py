#!/usr/bin/env python3
"""What the F0-contour pitch modification does to a contour that moves (the bars of
tests/test_contour_gpu.py's end-to-end tests): the fp64 restatement of tests/contour_ref.py on the CPU over a glide
(110 -> 190 Hz) and a vibrato row (150 +- 25 Hz at 3 Hz), 1.5 s each.  Frames voiced in both the input and the output
are counted, the first and the last three left out.  Prints, and returns as {gamma: {figure: [glide, vibrato]}}:

  gamma 0        the output's voiced-F0 standard deviation (std_out, against std_in) and |mean - target| (mean_err)
  gamma 0.5, 1   the worst per-frame |f0_out - (target + gamma (f0_in - mean_in))| (worst)

With ``--preserve_formants`` also the glide row at gamma 0 through the envelope warp (beta = 1): its F0 standard
deviation and the displacement of its cepstral-envelope peak from the input's, in Hz.

    python tools/contour_delta.py [target_hz] [--preserve_formants]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import contour_ref as Cr  # noqa: E402
from tests import formant_ref as F  # noqa: E402
from tests import pitch_ref as P  # noqa: E402


def preserved(target=170.0, report=print):
    """the glide row at gamma 0 with beta = 1 -> (F0 std in, F0 std out, |mean - target|, peak displacement in Hz)"""
    wav, lens = Cr.case_rows()[:1], torch.ones(1)
    N = wav.shape[1]
    out = Cr.normalize(wav, lens, target, 0.0, beta=1.0)[0]
    _, std_in, _ = Cr.f0_stats(P.yin(wav.double())[0], lens, N)
    mean, std, _ = Cr.f0_stats(P.yin(out)[0], lens, N)
    move = float((F.envelope_peak(out) - F.envelope_peak(wav)).abs()[0])
    report(f"preserve_formants, gamma 0, glide: f0 std {float(std_in[0]):.2f} -> {float(std[0]):.3f} Hz, mean "
           f"{float(mean[0]):.3f} Hz, envelope peak displaced by {move:.2f} Hz")
    return float(std_in[0]), float(std[0]), abs(float(mean[0]) - target), move


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    target = float(args[0]) if args else 170.0
    with torch.no_grad():
        res = Cr.delta_cases(target, report=lambda line: print(line, flush=True))
        if "--preserve_formants" in argv:
            res["preserve_formants"] = preserved(target)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
