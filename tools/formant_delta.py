#!/usr/bin/env python3
"""How well the formant-preserving pitch normalisation and the formant shift keep what they promise (DESIGN section
16; the bars of tests/test_formant_gpu.py's end-to-end tests): the fp64 restatement of tests/formant_ref.py on the CPU
over the three resonance rows (f0, F) = (125, 2200), (230, 1200), (210, 2600) Hz, 32 Griffin-Lim iterations, phase
seeds 0..2.  Prints per case the voiced-mean F0, the envelope peak and the voiced share, then the worst F0 error and
the worst peak displacement of the plain path, of preserve_formants and of formant_ratio 0.85 and 1.2.

    python tools/formant_delta.py [target_hz]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speech_anonymization_amd import vocoder  # noqa: E402
from tests import formant_ref as F  # noqa: E402


def main(argv):
    target = float(argv[0]) if argv else 170.0
    wav = F.resonance_rows()
    lens = torch.ones(wav.shape[0])
    f0_in, share_in = F.voiced_f0(wav)
    peak_in = F.envelope_peak(wav)
    print("input: f0", [f"{x:.2f}" for x in f0_in.tolist()], "peak", [f"{x:.1f}" for x in peak_in.tolist()],
          "voiced share", [f"{x:.2f}" for x in share_in.tolist()], flush=True)
    worst = {}

    def note(name, seed, out, f0_ref, peak_ref):
        f0, share = F.voiced_f0(out)
        peak = F.envelope_peak(out)
        df, dp = (f0 - f0_ref).abs(), (peak - peak_ref).abs()
        print(f"{name} seed {seed}: f0 {[f'{x:.2f}' for x in f0.tolist()]} peak {[f'{x:.1f}' for x in peak.tolist()]} "
              f"share {[f'{x:.2f}' for x in share.tolist()]} |df0| {float(df.max()):.3f} |dpeak| {float(dp.max()):.2f}",
              flush=True)
        w = worst.setdefault(name, [0.0, 0.0, 1.0])
        w[0], w[1], w[2] = max(w[0], float(df.max())), max(w[1], float(dp.max())), min(w[2], float(share.min()))

    tgt = torch.full_like(f0_in, target)
    for seed in range(3):
        phi = lambda: (lambda gl: (lambda s: gl.draw_phase(s).double()))(vocoder.GriffinLim(seed=seed))
        out, r = F.normalize(wav, lens, phi(), beta=None, target_hz=target)
        note("plain (peak against r x input)", seed, out, tgt, r * peak_in)
        out, _ = F.normalize(wav, lens, phi(), beta=1.0, target_hz=target)
        note("preserve_formants", seed, out, tgt, peak_in)
        for beta in (0.85, 1.2):
            out = F.formant_shift(wav, lens, phi(), beta)
            note(f"formant_ratio {beta}", seed, out, f0_in, beta * peak_in)
    for name, (df, dp, share) in worst.items():
        print(f"{name}: worst |f0 - expected| {df:.3f} Hz, worst |peak - expected| {dp:.2f} Hz, smallest voiced share "
              f"{share:.3f}")


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1:])
