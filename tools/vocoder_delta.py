#!/usr/bin/env python3
"""The scale on which two Griffin-Lim trajectories differ (the bars of tests/test_vocoder_gpu.py):
the fp64 restatement of that test file on its own signals, 32 iterations, phase seeds 0..7, on the CPU.  Prints the
batch-mean spectral convergence with true STFT magnitudes and the feature round trip's mean |dB| error per seed, and
for each delta = (max - min) / min.

    python tools/vocoder_delta.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speech_anonymization_amd import vocoder  # noqa: E402
from tests import test_vocoder_gpu as R  # noqa: E402


def main():
    sig = R.signals().astype(np.float64)
    S = np.abs(R.ref_stft(sig)[0]).astype(np.float32).astype(np.float64)
    m = R.m32()
    sc, db = [], []
    for seed in range(8):
        phi = vocoder.GriffinLim(seed=seed).draw_phase(S.shape).double().numpy()
        sc.append(float(R.ref_sc(R.ref_loop(S, phi, R.N_ITER, m), S).mean()))
        db.append(R.ref_round_trip(sig, phi, R.N_ITER, m))
        print(f"seed {seed}: spectral convergence {sc[-1]:.5f}; round trip mean |dB| {db[-1][0]:.4f}, "
              f"95th percentile {db[-1][1]:.2f}", flush=True)
    phi = vocoder.GriffinLim(seed=0).draw_phase(S.shape).double().numpy()
    print(f"0 iterations: spectral convergence {float(R.ref_sc(R.ref_loop(S, phi, 0, m), S).mean()):.4f}")
    means = [d[0] for d in db]
    print(f"delta, true magnitudes: {(max(sc) - min(sc)) / min(sc):.4f}  ({min(sc):.5f} .. {max(sc):.5f})")
    print(f"delta, round trip: {(max(means) - min(means)) / min(means):.4f}  ({min(means):.4f} .. {max(means):.4f})")


if __name__ == "__main__":
    main()
