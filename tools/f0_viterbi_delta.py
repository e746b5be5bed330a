#!/usr/bin/env python3
"""What the Viterbi F0 tracker changes against first-dip YIN, and how firmly: the restatement
tests/f0v_ref.py on the scenario signals (weak fundamental, noise burst, glide, 320 Hz row, white noise, silence;
N = 6277, T = 40), on the CPU, from the fp64 d' of tests/pitch_ref.py rounded to fp32.

Per signal it prints both tracks, then
  moved     on how many of --trials random rescalings of d' -- every element by its own factor in [1 - eps, 1 + eps],
            eps = 4e-5 (section 15's bound of the fp32 kernel's d' against the exact one is (W + tau_max + 8) 2^-24 =
            4.02e-5) -- the decoded path (the chosen LAGS, which is what the f0 is made of) differs from the unscaled
            one;
  gap       the cost gap between the best and the second-best final state of the unscaled decode, in units of 2^-16.
The GPU scenario test rests on ``moved`` being 0 for every signal: the GPU's d' is such a rescaling of this one.
Prints one JSON line last; main() returns the same dict."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

EPS = 4e-5


def main(argv=None):
    from tests import f0v_ref as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args(argv)
    dp = R.dprime32(R.scenario_rows())
    ones = np.ones(len(R.SCENARIOS))
    f0_v, path, tau, q = R.track(dp, ones, R.N_CASE)
    f0_y, _ = R.yin_f0(dp)
    lags = R.lags_of(tau, path)
    LOG, wq = R.log_table(), R.weights_q()
    g = np.random.default_rng(a.seed)
    moved = np.zeros(len(R.SCENARIOS), dtype=np.int64)
    for _ in range(a.trials):
        scaled = (dp.astype(np.float64) * g.uniform(1.0 - EPS, 1.0 + EPS, size=dp.shape)).astype(np.float32)
        _, p2, t2, _ = R.track(scaled, ones, R.N_CASE)
        moved += (R.lags_of(t2, p2) != lags).any(-1)
    out = {"N": R.N_CASE, "T": R.T_CASE, "eps": EPS, "trials": a.trials, "weights_q": list(wq), "signals": {}}
    for b, (name, _) in enumerate(R.SCENARIOS):
        _, costs = R.decode_row(tau[b].tolist(), q[b].tolist(), R.T_CASE, wq, LOG, return_costs=True)
        gap = costs[1] - costs[0] if len(costs) > 1 else None
        voiced_v, voiced_y = int((f0_v[b] > 0).sum()), int((f0_y[b] > 0).sum())
        differ = int((f0_v[b] != f0_y[b]).sum())
        print(f"{name}:")
        print("  yin      " + " ".join(f"{v:.0f}" for v in f0_y[b]))
        print("  viterbi  " + " ".join(f"{v:.0f}" for v in f0_v[b]))
        print(f"  voiced frames {voiced_y} -> {voiced_v}, frames that differ {differ}, path moved on {int(moved[b])} of "
              f"{a.trials} rescalings, final cost gap {gap}")
        out["signals"][name] = {"voiced_yin": voiced_y, "voiced_viterbi": voiced_v, "frames_differ": differ,
                                "moved": int(moved[b]), "final_gap_q16": gap}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
