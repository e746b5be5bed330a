#!/usr/bin/env python3
"""Times the formant report (csrc/sa_formants.hip, ops.formant_tracks, ops.formant_compare) at
B = 32 utterances of 10 s: pulse trains through three resonances (tests/mcadams_ref.voiced_row, one second of each
repeated) against their own McAdams output at alpha = 0.8.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  tracks_ms, frames_per_s       sa_formant_tracks through ops.formant_tracks on the [B, N] batch: the one launch and
                                the two output allocations
  tracks_pair_ms                the same on the [2 B, N] batch metrics.formant_shift forms (the concatenation included)
  compare_ms, rows_per_s        sa_formant_compare through ops.formant_compare on the tracks of the pair
  mcadams_ms                    ops.mcadams on the same [B, N] batch in the same session, the kernel this one is
                                modelled on (its frame kernel also runs the FIR and a 320-step IIR), and
                                tracks_over_mcadams
  ref_frames_per_s              the fp64 restatement's tracks (tests/lpcformant_ref.py, numpy) on the host
  stage_track_f0_ms, stage_formants_ms, stage_to_host_ms
                                anonymize.py --report_formants true: the two F0 trackings (reports.f0_tracks on a
                                fresh window), the formant tracks and the comparison with the report's collect, and
                                the report's fetch, the one copy of the eight result rows to the host"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tools.bench_common import time_calls, write_line  # noqa: E402

SR = 16000


def voiced_rows(B, N):
    """B rows: one second of voiced_row at 100 + 4 b Hz, repeated to N samples, fp32 [B, N]"""
    from tests import lpcformant_ref as R
    rows = [np.tile(R.voiced_row(100.0 + 4.0 * b, R.FORMANTS, SR, b), -(-N // SR))[:N] for b in range(B)]
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--alpha", type=float, default=0.8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "formant_report_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    import speech_anonymization_amd  # noqa: F401  (registers the package name)
    from speech_anonymization_amd import metrics, ops, reports
    from tests import lpcformant_ref as R
    B, N = a.B, int(a.seconds * SR)
    wav, lens_cpu = voiced_rows(B, N).to(dev), torch.ones(B)
    nv = torch.full((B,), N, dtype=torch.int32, device=dev)
    alpha = torch.full((B,), a.alpha, dtype=torch.float32, device=dev)
    deg = ops.mcadams(wav, alpha, nv)[0]
    win = reports.Batch(wav, lens_cpu, deg, [N] * B).window
    f_in, f_out = reports.f0_tracks(win, "yin")
    T = int(f_in.shape[1])

    res = {"B": B, "N": N, "T": T, "alpha": a.alpha, "steps": a.steps}
    res["tracks_ms"] = round(time_calls(lambda: ops.formant_tracks(wav, nv), a.warmup, a.steps), 4)
    res["frames_per_s"] = round(B * T / res["tracks_ms"] * 1e3)
    pair = lambda: ops.formant_tracks(torch.cat((win.ref, win.deg)), torch.cat((win.nv, win.nv)))
    res["tracks_pair_ms"] = round(time_calls(pair, a.warmup, a.steps), 4)
    F, st = pair()
    cmp_ = lambda: ops.formant_compare(F[:B], F[B:], st[:B], st[B:], f_in, f_out, win.frames)
    res["compare_ms"] = round(time_calls(cmp_, a.warmup, a.steps), 4)
    res["rows_per_s"] = round(B / res["compare_ms"] * 1e3)
    res["mcadams_ms"] = round(time_calls(lambda: ops.mcadams(wav, alpha, nv), a.warmup, a.steps), 4)
    res["tracks_over_mcadams"] = round(res["tracks_ms"] / res["mcadams_ms"], 3)
    cols = [c.cpu() for c in cmp_()]
    res["scored_rows"] = int((cols[7] > 0).sum())
    res["status_counts"] = [int((st == s).sum()) for s in range(4)]
    for name, c in zip(("f1_shift_mean", "f2_shift_mean", "f3_shift_mean", "formant_shift_mean"), cols[3:7]):
        res[name] = round(float(c[cols[7] > 0].double().mean()), 6) if res["scored_rows"] else None

    row = wav[:1, :4800].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.tracks(row, np.array([4800], np.int32))
    res["ref_frames_per_s"] = round(ref.status.size / (time.perf_counter() - t0), 1)

    ids, rep = [str(i) for i in range(B)], reports.Report("report_formants", {})

    def fresh():                                            # (a fresh Window, as every batch has)
        return reports.Window(win.width, win.nv, win.ref, win.deg)

    def score():
        w = fresh()
        rep.collect(ids, metrics.formant_shift(w.ref, w.deg, w.nv, f_in, f_out, w.frames))

    for name, fn in (("stage_track_f0_ms", lambda: reports.f0_tracks(fresh(), "yin")), ("stage_formants_ms", score),
                     ("stage_to_host_ms", rep.fetch)):
        res[name] = round(time_calls(fn, a.warmup, a.steps), 4)
    write_line(res, a.out)


if __name__ == "__main__":
    main()
