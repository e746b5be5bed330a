#!/usr/bin/env python3
"""Times the pitch-correlation scorer (csrc/sa_prosody.hip, ops.f0_compare) at B = 32 utterances
of 10 s: glides in the style of tests/contour_ref.py against their own --contour_scale 0.5 output.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  compare_ms, rows_per_s        sa_f0_compare through ops.f0_compare: the one launch and the six output allocations
  torch_ms                      the same computation written with torch operators in fp64 on the same GPU (a loop
                                over the 17 lags with masked sums, then the shift statistics at the chosen lag), and
                                max_abs_diff of its real outputs from sa_f0_compare's, lags_equal
  ref_rows_per_s                the fp64 restatement (tests/prosody_ref.py, numpy) on the host
  stage_track_ms, stage_compare_ms, stage_to_host_ms
                                anonymize.py --report_prosody true: the two trackings (reports.f0_tracks on the
                                window of reports.Batch), the comparison on those tracks (ops.f0_compare over the
                                window's frame counts and the report's collect, the running means) and the report's
                                fetch, the one copy of the six result rows to the host"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from tools.bench_common import time_calls, write_line  # noqa: E402

SR = 16000


def torch_compare(f_ref, f_deg, frames, max_lag=8, min_common=8):
    """the definition of include/sa_hip.h with torch operators, fp64 -> (rho, lag, common, shift_st, dev_st, voicing)"""
    B, T = f_ref.shape
    dev = f_ref.device
    x, y = f_ref.double(), f_deg.double()
    idx = torch.arange(T, device=dev)[None, :]
    F = frames.long().clamp(0, T)[:, None]
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    vx = f_ref > 0
    best = torch.full((B,), -float("inf"), dtype=torch.float64, device=dev)
    have = torch.zeros(B, dtype=torch.bool, device=dev)
    lag_of = torch.zeros(B, dtype=torch.long, device=dev)
    for k in range(2 * max_lag + 1):
        lag = -((k + 1) // 2) if k % 2 else k // 2
        j = (idx + lag).clamp(0, T - 1).expand(B, T)
        both = (idx < F) & (idx + lag >= 0) & (idx + lag < F) & vx & (f_deg.gather(1, j) > 0)
        ys = y.gather(1, j)
        n = both.sum(1)
        nn = n.clamp(min=1).double()
        dx = torch.where(both, x - (torch.where(both, x, zero).sum(1) / nn)[:, None], zero)
        dy = torch.where(both, ys - (torch.where(both, ys, zero).sum(1) / nn)[:, None], zero)
        sxx, syy, sxy = (dx * dx).sum(1), (dy * dy).sum(1), (dx * dy).sum(1)
        valid = (n >= min_common) & (sxx > 0) & (syy > 0)
        rho = sxy / torch.where(valid, sxx * syy, torch.ones_like(sxx)).sqrt()
        better = valid & (~have | (rho > best))
        best, lag_of = torch.where(better, rho, best), torch.where(better, torch.full_like(lag_of, lag), lag_of)
        have = have | valid
    l = lag_of[:, None]
    j = (idx + l).clamp(0, T - 1)
    over = (idx < F) & (idx + l >= 0) & (idx + l < F)
    vy = f_deg.gather(1, j) > 0
    both = over & vx & vy & have[:, None]
    n = both.sum(1)
    nn = n.clamp(min=1).double()
    e = torch.where(both, 12.0 * torch.log2(torch.where(both, y.gather(1, j) / x, torch.ones_like(x))), zero)
    shift = e.sum(1) / nn
    dev_st = (torch.where(both, (e - shift[:, None]) ** 2, zero).sum(1) / nn).sqrt()
    voicing = (over & (vx == vy)).sum(1).double() / over.sum(1).clamp(min=1).double()
    return torch.where(have, best, zero), lag_of, n, shift, dev_st, voicing


def glides(B, N, seed=2022):
    """B rows in the style of contour_ref.case_rows: glides between random ends in 100..220 Hz, fp32 [B, N]"""
    from tests import contour_ref as Cr
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(B):
        lo, hi = (100.0 + 120.0 * torch.rand(2, generator=g, dtype=torch.float64)).tolist()
        rows.append(Cr.glide_row(lambda t: lo + (hi - lo) * t / (N / SR), N, g))
    return torch.stack(rows).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prosody_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    import speech_anonymization_amd  # noqa: F401  (registers the package name)
    from speech_anonymization_amd import ops, pitchnorm, reports
    from tests import prosody_ref as R
    B, N = a.B, int(a.seconds * SR)
    wav, lens_cpu = glides(B, N).to(dev), torch.ones(B)
    out_wav = pitchnorm.PitchNormalizer(170.0, phase="vocoder", contour_scale=a.gamma)(wav, lens_cpu)
    win = reports.Batch(wav, lens_cpu, out_wav, [out_wav.shape[1]] * B).window
    track = lambda: reports.f0_tracks(win, "yin")
    (f_in, f_out), frames = track(), win.frames
    got = ops.f0_compare(f_in, f_out, frames)
    ms = time_calls(lambda: ops.f0_compare(f_in, f_out, frames), a.warmup, a.steps)
    tor = torch_compare(f_in, f_out, frames)
    ms_torch = time_calls(lambda: torch_compare(f_in, f_out, frames), a.warmup, a.steps)
    diff = max(float((got[i].double() - tor[i]).abs().max()) for i in (0, 3, 4, 5))
    res = {"B": B, "N": N, "T": int(f_in.shape[1]), "gamma": a.gamma, "steps": a.steps,
           "f0_corr_mean": round(float(got[0].mean()), 6), "f0_dev_st_mean": round(float(got[4].mean()), 6),
           "compare_ms": round(ms, 4), "rows_per_s": round(B / ms * 1e3), "torch_ms": round(ms_torch, 4),
           "torch_over_kernel": round(ms_torch / ms, 1), "max_abs_diff": float(f"{diff:.3e}"),
           "lags_equal": bool(torch.equal(got[1].long(), tor[1]) and torch.equal(got[2].long(), tor[2]))}

    t0 = time.perf_counter()
    ref = R.compare(f_in.cpu().numpy(), f_out.cpu().numpy(), frames.cpu().numpy())
    res["ref_rows_per_s"] = round(B / (time.perf_counter() - t0), 2)
    vs_ref = max(float(abs(got[i].double().cpu().numpy() - getattr(ref, k)).max())
                 for i, k in ((0, "rho"), (3, "shift_st"), (4, "dev_st"), (5, "voicing")))
    res["max_abs_diff_vs_ref"] = float(f"{vs_ref:.3e}")

    ids, rep = [str(i) for i in range(B)], reports.Report("report_prosody", {})

    def score():                                            # (a fresh Window forms its frame counts, as every batch does)
        fr = reports.Window(win.width, win.nv, win.ref, win.deg).frames
        rep.collect(ids, ops.f0_compare(f_in, f_out, fr, max_lag=rep.opts["prosody_max_lag"]))

    for name, fn in (("stage_track_ms", track), ("stage_compare_ms", score), ("stage_to_host_ms", rep.fetch)):
        res[name] = round(time_calls(fn, a.warmup, a.steps), 4)
    write_line(res, a.out)


if __name__ == "__main__":
    main()
