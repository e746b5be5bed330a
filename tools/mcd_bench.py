#!/usr/bin/env python3
"""Times the mel-cepstral distortion scorer (csrc/sa_mcd.hip, ops.mcd) at B = 32 utterances of
T = 1001 frames (10 s), n_mels 80, order 13, at the bands 16 and 63: log-Mel-like fields in the style of
tests/mcd_ref.py against their warped copies.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  band16_ms, band63_ms, rows_per_s_16, rows_per_s_63
                                sa_mcd through ops.mcd: the three launches, the outputs and the workspace allocation
  torch16_ms, torch63_ms        the same recurrence written with torch operators in fp64 on the same GPU: the cepstra
                                by a matrix product, the band of distances offset by offset, then one anti-diagonal
                                per step (the median of --torch_steps calls), and max_abs_diff of its two figures from
                                sa_mcd's
  ref_rows_per_s                the fp64 restatement (tests/mcd_ref.py, numpy) on the host at band 16, over --ref_rows
                                rows, and max_abs_diff_vs_ref over them
  stage_fbank_ms, stage_score_ms, stage_to_host_ms
                                anonymize.py --report_mcd true at 32 x 10 s: the two feature passes with their clamp
                                (metrics.log_mels on the window of reports.Batch), the scoring on those spectra (the
                                two steps that metrics.mel_cepstral_distortion takes after them, frame_counts and
                                ops.mcd, and the report's collect, the running means) and the report's fetch, the one
                                copy of the three result rows to the host"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tools.bench_common import time_calls, write_line  # noqa: E402

SR, HOP = 16000, 160


def torch_mcd(mel_ref, mel_deg, n_ref, n_deg, order, band):
    """the definition of include/sa_hip.h with torch operators, fp64, one anti-diagonal per step -> (mcd, mcd_sync)"""
    dev = mel_ref.device
    B, T_ref, n_mels = mel_ref.shape
    T_deg, R, W = mel_deg.shape[1], band, 2 * band + 1
    m = torch.arange(n_mels, dtype=torch.float64, device=dev)[:, None]
    k = torch.arange(1, order + 1, dtype=torch.float64, device=dev)[None, :]
    C = torch.cos(torch.pi * k * (m + 0.5) / n_mels) / n_mels
    cr, cd = mel_ref.double() @ C, mel_deg.double() @ C
    N, M = n_ref.long().clamp(0, T_ref)[:, None], n_deg.long().clamp(0, T_deg)[:, None]
    # the band of distances: D[b, i, q] = d(i, i + q - R), 0 where j falls outside the input
    cdp = torch.nn.functional.pad(cd, (0, 0, R, R + max(T_ref - T_deg, 0)))
    D = torch.stack([(0.5 * ((cr - cdp[:, q:q + T_ref]) ** 2).sum(-1)).sqrt() for q in range(W)], dim=2)
    o = torch.arange(-R, R + 1, device=dev)[None, :]
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    g1 = g2 = torch.full((B, W), float("inf"), dtype=torch.float64, device=dev)
    out = torch.zeros(B, dtype=torch.float64, device=dev)
    rows = torch.arange(B, device=dev)[:, None]
    pad = inf.expand(B, 1)
    for s in range(T_ref + T_deg - 1):
        i2 = s - o                                              # 2 i
        i, j = i2 // 2, (s + o) // 2
        cell = (i2 % 2 == 0) & (i >= 0) & (i < N) & (j >= 0) & (j < M)
        d = D[rows, i.clamp(0, T_ref - 1).expand(B, W), (o + R).expand(B, W)]
        step = torch.minimum(torch.cat([g1[:, 1:], pad], 1), torch.cat([pad, g1[:, :-1]], 1)) + d
        g = torch.minimum(g2 + 2.0 * d, step) if s else 2.0 * d
        g = torch.where(cell, g, inf)
        last = (N + M - 2 == s) & (o == M - N)
        out = out + torch.where(last & cell, g, torch.zeros_like(g)).sum(1)
        g2, g1 = g1, g
    L = torch.minimum(N, M)
    t = torch.arange(T_ref, device=dev)[None, :]
    sync = torch.where(t < L, D[:, :, R], torch.zeros_like(D[:, :, R])).sum(1) / L[:, 0].clamp(min=1)
    scored = (N[:, 0] >= 1) & (M[:, 0] >= 1) & ((N - M)[:, 0].abs() <= R)
    zero = torch.zeros_like(out)
    return torch.where(scored, out / (N + M)[:, 0].clamp(min=1), zero), torch.where(scored, sync, zero)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1001)
    ap.add_argument("--order", type=int, default=13)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--torch_steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref_rows", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcd_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    import speech_anonymization_amd  # noqa: F401  (registers the package name)
    from speech_anonymization_amd import metrics, ops, reports
    from tests import mcd_ref as R
    B, T = a.B, a.T
    fields = [R.mel_field(T, 4000 + 2 * b) for b in range(B)]
    ref = torch.from_numpy(np.stack(fields).astype(np.float32)).to(dev)
    deg = torch.from_numpy(np.stack([R.warped(f, T, 4001 + 2 * b) for b, f in enumerate(fields)])
                           .astype(np.float32)).to(dev)
    n = torch.full((B,), T, dtype=torch.int32, device=dev)
    res = {"B": B, "T": T, "n_mels": int(ref.shape[2]), "order": a.order, "steps": a.steps,
           "torch_steps": a.torch_steps}
    for band in (16, 63):
        got = ops.mcd(ref, deg, n, n, order=a.order, band=band)
        ms = time_calls(lambda: ops.mcd(ref, deg, n, n, order=a.order, band=band), a.warmup, a.steps)
        tor = torch_mcd(ref, deg, n, n, a.order, band)
        ms_torch = time_calls(lambda: torch_mcd(ref, deg, n, n, a.order, band), 1, a.torch_steps)
        diff = max(float((got[i].double() - tor[i]).abs().max()) for i in (0, 1))
        res.update({f"band{band}_ms": round(ms, 4), f"rows_per_s_{band}": round(B / ms * 1e3),
                    f"torch{band}_ms": round(ms_torch, 2), f"torch_over_kernel_{band}": round(ms_torch / ms, 1),
                    f"max_abs_diff_{band}": float(f"{diff:.3e}"),
                    f"mcd_mean_{band}": round(float(got[0].mean()), 6),
                    f"mcd_sync_mean_{band}": round(float(got[1].mean()), 6)})
        if band == 16:
            rows = min(a.ref_rows, B)
            t0 = time.perf_counter()
            want = R.score(ref[:rows].cpu().numpy(), deg[:rows].cpu().numpy(), [T] * rows, [T] * rows, a.order, band)
            res["ref_rows_per_s"] = round(rows / (time.perf_counter() - t0), 2)
            vs_ref = max(float(np.abs(got[i][:rows].double().cpu().numpy() - getattr(want, k)).max())
                         for i, k in enumerate(R.OUTPUTS))
            res["max_abs_diff_vs_ref"] = float(f"{vs_ref:.3e}")

    from tests import contour_ref as Cr
    g = torch.Generator().manual_seed(2023)
    N = (T - 1) * HOP
    wav = torch.stack([Cr.glide_row(lambda t: 110.0 + 80.0 * t / (N / SR), N, g) for _ in range(2)]).float()
    wav = wav.repeat(B // 2 + 1, 1)[:B].to(dev).contiguous()
    out_wav = torch.roll(wav, 3 * HOP, 1).contiguous()
    win = reports.Batch(wav, torch.ones(B), out_wav, [N] * B).window
    mels = lambda: metrics.log_mels(win.ref, win.deg)
    m_ref, m_deg = mels()
    ids, rep = [str(i) for i in range(B)], reports.Report("report_mcd", {})

    def score():
        fr = metrics.frame_counts(win.nv, win.width)
        rep.collect(ids, ops.mcd(m_ref, m_deg, fr, fr, order=rep.opts["mcd_order"], band=rep.opts["mcd_band"]))

    for name, fn in (("stage_fbank_ms", mels), ("stage_score_ms", score), ("stage_to_host_ms", rep.fetch)):
        res[name] = round(time_calls(fn, a.warmup, a.steps), 4)
    write_line(res, a.out)


if __name__ == "__main__":
    main()
