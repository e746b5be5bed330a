#!/usr/bin/env python3
"""Times the spectral-envelope warp (csrc/sa_envelope.hip, pitchnorm.py) at B = 32 utterances of
10 s: one launch of sa_env_warp on the stretched magnitudes of the batch against the same definition in torch
operators on the same device in the same run, PitchNormalizer with and without the warp, and FormantShifter.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  env_warp_ms, env_warp_gbs   one launch at q_b = r_b (preserve_formants); bytes = one read and one write of S
  torch_env_warp_ms, speedup_vs_torch
                              log, two matrix products with cosine matrices made once outside the timed region, exp;
                              its output is compared with the kernel's before anything is timed
  normalizer_plain_ms, normalizer_preserve_ms
                              PitchNormalizer(170) and PitchNormalizer(170, preserve_formants=True), the whole call
  formant_shifter_ms          FormantShifter(1.2), the whole call"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from tools.bench_common import time_calls, write_line  # noqa: E402

SR, HOP, N_FFT, K = 16000, 160, 400, 201


def torch_tables(q, n_c, dev):
    """(analysis matrix [201, n_c + 1], synthesis at w_k [n_c + 1, 201], synthesis at theta_k [B, n_c + 1, 201]) fp32"""
    n = torch.arange(n_c + 1, dtype=torch.float64)
    k = torch.arange(K, dtype=torch.float64)
    cos = torch.cos(2 * math.pi * ((n[:, None] * k[None, :]) % N_FFT) / N_FFT)
    wk = torch.full((K,), 2.0, dtype=torch.float64)
    wk[0] = wk[-1] = 1.0
    ana = (cos * wk[None, :] / N_FFT).T
    two = torch.full((n_c + 1,), 2.0, dtype=torch.float64)
    two[0] = 1.0
    theta = (q.double().cpu()[:, None] * k[None, :] / 200.0).clamp(max=1.0) * math.pi
    syn_t = torch.cos(n[None, :, None] * theta[:, None, :]) * two[None, :, None]
    return ana.float().to(dev), (cos * two[:, None]).float().to(dev), syn_t.float().to(dev)


def torch_env_warp(S, tables, floor_rel, limit):
    ana, syn_w, syn_t = tables
    L = torch.log(torch.maximum(torch.maximum(S, floor_rel * S.amax(-1, keepdim=True)), S.new_tensor(1e-10)))
    c = L @ ana
    g = (torch.bmm(c, syn_t) - c @ syn_w).clamp(-limit, limit)
    return S * torch.exp(g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "formant_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    from speech_anonymization_amd import data, ops, pitchnorm
    B, N = a.B, int(a.seconds * SR)
    wav_cpu, lens_cpu = next(iter(data.synthetic_gender_dataset(B, B, n_samples=N))).sig
    wav, lens = wav_cpu.to(dev), lens_cpu.to(dev)

    ratio = ops.pitch_ratio(ops.yin_f0(wav), lens, N)[0]
    R = pitchnorm.padded_stft(wav)[1]
    Tout = max(pitchnorm.stretched_frames(R.shape[1], r) for r in ratio.cpu().tolist())
    S = ops.pitch_stretch_mag(R, ratio, Tout)
    n_c, floor_rel, limit = 30, 1e-4, 40.0 * ops.LN10_OVER_20
    tables = torch_tables(ratio, n_c, dev)
    got, want = ops.env_warp(S, ratio, n_c), torch_env_warp(S, tables, floor_rel, limit)
    rel = float(((got - want).abs() / want.abs().clamp(min=1e-30)).max())
    assert rel <= 5e-2, rel
    env_ms = time_calls(lambda: ops.env_warp(S, ratio, n_c), a.warmup, a.steps)
    torch_ms = time_calls(lambda: torch_env_warp(S, tables, floor_rel, limit), a.warmup, a.steps)
    out = {"B": B, "N": N, "Tout": Tout, "n_c": n_c, "steps": a.steps, "ratio_min": round(float(ratio.min()), 4),
           "ratio_max": round(float(ratio.max()), 4), "max_rel_diff_vs_torch": float(f"{rel:.3e}"),
           "env_warp_ms": round(env_ms, 4), "env_warp_gbs": round(2 * S.numel() * 4 / env_ms / 1e6, 1),
           "torch_env_warp_ms": round(torch_ms, 4), "speedup_vs_torch": round(torch_ms / env_ms, 2)}
    plain, keep = pitchnorm.PitchNormalizer(170.0), pitchnorm.PitchNormalizer(170.0, preserve_formants=True)
    shifter = pitchnorm.FormantShifter(1.2)
    for name, fn in (("normalizer_plain_ms", lambda: plain(wav, lens)),
                     ("normalizer_preserve_ms", lambda: keep(wav, lens)),
                     ("formant_shifter_ms", lambda: shifter(wav, lens))):
        out[name] = round(time_calls(fn, a.warmup, a.steps), 4)
    write_line(out, a.out)


if __name__ == "__main__":
    main()
