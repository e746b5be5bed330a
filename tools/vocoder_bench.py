#!/usr/bin/env python3
"""Times the Griffin-Lim inversion (csrc/sa_vocoder.hip) at B = 32, T = 1008, 32 iterations, the same loop on
torch.stft / torch.istft on the same device in the same run, and the stages of anonymize.py one by one.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  istft_ms, project_ms   one launch of sa_gl_istft / sa_gl_project
  loop_ms                GriffinLim on uploaded phases: 2 n_iter + 1 launches (and the two torch calls that make C0)
  module_ms              the same with the phases drawn on the host and uploaded
  torch_loop_ms, speedup_vs_torch
                         the loop in torch operators (istft, stft, the update element-wise); after 2 iterations its
                         signal is compared with the kernels' before anything is timed
  stage_*_ms             Fbank, normalise (pad to 36), ConvAutoencoder.reconstruct (random weights, bf16x3),
                         sa_mel_to_mag, the loop (= loop_ms), spectral_convergence
  dense_gflop            the dense form's arithmetic per direction per iteration, 2 * 400 * 402 * B * T, for scale; the
                         kernels issue a quarter (inverse) and half (forward) of its multiplications"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from tools.bench_common import time_calls  # noqa: E402


def torch_loop(S, phi, n_iter, m, window):
    """the definition in torch operators; spectra as [B, 201, T], torch's layout"""
    N = (S.shape[1] - 1) * 160
    St = S.transpose(1, 2)
    ist = lambda C: torch.istft(C, 400, 160, 400, window, center=True, length=N)
    C = torch.polar(St, phi.transpose(1, 2))
    Tprev = torch.zeros_like(C)
    for _ in range(n_iter):
        R = torch.stft(ist(C), 400, 160, 400, window, center=True, pad_mode="constant", return_complex=True)
        A = R - m * Tprev
        C, Tprev = St * A / (A.abs() + 1e-16), R
    return ist(C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1008)
    ap.add_argument("--n_iter", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocoder_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    from speech_anonymization_amd import convae, features, ops, vocoder
    from speech_anonymization_amd.data import synthetic_dataset
    B, T, N = a.B, a.T, (a.T - 1) * 160
    wavs = next(iter(synthetic_dataset(B, B, n_samples=N)))
    wav, lens = wavs.sig[0].to(dev), wavs.sig[1]
    w, tw, M = vocoder.tables(dev)
    S = vocoder.stft(wav).abs().contiguous()
    gl = vocoder.GriffinLim(n_iter=a.n_iter, seed=0)
    phi = gl.draw_phase(S.shape).to(dev)
    m = float(torch.tensor(gl.m, dtype=torch.float32))

    two = vocoder.GriffinLim(n_iter=2, seed=0)(S, phase=phi)
    want = torch_loop(S, phi, 2, m, w)
    diff = float((two - want).norm() / want.norm())
    assert diff <= 1e-4, diff

    C0 = torch.polar(S, phi)
    y0 = ops.gl_istft(C0, w, tw)
    out = {"B": B, "T": T, "n_iter": a.n_iter, "steps": a.steps, "dense_gflop": round(2 * 400 * 402 * B * T / 1e9, 2),
           "rel_diff_vs_torch_after_2_iterations": diff}
    out["istft_ms"] = round(time_calls(lambda: ops.gl_istft(C0, w, tw), a.warmup, a.steps), 4)
    out["project_ms"] = round(time_calls(lambda: ops.gl_project(y0, S, C0, m, w, tw), a.warmup, a.steps), 4)
    out["loop_ms"] = round(time_calls(lambda: gl(S, phase=phi), a.warmup, a.steps), 4)
    out["module_ms"] = round(time_calls(lambda: gl(S), a.warmup, a.steps), 4)
    out["torch_loop_ms"] = round(time_calls(lambda: torch_loop(S, phi, a.n_iter, m, w), a.warmup, a.steps), 4)
    out["speedup_vs_torch"] = round(out["torch_loop_ms"] / out["loop_ms"], 2)
    y = gl(S, phase=phi)
    out["spectral_convergence_mean"] = round(float(vocoder.spectral_convergence(y, S).mean()), 5)

    fbank = features.Fbank().to(dev)
    norm = features.InputNormalization(norm_type="global").to(dev).train()
    feats = fbank(wav)
    norm(feats, lens, epoch=0)
    norm.eval()
    torch.manual_seed(0)
    model = convae.ConvAutoencoder(precision="bf16x3").to(dev).eval()
    normed = norm(feats, lens, epoch=1, pad_multiple=36)
    recon = model.reconstruct(normed)
    mean, std = norm.glob_mean.contiguous(), norm.glob_std.contiguous()
    Sm = ops.mel_to_mag(normed, mean, std, M, T)
    out["stage_fbank_ms"] = round(time_calls(lambda: fbank(wav), a.warmup, a.steps), 4)
    out["stage_normalise_ms"] = round(time_calls(lambda: norm(feats, lens, epoch=1, pad_multiple=36), a.warmup, a.steps), 4)
    out["stage_reconstruct_ms"] = round(time_calls(lambda: model.reconstruct(normed), a.warmup, a.steps), 4)
    out["stage_mel_to_mag_ms"] = round(time_calls(lambda: ops.mel_to_mag(recon, mean, std, M, T), a.warmup, a.steps), 4)
    out["stage_loop_ms"] = out["loop_ms"]
    out["stage_spectral_convergence_ms"] = round(time_calls(lambda: vocoder.spectral_convergence(y, Sm), a.warmup,
                                                            a.steps), 4)
    assert math.isfinite(out["spectral_convergence_mean"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
