#!/usr/bin/env python3
"""Times the phase-vocoder resynthesis (csrc/sa_phasevoc.hip, ops.pv_synth) at B = 32 utterances
of 10 s: sa_pv_synth against the same definition in torch operators on the same device in the same run, both classes
of pitchnorm.py with both ``phase`` settings, and the gender recipe's train step with both.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  pv_synth_ms, pv_synth_null_ms   the three launches of sa_pv_synth with the magnitudes given and with S = NULL;
                                  pv_synth_gbs: R read twice, S read once, C written once, over pv_synth_ms
  torch_pv_ms, speedup_vs_torch   angle and diff in fp64, a gather by i_s, cumsum, polar; its C is compared with the
                                  kernel's before anything is timed (max |C - C_torch| / max |S|)
  stretch_ms                      sa_pitch_stretch_mag alone, what the vocoder path no longer launches
  normalizer_{griffin_lim,vocoder}_ms, shifter_{griffin_lim,vocoder}_ms
                                  PitchNormalizer and FormantShifter(1.15), the whole call
  step_{griffin_lim,vocoder}_ms   the pitch_norm recipe's fit_batch on the same batch"""
import argparse
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from tools.bench_common import bench_brain, time_calls, write_line  # noqa: E402

SR, HOP, NBIN = 16000, 160, 201


def torch_pv(R, ratio, Tout, S):
    """the definition in torch operators on the device, phases in fp64"""
    B, T, K = R.shape
    r = ratio.double().clamp(0.5, 2.0)[:, None]
    tp = torch.arange(Tout, device=R.device, dtype=torch.float64)[None, :]
    live = tp < torch.ceil((T - 1) * r) + 1
    pos = (tp / r).clamp(max=T - 1)
    i = pos.floor().long().clamp(max=T - 2)
    th = torch.angle(R.to(torch.complex128)) / (2.0 * math.pi)
    inc = torch.diff(th, dim=1).gather(1, i[:, :, None].expand(-1, -1, K))
    phi = (th[:, :1] + inc.cumsum(1) - inc) % 1.0
    C = torch.polar(S.double(), 2.0 * math.pi * phi).to(torch.complex64)
    return torch.where(live[:, :, None], C, torch.zeros((), dtype=C.dtype, device=C.device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the recipe-step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phasevoc_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    from speech_anonymization_amd import data, ops, pitchnorm
    B, N = a.B, int(a.seconds * SR)
    batch = next(iter(data.synthetic_gender_dataset(B, B, n_samples=N)))
    wav_cpu, lens_cpu = batch.sig
    wav, lens = wav_cpu.to(dev), lens_cpu.to(dev)

    ratio = ops.pitch_ratio(ops.yin_f0(wav), lens, N)[0]
    R = pitchnorm.padded_stft(wav)[1]
    Tout = max(pitchnorm.stretched_frames(R.shape[1], r) for r in ratio.cpu().tolist())
    S = ops.pitch_stretch_mag(R, ratio, Tout)
    C = ops.pv_synth(R, ratio, Tout, S=S)
    assert torch.equal(C, ops.pv_synth(R, ratio, Tout))
    diff = float((C - torch_pv(R, ratio, Tout, S)).abs().max() / S.max())
    assert diff <= 1e-6, diff
    out = {"B": B, "N": N, "T": R.shape[1], "Tout": Tout, "steps": a.steps, "elements": B * Tout * NBIN,
           "ratio_min": round(float(ratio.min()), 4), "ratio_max": round(float(ratio.max()), 4),
           "max_diff_vs_torch_rel": float(f"{diff:.3e}")}
    out["pv_synth_ms"] = round(time_calls(lambda: ops.pv_synth(R, ratio, Tout, S=S), a.warmup, a.steps), 4)
    out["pv_synth_null_ms"] = round(time_calls(lambda: ops.pv_synth(R, ratio, Tout), a.warmup, a.steps), 4)
    out["pv_synth_gbs"] = round((2 * R.numel() * 8 + S.numel() * 4 + C.numel() * 8) / out["pv_synth_ms"] / 1e6, 1)
    out["torch_pv_ms"] = round(time_calls(lambda: torch_pv(R, ratio, Tout, S), a.warmup, a.steps), 4)
    out["speedup_vs_torch"] = round(out["torch_pv_ms"] / out["pv_synth_ms"], 2)
    out["stretch_ms"] = round(time_calls(lambda: ops.pitch_stretch_mag(R, ratio, Tout), a.warmup, a.steps), 4)
    del C, S
    for phase in pitchnorm.PHASES:
        norm = pitchnorm.PitchNormalizer(phase=phase)
        out[f"normalizer_{phase}_ms"] = round(time_calls(lambda: norm(wav, lens), a.warmup, a.steps), 4)
        fs = pitchnorm.FormantShifter(1.15, phase=phase)
        out[f"shifter_{phase}_ms"] = round(time_calls(lambda: fs(wav, lens), a.warmup, a.steps), 4)

    if not a.no_step:
        with tempfile.TemporaryDirectory() as tmp:
            for phase in pitchnorm.PHASES:
                b = bench_brain("gender_classifier_train_pitch_norm", B, tmp, {"phase": phase})
                out[f"step_{phase}_ms"] = round(time_calls(lambda: b.fit_batch(batch), a.warmup, a.steps), 4)
                del b
                torch.cuda.empty_cache()
    write_line(out, a.out)


if __name__ == "__main__":
    main()
