#!/usr/bin/env python3
"""Times the pitch normalisation (csrc/sa_pitch.hip, pitchnorm.py) at B = 32 utterances of 10 s:
sa_yin_f0 against a restatement in torch operators on the same device in the same run, the stages of
PitchNormalizer one by one, and the gender recipe's train step with and without it.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  yin_ms, yin_gflops     one launch of sa_yin_f0; 3 * 266 * 400 operations per frame
  torch_yin_ms, speedup_vs_torch
                         d by unfold + broadcast (rows in chunks of --chunk: the difference tensor is B T 266 400
                         floats), cumsum, the pick and the parabola in torch operators; its f0 is compared with the
                         kernel's before anything is timed (frames that agree within 0.01 Hz)
  stage_*_ms             sa_yin_f0, sa_pitch_ratio, vocoder.stft, sa_pitch_stretch_mag, GriffinLim, sa_pitch_resample
                         at the ratios of the batch, and normalizer_ms, the whole call with its one host copy
  step_plain_ms, step_pitch_norm_ms
                         the plain and the pitch_norm recipe's fit_batch on the same batch"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from tools.bench_common import bench_brain, time_calls, write_line  # noqa: E402

SR, HOP, W, TAU_MIN, TAU_MAX = 16000, 160, 400, 40, 266


def torch_yin(wav, threshold, chunk):
    """the definition in torch operators, fp32 on the device"""
    B, N = wav.shape
    T, L = N // HOP + 1, W + TAU_MAX
    x = torch.nn.functional.pad(wav, (L // 2, max(0, HOP * (T - 1) - L // 2 + L - N))).unfold(1, L, HOP)[:, :T]
    tau = torch.arange(TAU_MAX + 1, device=wav.device, dtype=torch.float32)
    out = []
    for b0 in range(0, B, chunk):
        xb = x[b0:b0 + chunk]
        lag = xb.unfold(2, W, 1)                                  # [b, T, 267, 400]: lag[..., tau, j] = x[j + tau]
        d = ((xb[..., None, :W] - lag) ** 2).sum(-1)
        c = d.cumsum(-1)
        dp = torch.where(c > 0, d * tau / c.clamp(min=1e-30), torch.ones_like(c))
        dp[..., 0] = 1.0
        mid = dp[..., TAU_MIN:TAU_MAX]
        ok = (mid < threshold) & (mid <= dp[..., TAU_MIN - 1:TAU_MAX - 1]) & (mid < dp[..., TAU_MIN + 1:TAU_MAX + 1])
        p = ok.to(torch.int64).argmax(-1) + TAU_MIN
        a, cc, e = (dp.gather(-1, (p + k)[..., None])[..., 0] for k in (-1, 0, 1))
        den = a - 2 * cc + e
        off = torch.where(den > 0, 0.5 * (a - e) / den.clamp(min=1e-30), torch.zeros_like(den))
        out.append(torch.where(ok.any(-1), SR / (p + off), torch.zeros_like(off)))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the recipe-step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_norm_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    from speech_anonymization_amd import data, ops, pitchnorm, vocoder
    B, N = a.B, int(a.seconds * SR)
    batch = next(iter(data.synthetic_gender_dataset(B, B, n_samples=N)))
    wav_cpu, lens_cpu = batch.sig
    wav, lens = wav_cpu.to(dev), lens_cpu.to(dev)
    T = N // HOP + 1

    got, want = ops.yin_f0(wav), torch_yin(wav, 0.15, a.chunk)
    agree = float(((got - want).abs() <= 0.01).double().mean())
    assert agree >= 0.99, agree
    yin_ms = time_calls(lambda: ops.yin_f0(wav), a.warmup, a.steps)
    torch_ms = time_calls(lambda: torch_yin(wav, 0.15, a.chunk), 1, max(3, a.steps // 5))
    out = {"B": B, "N": N, "T": T, "steps": a.steps, "frames_agreeing_with_torch": round(agree, 5),
           "yin_ms": round(yin_ms, 4), "yin_gflops": round(3 * TAU_MAX * W * B * T / yin_ms / 1e6, 1),
           "torch_yin_ms": round(torch_ms, 4), "speedup_vs_torch": round(torch_ms / yin_ms, 2)}

    norm = pitchnorm.PitchNormalizer()
    f0 = ops.yin_f0(wav)
    ratio, mean, voiced = ops.pitch_ratio(f0, lens, N)
    wp, R = pitchnorm.padded_stft(wav)
    Tout = max(pitchnorm.stretched_frames(R.shape[1], r) for r in ratio.cpu().tolist())
    S = ops.pitch_stretch_mag(R, ratio, Tout)
    phi = norm.gl.draw_phase(S.shape).to(dev)
    y = norm.gl(S, phase=phi)
    nv = pitchnorm.n_valid(lens, N, dev).to(torch.int32)
    out.update(ratio_min=round(float(ratio.min()), 4), ratio_max=round(float(ratio.max()), 4), Tout=Tout)
    for name, fn in (("stage_yin_ms", lambda: ops.yin_f0(wav)),
                     ("stage_ratio_ms", lambda: ops.pitch_ratio(f0, lens, N)),
                     ("stage_stft_ms", lambda: vocoder.stft(wp)),
                     ("stage_stretch_ms", lambda: ops.pitch_stretch_mag(R, ratio, Tout)),
                     ("stage_griffin_lim_ms", lambda: norm.gl(S, phase=phi)),
                     ("stage_resample_ms", lambda: ops.pitch_resample(y, ratio, nv, N)),
                     ("normalizer_ms", lambda: norm(wav, lens))):
        out[name] = round(time_calls(fn, a.warmup, a.steps), 4)

    if not a.no_step:
        with tempfile.TemporaryDirectory() as tmp:
            for name, fn in (("step_plain_ms", "gender_classifier_train"),
                             ("step_pitch_norm_ms", "gender_classifier_train_pitch_norm")):
                b = bench_brain(fn, B, tmp)
                out[name] = round(time_calls(lambda: b.fit_batch(batch), a.warmup, a.steps), 4)
                del b
                torch.cuda.empty_cache()
    write_line(out, a.out)


if __name__ == "__main__":
    main()
