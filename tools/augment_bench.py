#!/usr/bin/env python3
"""Times the fused waveform augmentation (csrc/sa_augment.hip) at B = 32, L = 161 120 with noise rows, a
torch-operator restatement of the same plan on the GPU in the same run, and the gender recipe's train step with
augmentation off and on.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line:
  fused_ms               sa_wav_abs_sums + sa_noise_scales + sa_wav_augment on an uploaded plan (noise given)
  fused_gbps             4 (2 B L + R L') bytes over that time
  torch_ms, speedup      speechbrain's structure in torch operators: per phase conv1d (stride S_in) +
                         conv_transpose1d (stride S_out) + add, a 101-tap conv1d, indexed zeroing, cat, the
                         element-wise noise passes; its result is compared with the fused one before it is timed
  train_augment_ms       one TrainAugment call: plan draw on the host, upload, torch.randn, the three launches
  step_*_ms              GenderBrain.fit_batch at B = 32 without augmentation, the same at B = 64 (what doubling
                         the batch alone costs), and at B = 32 with augmentation on"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from tools.bench_common import bench_brain, time_calls  # noqa: E402


def torch_restatement(wav, lens, plan, noise, snr, first, w, h):
    B, L = wav.shape
    den = lens * L
    ac, an = wav.abs().sum(1) / den, noise.abs().sum(1) / den
    f = 1.0 / (10.0 ** (snr / 20.0) + 1.0)
    g = f * ac / (an + 1e-14)
    x = torch.cat([wav, (1.0 - f)[:, None] * wav + g[:, None] * noise])
    if plan.S_out == 1 and plan.W == 1:
        r = x
    else:
        r = torch.zeros(plan.R, plan.Lp, device=wav.device, dtype=wav.dtype)
        one = torch.ones(1, 1, 1, device=wav.device, dtype=wav.dtype)
        for i in range(plan.S_out):
            nq = (plan.Lp - i + plan.S_out - 1) // plan.S_out
            if nq <= 0:
                continue
            pl = max(0, -first[i])
            start = first[i] + pl
            pr = max(0, (nq - 1) * plan.S_in + plan.W + start - (L + pl))
            seg = F.pad(x[:, None, :], (pl, pr))[..., start:]
            y = F.conv1d(seg, w[i].view(1, 1, -1), stride=plan.S_in)[..., :nq]
            yt = F.conv_transpose1d(y, one, stride=plan.S_out)[:, 0, :]
            r[:, i:i + yt.shape[-1]] += yt
    y = F.conv1d(r[:, None, :], h.view(1, 1, -1), padding=50)[:, 0, :]
    for row, ivs in enumerate(plan.chunks):
        for s, e in ivs:
            y[row, s:e] = 0.0
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=161120)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--speed", type=int, default=95, help="the plan's speed (95 / 105 resample, 100 copies)")
    ap.add_argument("--no-step", action="store_true", help="skip the recipe-step timings")
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    from speech_anonymization_amd import augment, ops
    from speech_anonymization_amd.brain import Batch
    B, L = a.B, a.L
    g = torch.Generator().manual_seed(0)
    host_lens = 0.6 + 0.4 * torch.rand(B, generator=g)
    host_lens[0] = 1.0
    wav_cpu = 0.1 * torch.randn(B, L, generator=g)
    wav, lens = wav_cpu.to(dev), host_lens.to(dev)
    noise = torch.randn(B, L, device=dev)
    # a drawn plan with the speed fixed and the largest notch and chunk counts
    drawn = augment.draw_plan(g, host_lens, L, {"speeds": [a.speed], "drop_freq_count_low": 3,
                                                "drop_chunk_count_low": 5})
    plan = drawn
    words = plan.words().to(dev)
    snr = words[plan.snr_offset:].view(torch.float32)
    fmin, fmax = int(plan.first.min()), int(plan.first.max())

    def fused():
        scales = ops.noise_scales(ops.wav_abs_sums(wav, noise), lens, snr, L)
        return ops.wav_augment(wav, noise, scales, words, plan.R, plan.Lp, plan.S_in, plan.S_out, plan.W, fmin, fmax)

    first, w, h = plan.first.tolist(), plan.w.to(dev), plan.h.to(dev)
    restated = lambda: torch_restatement(wav, lens, plan, noise, snr, first, w, h)
    got, want = fused(), restated()
    diff = float((got - want).abs().max())
    scale = float(want.abs().max())
    assert diff <= 1e-4 * scale, (diff, scale)
    fused_ms = time_calls(fused, a.warmup, a.steps)
    torch_ms = time_calls(restated, a.warmup, a.steps)
    nbytes = 4 * (B * L * 2 + plan.R * plan.Lp)
    out = {"B": B, "L": L, "R": plan.R, "Lp": plan.Lp, "speed": plan.speed, "notches": len(plan.centres),
           "steps": a.steps, "fused_ms": round(fused_ms, 4), "bytes": nbytes,
           "fused_gbps": round(nbytes / fused_ms / 1e6, 1), "torch_ms": round(torch_ms, 4),
           "speedup_vs_torch": round(torch_ms / fused_ms, 2), "max_abs_diff_vs_torch": diff}
    aug = augment.TrainAugment(seed=1)
    out["train_augment_ms"] = round(time_calls(lambda: aug(wav, lens, host_lens=host_lens), a.warmup, a.steps), 4)

    if not a.no_step:
        with tempfile.TemporaryDirectory() as tmp:
            label = torch.arange(B) % 2
            batch = Batch(wav_cpu, host_lens, label)
            twice = Batch(torch.cat([wav_cpu, wav_cpu]), host_lens.repeat(2), label.repeat(2))
            for name, on, bt in (("step_off_B32_ms", False, batch), ("step_off_B64_ms", False, twice),
                                 ("step_on_B32_ms", True, batch)):
                b = bench_brain("gender_classifier_train", bt.sig[0].shape[0], tmp, {"augment": on})
                out[name.replace("32", str(B)).replace("64", str(2 * B))] = round(
                    time_calls(lambda: b.fit_batch(bt), a.warmup, a.steps), 4)
                del b
                torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
