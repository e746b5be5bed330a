#!/usr/bin/env python3
"""Times the modulation-spectrum smoothing (csrc/sa_modspec.hip, modspec.py) at B = 32 utterances
of 10 s (1001 frames): the STFT of amplitude-modulated harmonic rows.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  smooth_J20_ms, smooth_J64_ms       ops.modspec_smooth (both launches, outputs and workspace allocated) with the 10 Hz
                                     taps (J = 20) and with 64 taps a side
  gbytes_per_s_J20, gbytes_per_s_J64 24 bytes an element (R read twice, C written once) over that time
  torch_fp64_J20_ms, torch_fp64_J64_ms, torch_fp32_J20_ms, torch_fp32_J64_ms
                                     the same arithmetic in torch operators (abs, amax, log, clamp, a grouped conv1d
                                     along time over replicate padding, exp, multiply), in fp64 as the kernel computes
                                     and in fp32
  stage_stft_ms, stage_smooth_ms, stage_istft_ms, smoother_ms
                                     ModulationSmoother's stages (pitchnorm.padded_stft, ops.modspec_smooth,
                                     ops.gl_istft) and its whole call
  step_plain_ms, step_modspec_ms     GenderBrain.fit_batch without and with the smoother among its
                                     waveform_transforms (the plain and the modspec recipe), on the same synthetic batch"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tools.bench_common import bench_brain, time_calls, write_line  # noqa: E402

SR = 16000


def modulated_rows(B, N):
    """B rows: a harmonic series at 100 + 4 b Hz under a (3 + b / 4) Hz amplitude modulation, fp32 [B, N]"""
    t = np.arange(N, dtype=np.float64) / SR
    rows = [0.1 * (1.0 + 0.5 * np.cos(2 * np.pi * (3.0 + b / 4.0) * t)) *
            sum(np.sin(2 * np.pi * (100.0 + 4.0 * b) * k * t) / k for k in range(1, 20)) for b in range(B)]
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def torch_chain(R, taps, floor_rel, gmax, dtype):
    """sa_modspec_smooth at depth 1 and full rows in torch operators -> C"""
    J = taps.numel() - 1
    full = torch.cat([taps.flip(0)[:-1], taps]).to(dtype)
    w = full[None, None, :].expand(201, 1, 2 * J + 1).contiguous()
    m = R.abs().to(dtype)
    fl = (floor_rel * m.amax((1, 2), keepdim=True)).clamp_min(1e-10)
    L = torch.log(torch.maximum(m, fl)).transpose(1, 2)
    s = torch.nn.functional.conv1d(torch.nn.functional.pad(L, (J, J), mode="replicate"), w, groups=201)
    g = (s - L).clamp(-gmax, gmax).transpose(1, 2)
    return R * torch.exp(g).to(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--cutoff_hz", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the recipe-step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modspec_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    import speech_anonymization_amd  # noqa: F401  (registers the package name)
    from speech_anonymization_amd import data, modspec, ops, pitchnorm, vocoder
    B, N = a.B, int(a.seconds * SR)
    wav, lens = modulated_rows(B, N).to(dev), torch.ones(B, device=dev)
    _, R = pitchnorm.padded_stft(wav)
    T = R.shape[1]
    depth = torch.ones(B, dtype=torch.float32, device=dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    t20, J20 = ops.modspec_taps(a.cutoff_hz, dev)
    j = torch.arange(65, dtype=torch.float64)
    t64 = 0.5 + 0.5 * torch.cos(torch.pi * j / 65)
    t64 = (t64 / (t64[0] + 2 * t64[1:].sum())).to(dev)
    gmax = 40.0 * ops.LN10_OVER_20
    res = {"B": B, "N": N, "T": T, "cutoff_hz": a.cutoff_hz, "J": J20, "steps": a.steps, "elements": B * T * 201,
           "bytes_moved": 24 * B * T * 201}
    for tag, taps in ((f"J{J20}", t20), ("J64", t64)):
        C, _ = ops.modspec_smooth(R, taps, depth, frames)
        for dt, name in ((torch.float64, "fp64"), (torch.float32, "fp32")):
            ref = torch_chain(R, taps, 1e-4, gmax, dt)
            res[f"torch_{name}_{tag}_rel_dist"] = float((torch.view_as_real(C - ref).double().norm() /
                                                         torch.view_as_real(ref).double().norm()))
            res[f"torch_{name}_{tag}_ms"] = round(time_calls(lambda: torch_chain(R, taps, 1e-4, gmax, dt), a.warmup,
                                                             a.steps), 4)
        ms = time_calls(lambda: ops.modspec_smooth(R, taps, depth, frames), a.warmup, a.steps)
        res[f"smooth_{tag}_ms"] = round(ms, 4)
        res[f"gbytes_per_s_{tag}"] = round(res["bytes_moved"] / ms / 1e6, 1)
        res[f"torch_fp64_over_smooth_{tag}"] = round(res[f"torch_fp64_{tag}_ms"] / ms, 2)

    sm = modspec.ModulationSmoother(a.cutoff_hz)
    w, tw, _ = vocoder.tables(dev)
    C, _ = ops.modspec_smooth(R, t20, depth, frames)
    for name, call in (("stage_stft_ms", lambda: pitchnorm.padded_stft(wav)),
                       ("stage_smooth_ms", lambda: ops.modspec_smooth(R, t20, depth, frames)),
                       ("stage_istft_ms", lambda: ops.gl_istft(C, w, tw)),
                       ("smoother_ms", lambda: sm(wav, lens))):
        res[name] = round(time_calls(call, a.warmup, a.steps), 4)

    if not a.no_step:
        batch = next(iter(data.synthetic_gender_dataset(B, B, n_samples=N)))
        with tempfile.TemporaryDirectory() as tmp:
            for name, cfg, over in (("step_plain_ms", "gender_classifier_train", None),
                                    ("step_modspec_ms", "gender_classifier_train_modspec",
                                     {"modspec_cutoff_hz": a.cutoff_hz})):
                b = bench_brain(cfg, B, tmp, over)
                res[name] = round(time_calls(lambda: b.fit_batch(batch), a.warmup, a.steps), 4)
                del b
                torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
