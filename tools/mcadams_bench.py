#!/usr/bin/env python3
"""Times the McAdams transform (csrc/sa_mcadams.hip, mcadams.py) at B = 32 utterances of 10 s.

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  mcadams_ms, frames_per_s      sa_mcadams through ops.mcadams with level on: the frame kernel, the level sums, the
                                gain and the last pass; frames = B T
  mcadams_no_level_ms           the same with level off (no sums)
  ref_frames_per_s              the fp64 restatement (tests/mcadams_ref.py, numpy) on the host, one row of 0.2 s
  stage_transform_ms, stage_f0_report_ms, stage_to_host_ms
                                anonymize.py's stages in this mode: McAdams.__call__ (the launch and the status
                                counts), the --report_f0 tracker, the copy of the batch to the host
  step_plain_ms, step_mcadams_ms
                                GenderBrain.fit_batch without and with the transform among its waveform_transforms
                                (the plain and the mcadams recipe), on the same batch"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from tools.bench_common import bench_brain, time_calls, write_line  # noqa: E402

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--alpha", type=float, default=0.8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the recipe-step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcadams_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    from speech_anonymization_amd import data, mcadams, ops, pitchnorm
    from tests import mcadams_ref as M
    B, N = a.B, int(a.seconds * SR)
    batch = next(iter(data.synthetic_gender_dataset(B, B, n_samples=N)))
    wav_cpu, lens_cpu = batch.sig
    wav, lens = wav_cpu.to(dev), lens_cpu.to(dev)
    alpha = torch.full((B,), a.alpha, device=dev)
    nv = pitchnorm.n_valid(lens, N, dev).to(torch.int32)
    T = ops.mcadams_frames(N)

    out_gpu, gain, status = ops.mcadams(wav, alpha, nv, True, return_status=True)
    counts = [int((status == k).sum()) for k in range(3)]
    ms = time_calls(lambda: ops.mcadams(wav, alpha, nv, True), a.warmup, a.steps)
    ms_plain = time_calls(lambda: ops.mcadams(wav, alpha, nv, False), a.warmup, a.steps)
    out = {"B": B, "N": N, "T": T, "alpha": a.alpha, "steps": a.steps, "frames": B * T, "frames_ok": counts[0],
           "frames_silent": counts[1], "frames_fallback": counts[2], "gain_min": round(float(gain.min()), 4),
           "gain_max": round(float(gain.max()), 4), "mcadams_ms": round(ms, 4),
           "frames_per_s": round(B * T / ms * 1e3), "mcadams_no_level_ms": round(ms_plain, 4)}

    n_ref = 3200
    t0 = time.perf_counter()
    ref = M.mcadams(wav_cpu[:1, :n_ref].numpy(), np.array([a.alpha], np.float32), np.array([n_ref], np.int32), True)
    dt = time.perf_counter() - t0
    out["ref_frames_per_s"] = round(ref.status.size / dt, 1)
    out["max_abs_diff_vs_ref_first_row"] = float(f"{np.abs(ops.mcadams(wav[:1, :n_ref].contiguous(), alpha[:1], torch.tensor([n_ref], dtype=torch.int32, device=dev), True)[0].cpu().double().numpy() - ref.out).max():.3e}")

    mc = mcadams.McAdams(a.alpha)
    for name, fn in (("stage_transform_ms", lambda: mc(wav, lens)),
                     ("stage_f0_report_ms", lambda: ops.pitch_ratio(pitchnorm.f0_track(out_gpu), lens, N)),
                     ("stage_to_host_ms", lambda: out_gpu.cpu())):
        out[name] = round(time_calls(fn, a.warmup, a.steps), 4)

    if not a.no_step:
        with tempfile.TemporaryDirectory() as tmp:
            for name, fn in (("step_plain_ms", "gender_classifier_train"),
                             ("step_mcadams_ms", "gender_classifier_train_mcadams")):
                b = bench_brain(fn, B, tmp)
                out[name] = round(time_calls(lambda: b.fit_batch(batch), a.warmup, a.steps), 4)
                del b
                torch.cuda.empty_cache()
    write_line(out, a.out)


if __name__ == "__main__":
    main()
