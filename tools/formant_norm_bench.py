#!/usr/bin/env python3
"""Times the formant normalisation (csrc/sa_formant_norm.hip, formantnorm.py) at B = 32 utterances
of 10 s: pulse trains through three resonances (tests/mcadams_ref.voiced_row, one second of each repeated).

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  pole_warp_ms, frames_per_s    sa_pole_warp through ops.pole_warp with level on, at q = 0.85: the frame kernel, the
                                level sums, the gain and the last pass; frames = B T
  pole_warp_no_level_ms         the same with level off (no sums)
  mcadams_ms, pole_warp_over_mcadams
                                ops.mcadams at alpha = 0.8 on the same batch in the same session: the kernel this one
                                shares its structure with
  centre_ms, compare_ms         sa_formant_centre through ops.formant_centre on the batch's tracks, and
                                sa_formant_compare through ops.formant_compare on the tracks of the batch and of its
                                warped copy, in the same session: the select on three keys next to the one on six
  stage_f0_ms, stage_tracks_ms, stage_centre_ms, stage_warp_ms, normalizer_ms
                                FormantNormalizer's stages (pitchnorm.f0_track, ops.formant_tracks,
                                ops.formant_centre, ops.pole_warp with its status counts) and its whole call
  step_plain_ms, step_formant_norm_ms, step_formant_norm_psola_ms
                                the plain recipe's fit_batch, and the formant_norm recipe's without and with the PSOLA
                                stage, on the same synthetic batch"""
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


def voiced_rows(B, N):
    """B rows: one second of voiced_row at 100 + 4 b Hz, repeated to N samples, fp32 [B, N]"""
    from tests import mcadams_ref as M
    rows = [np.tile(M.voiced_row(100.0 + 4.0 * b, M.FORMANTS, SR, b), -(-N // SR))[:N] for b in range(B)]
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--q", type=float, default=0.85)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the recipe-step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "formant_norm_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    import speech_anonymization_amd  # noqa: F401  (registers the package name)
    from speech_anonymization_amd import data, formantnorm, ops, pitchnorm
    B, N = a.B, int(a.seconds * SR)
    wav, lens = voiced_rows(B, N).to(dev), torch.ones(B, device=dev)
    nv = torch.full((B,), N, dtype=torch.int32, device=dev)
    q = torch.full((B,), a.q, dtype=torch.float32, device=dev)
    alpha = torch.full((B,), 0.8, dtype=torch.float32, device=dev)
    T = ops.mcadams_frames(N)

    warped, gain, status = ops.pole_warp(wav, q, nv, True, return_status=True)
    counts = [int((status == k).sum()) for k in range(3)]
    res = {"B": B, "N": N, "T": T, "q": a.q, "steps": a.steps, "frames": B * T, "frames_ok": counts[0],
           "frames_silent": counts[1], "frames_fallback": counts[2], "gain_min": round(float(gain.min()), 4),
           "gain_max": round(float(gain.max()), 4)}
    res["pole_warp_ms"] = round(time_calls(lambda: ops.pole_warp(wav, q, nv, True), a.warmup, a.steps), 4)
    res["frames_per_s"] = round(B * T / res["pole_warp_ms"] * 1e3)
    res["pole_warp_no_level_ms"] = round(time_calls(lambda: ops.pole_warp(wav, q, nv, False), a.warmup, a.steps), 4)
    res["mcadams_ms"] = round(time_calls(lambda: ops.mcadams(wav, alpha, nv, True), a.warmup, a.steps), 4)
    res["pole_warp_over_mcadams"] = round(res["pole_warp_ms"] / res["mcadams_ms"], 3)

    f0 = pitchnorm.f0_track(wav, 0.15, "yin", lens)
    Tf = int(f0.shape[1])
    frames = torch.full((B,), Tf, dtype=torch.int32, device=dev)
    F, st = ops.formant_tracks(wav, nv)
    Fw, stw = ops.formant_tracks(warped, nv)
    f0w = pitchnorm.f0_track(warped, 0.15, "yin", lens)
    target = formantnorm.TARGET_DEFAULT
    res["centre_ms"] = round(time_calls(lambda: ops.formant_centre(F, st, f0, frames, target), a.warmup, a.steps), 4)
    res["compare_ms"] = round(time_calls(lambda: ops.formant_compare(F, Fw, st, stw, f0, f0w, frames), a.warmup,
                                         a.steps), 4)
    med, qc, count = (v.cpu() for v in ops.formant_centre(F, st, f0, frames, target))
    res["track_frames"] = Tf
    res["scored_rows"] = int((count > 0).sum())
    res["q_min"], res["q_max"] = round(float(qc.min()), 4), round(float(qc.max()), 4)

    fn = formantnorm.FormantNormalizer()
    for name, call in (("stage_f0_ms", lambda: pitchnorm.f0_track(wav, 0.15, "yin", lens)),
                       ("stage_tracks_ms", lambda: ops.formant_tracks(wav, nv)),
                       ("stage_centre_ms", lambda: ops.formant_centre(F, st, f0, frames, target)),
                       ("stage_warp_ms", lambda: ops.pole_warp(wav, qc.to(dev), nv, True, return_status=True)),
                       ("normalizer_ms", lambda: fn(wav, lens))):
        res[name] = round(time_calls(call, a.warmup, a.steps), 4)

    if not a.no_step:
        batch = next(iter(data.synthetic_gender_dataset(B, B, n_samples=N)))
        with tempfile.TemporaryDirectory() as tmp:
            fname = "gender_classifier_train_formant_norm"
            for name, cfg, over in (("step_plain_ms", "gender_classifier_train", None),
                                    ("step_formant_norm_ms", fname, {"pitch_norm": False}),
                                    ("step_formant_norm_psola_ms", fname, {"pitch_norm": True})):
                b = bench_brain(cfg, B, tmp, over)
                res[name] = round(time_calls(lambda: b.fit_batch(batch), a.warmup, a.steps), 4)
                del b
                torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
