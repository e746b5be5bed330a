#!/usr/bin/env python3
"""Times the source-filter resynthesis (csrc/sa_srcfilt.hip, sourcefilter.py) at B = 32 utterances
of 10 s: pulse trains through three resonances (tests/mcadams_ref.voiced_row, one second of each repeated).

Device events around each call after a warm-up; the median of --steps calls.  Prints one JSON line (and writes it
to --out):
  pulses_ms, excite_ms, synth_ms     the three entry points through their bindings (synth with level on), on the
                                     batch's YIN track with rho_q to 170 Hz
  synth_no_level_ms                  the synthesis with level off (no sums)
  srcfilt_ms, frames_per_s           ops.srcfilt, the three in a row; frames = B T'
  mcadams_ms, srcfilt_over_mcadams, synth_over_mcadams
                                     ops.mcadams at alpha = 0.8 on the same batch in the same session: the kernel the
                                     synthesis shares its framing with
  stage_f0_ms, stage_ratio_ms, stage_srcfilt_ms, sourcefilter_ms
                                     SourceFilter's stages (pitchnorm.f0_track, ops.pitch_ratio with the rho_q table,
                                     ops.srcfilt with its status counts) and its whole call
  step_plain_ms, step_resynth_ms     GenderBrain.fit_batch without and with the SourceFilter among its
                                     waveform_transforms (the plain and the resynth recipe), on the same synthetic batch"""
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
    ap.add_argument("--target_hz", type=float, default=170.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the recipe-step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srcfilt_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    import speech_anonymization_amd  # noqa: F401  (registers the package name)
    from speech_anonymization_amd import data, ops, pitchnorm, sourcefilter
    B, N = a.B, int(a.seconds * SR)
    wav, lens = voiced_rows(B, N).to(dev), torch.ones(B, device=dev)
    nv = torch.full((B,), N, dtype=torch.int32, device=dev)
    alpha = torch.full((B,), 0.8, dtype=torch.float32, device=dev)
    seed = torch.arange(B, dtype=torch.int32, device=dev)
    T = ops.mcadams_frames(N)

    f0 = pitchnorm.f0_track(wav, 0.15, "yin", lens)

    def rho_of():
        ratio = ops.pitch_ratio(f0, lens, N, a.target_hz)[0]
        return torch.round(ratio.double() * ops.SRCFILT_RHO_ONE).to(torch.int32)[:, None].expand(B, f0.shape[1]) \
            .contiguous()

    rho_q = rho_of()
    pos, per, count = ops.srcfilt_pulses(f0, rho_q, nv, N=N)
    exc = ops.srcfilt_excite(f0, pos, per, count, seed, nv, 0.3, N=N)
    out, gain, status = ops.srcfilt_synth(wav, exc, nv, True, return_status=True)
    counts = [int((status == k).sum()) for k in range(4)]
    res = {"B": B, "N": N, "T": T, "track_frames": int(f0.shape[1]), "target_hz": a.target_hz, "steps": a.steps,
           "frames": B * T, "frames_ok": counts[0], "frames_silent": counts[1], "frames_fallback": counts[2],
           "frames_unexcited": counts[3], "pulses_min": int(count.min()), "pulses_max": int(count.max()),
           "gain_min": round(float(gain.min()), 4), "gain_max": round(float(gain.max()), 4)}
    for name, call in (("pulses_ms", lambda: ops.srcfilt_pulses(f0, rho_q, nv, N=N)),
                       ("excite_ms", lambda: ops.srcfilt_excite(f0, pos, per, count, seed, nv, 0.3, N=N)),
                       ("synth_ms", lambda: ops.srcfilt_synth(wav, exc, nv, True)),
                       ("synth_no_level_ms", lambda: ops.srcfilt_synth(wav, exc, nv, False)),
                       ("srcfilt_ms", lambda: ops.srcfilt(wav, f0, rho_q, seed, nv, 0.3, True)),
                       ("mcadams_ms", lambda: ops.mcadams(wav, alpha, nv, True))):
        res[name] = round(time_calls(call, a.warmup, a.steps), 4)
    res["frames_per_s"] = round(B * T / res["srcfilt_ms"] * 1e3)
    res["srcfilt_over_mcadams"] = round(res["srcfilt_ms"] / res["mcadams_ms"], 3)
    res["synth_over_mcadams"] = round(res["synth_ms"] / res["mcadams_ms"], 3)

    sf = sourcefilter.SourceFilter(a.target_hz)
    for name, call in (("stage_f0_ms", lambda: pitchnorm.f0_track(wav, 0.15, "yin", lens)),
                       ("stage_ratio_ms", rho_of),
                       ("stage_srcfilt_ms", lambda: ops.srcfilt(wav, f0, rho_q, seed, nv, 0.3, True,
                                                                return_status=True)),
                       ("sourcefilter_ms", lambda: sf(wav, lens))):
        res[name] = round(time_calls(call, a.warmup, a.steps), 4)

    if not a.no_step:
        batch = next(iter(data.synthetic_gender_dataset(B, B, n_samples=N)))
        with tempfile.TemporaryDirectory() as tmp:
            for name, cfg, over in (("step_plain_ms", "gender_classifier_train", None),
                                    ("step_resynth_ms", "gender_classifier_train_resynth",
                                     {"resynth_pitch_hz": a.target_hz})):
                b = bench_brain(cfg, B, tmp, over)
                res[name] = round(time_calls(lambda: b.fit_batch(batch), a.warmup, a.steps), 4)
                del b
                torch.cuda.empty_cache()
    write_line(res, a.out)


if __name__ == "__main__":
    main()
