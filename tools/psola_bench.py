#!/usr/bin/env python3
"""Times the TD-PSOLA pitch modification (csrc/sa_psola.hip) at B = 32 utterances of 10 s: the three
kernels, PitchNormalizer(psola=True) against the two STFT-domain paths in the same process, and the gender recipe's
train step with each.  The utterances are data.synthetic_gender_dataset's.

Device events around each call after a warm-up; the median of --steps calls.  Every figure is a call THROUGH THE BINDING:
the launch and the binding's allocations are inside it.  Nothing is asserted on the times.  Prints one JSON line (and
writes it to --out):
  marks_ms, plan_ms, ola_ms            ops.psola_marks, ops.psola_plan, ops.psola_ola at the normaliser's own ratios;
                                       marks, grains: the largest counts of a row
  psola_ms                             ops.psola, the three together;  yin_ms: the tracker in front of them
  normalizer_psola_ms, normalizer_psola_contour_ms, normalizer_vocoder_ms, normalizer_griffin_lim_ms   the whole call
  step_psola_ms, step_vocoder_ms, step_griffin_lim_ms   the pitch_norm recipe's fit_batch on the same batch"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from tools.bench_common import bench_brain, write_line  # noqa: E402
from tools.contour_bench import time_calls  # noqa: E402

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the recipe-step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psola_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    from speech_anonymization_amd import data, ops, pitchnorm
    B, N = a.B, int(a.seconds * SR)
    batch = next(iter(data.synthetic_gender_dataset(B, B, n_samples=N)))
    wav, lens = batch.sig[0].to(dev).contiguous(), batch.sig[1].to(dev).float().contiguous()

    f0 = ops.yin_f0(wav)
    T = f0.shape[1]
    ratio = ops.pitch_ratio(f0, lens, N)[0]
    rho_q = torch.round(ratio.double() * 65536.0).to(torch.int32)[:, None].expand(B, T).contiguous()
    nv = pitchnorm.n_valid(lens, N, dev).to(torch.int32)
    marks, count = ops.psola_marks(wav, f0, nv)
    pos, src, jc = ops.psola_plan(marks, count, f0, rho_q, nv, N=N)
    out = {"B": B, "N": N, "T": T, "steps": a.steps, "marks": int(count.max()), "grains": int(jc.max()),
           "ratio_min": round(float(ratio.min()), 4), "ratio_max": round(float(ratio.max()), 4)}
    tm = lambda fn: round(time_calls(fn, a.warmup, a.steps), 4)
    out["yin_ms"] = tm(lambda: ops.yin_f0(wav))
    out["marks_ms"] = tm(lambda: ops.psola_marks(wav, f0, nv))
    out["plan_ms"] = tm(lambda: ops.psola_plan(marks, count, f0, rho_q, nv, N=N))
    out["ola_ms"] = tm(lambda: ops.psola_ola(wav, marks, count, pos, src, jc, nv))
    out["psola_ms"] = tm(lambda: ops.psola(wav, f0, rho_q, nv))
    for name, kw in (("psola", {"psola": True}), ("psola_contour", {"psola": True, "contour_scale": 1.0}),
                     ("vocoder", {"phase": "vocoder"}), ("griffin_lim", {})):
        norm = pitchnorm.PitchNormalizer(**kw)
        out[f"normalizer_{name}_ms"] = tm(lambda: norm(wav, lens))

    if not a.no_step:
        with tempfile.TemporaryDirectory() as tmp:
            for name, over in (("psola", {"psola": True}), ("vocoder", {"phase": "vocoder"}), ("griffin_lim", {})):
                b = bench_brain("gender_classifier_train_pitch_norm", B, tmp, over)
                out[f"step_{name}_ms"] = tm(lambda: b.fit_batch(batch))
                del b
                torch.cuda.empty_cache()
    write_line(out, a.out)


if __name__ == "__main__":
    main()
