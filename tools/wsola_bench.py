#!/usr/bin/env python3
"""Times the WSOLA time-scale modification (csrc/sa_wsola.hip) at B = 32 utterances of 10 s, tempo
0.5, 0.8 and 1.25: the three kernels, ops.wsola, TimeScaler next to the two existing ways to move samples along time
(ops.pv_synth at the same stretch, which changes the duration in the STFT domain, and ops.psola at ratio 1), and the
gender recipe's train step with the scaler in front.  The utterances are data.synthetic_gender_dataset's.

Device events around each call after a warm-up; the median of --steps calls.  Every figure is a call THROUGH THE BINDING:
the launch and the binding's allocations are inside it.  Nothing is asserted on the times.  Prints one JSON line (and
writes it to --out); per tempo (``tempo_0.5`` ...):
  quant_ms, search_ms, ola_ms   ops.wsola_quant, ops.wsola_search, ops.wsola_ola;  wsola_ms: ops.wsola, the three in a row
  steps, us_per_step            the chain steps of the longest row (count - 1) and search_ms over them
  jumps                         the windows of the batch that do not continue their predecessor, over all windows
  scaler_ms                     TimeScaler(tempo) with the lengths on the CPU, the whole call
  pv_synth_ms                   ops.pv_synth of the batch's STFT to round((T - 1) / tempo) + 1 frames (no STFT, no ISTFT)
and once:  psola_ms (ops.psola at ratio 1 with the tracker's f0),  step_ms (the tempo recipe's fit_batch at tempo 0.8),
step_plain_ms (GenderBrain.fit_batch without the scaler, on the same settings and batch)."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from tools.bench_common import bench_brain, time_calls, write_line  # noqa: E402

SR = 16000
TEMPOS = (0.5, 0.8, 1.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the recipe-step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wsola_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    from speech_anonymization_amd import data, ops, pitchnorm, timescale
    B, N = a.B, int(a.seconds * SR)
    batch = next(iter(data.synthetic_gender_dataset(B, B, n_samples=N)))
    wav, lens = batch.sig[0].to(dev).contiguous(), batch.sig[1].float()
    nv = pitchnorm.n_valid(lens, N, dev).to(torch.int32)
    out = {"B": B, "N": N, "steps": a.steps}
    tm = lambda fn: round(time_calls(fn, a.warmup, a.steps), 4)
    _, R = pitchnorm.padded_stft(wav)
    T = R.shape[1]
    for tempo in TEMPOS:
        tq = torch.full((B,), timescale.tempo_to_q(tempo), dtype=torch.int32, device=dev)
        Nout = max(ops.wsola_out_len(int(v), int(tq[0])) for v in nv.cpu().tolist())
        ws = ops.wsola_workspace(B, N, dev)
        q = ops.wsola_quant(wav, nv, ws)
        pos, count, n_out = ops.wsola_search(q, tq, nv, Nout)
        moved = (pos[:, 1:] != pos[:, :-1] + ops.WSOLA_H) & (torch.arange(1, pos.shape[1], device=dev) < count[:, None])
        res = {"Nout": Nout, "steps": int(count.max()) - 1,
               "jumps": round(float(moved.sum()) / max(1, int((count - 1).clamp(min=0).sum())), 4)}
        res["quant_ms"] = tm(lambda: ops.wsola_quant(wav, nv, ws))
        res["search_ms"] = tm(lambda: ops.wsola_search(q, tq, nv, Nout))
        res["ola_ms"] = tm(lambda: ops.wsola_ola(wav, pos, count, tq, nv, Nout))
        res["wsola_ms"] = tm(lambda: ops.wsola(wav, tq, nv, Nout))
        res["us_per_step"] = round(1e3 * res["search_ms"] / max(1, res["steps"]), 4)
        ts = timescale.TimeScaler(tempo)
        res["scaler_ms"] = tm(lambda: ts(wav, lens))
        ratio = torch.full((B,), 1.0 / tempo, dtype=torch.float32, device=dev)
        Tout = int(round((T - 1) / tempo)) + 1
        res["pv_synth_ms"] = tm(lambda: ops.pv_synth(R, ratio, Tout))
        out[f"tempo_{tempo:g}"] = res
    f0 = ops.yin_f0(wav)
    rho_q = torch.full(f0.shape, 1 << 16, dtype=torch.int32, device=dev)
    out["psola_ms"] = tm(lambda: ops.psola(wav, f0, rho_q, nv))

    if not a.no_step:
        with tempfile.TemporaryDirectory() as tmp:
            for name, plain in (("step_ms", False), ("step_plain_ms", True)):
                b = bench_brain("gender_classifier_train_tempo", B, tmp, plain=plain)
                out[name] = tm(lambda: b.fit_batch(batch))
                del b
                torch.cuda.empty_cache()
    write_line(out, a.out)


if __name__ == "__main__":
    main()
