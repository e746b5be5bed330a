#!/usr/bin/env python3
"""What plain fp32 arithmetic does to the feature front end, on the CPU: the figures the bars of
tests/test_frontend_gpu.py are made of.  Nothing here runs a kernel; the cases are the GPU test's own
(tests/fbank_ref.py: gpu_cases, norm_cases), the arbiter is that module's fp64 restatement.

    python tools/fbank_delta.py [--out profiles/fbank_delta.json]

  mel    the worst fbank_ref.mel_error, over every element of every case, of two fp32 evaluations:
           stft    oracle.features.Fbank in fp32: torch.stft, the reference's own arithmetic
           matmul  the restatement's formula in fp32: windowed frames @ cos / sin tables, squares, @ Mel matrix
         mel_bar = 8 x the worse of the two, POOLED over the cases: the kernel's 2-way bf16 split of the Mel
         product costs about 3 * 2^-18 on every energy however clean the spectrum is, so a bar taken case by
         case from fp32 (2e-7 on an impulse) would fail a correct kernel on the cleanest inputs.
  norm   the worst of fbank_ref.norm_errors (mean, std, output; in units of u = 2^-24) of
         oracle.features.InputNormalization in fp32 over the call sequence of every case; the case with an n = 1
         row is left out, the oracle's std is NaN there (fbank_ref's docstring).  norm_bar_u = 8 x the worst.
The margin 8 is that of tests/ref64.distance_tau."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import features as OF  # noqa: E402
from tests import fbank_ref as R  # noqa: E402

MARGIN = 8.0
U = 2.0 ** -24


def raw_db32(M):
    return 10.0 * torch.log10(torch.clamp(M, min=1e-10))


def mel_stft32(wav):
    fb = OF.Fbank()
    return raw_db32(torch.matmul(fb.power_spectrum(wav.float()), fb.fb))


def mel_matmul32(wav):
    c, s = (t.float() for t in R.dft_tables())
    x = R.frames(wav).float() * R.window().float()
    return raw_db32(((x @ c) ** 2 + (x @ s) ** 2) @ R.mel_matrix32())


def mel_delta():
    worst = {"stft": (0.0, None), "matmul": (0.0, None)}
    for name, wav in R.gpu_cases().items():
        ref = R.case_ref(name)
        for key, fn in (("stft", mel_stft32), ("matmul", mel_matmul32)):
            e = float(R.mel_error(fn(wav), ref).max())
            if e > worst[key][0]:
                worst[key] = (e, name)
    return worst


def oracle_sequence32(xs, lens, calls, state=None):
    """oracle.features.InputNormalization in fp32 through the calls -> [(out, gm, gs)] per call"""
    nrm = OF.InputNormalization(update_until_epoch=R.UNTIL)
    if state is not None:
        nrm.count, nrm.glob_mean, nrm.glob_std = state[0], state[1].float(), state[2].float()
    res = []
    for i, (training, epoch) in enumerate(calls):
        nrm.training = training
        out = OF.pad_to_multiple(nrm(xs[i % len(xs)], lens, epoch=epoch), 36)
        res.append((out, nrm.glob_mean.clone(), nrm.glob_std.clone()))
    return res


def norm_delta():
    worst = {"mean": (0.0, None), "std": (0.0, None), "out": (0.0, None)}
    for name, (xs, lens) in R.norm_cases().items():
        if int(R.frame_counts(lens.numpy(), xs[0].shape[1]).min()) < 2:
            continue                                                # torch.std of one frame is NaN
        fresh, loaded = R.norm_case_ref(name)
        got = oracle_sequence32(xs, lens, R.CALLS) + oracle_sequence32(xs, lens, R.LOAD_CALL, R.loaded_state())
        xseq = [xs[i % 2] for i in range(len(R.CALLS))] + [xs[0]]
        for (out, gm, gs), ref, x in zip(got, fresh + loaded, xseq):
            for key, e in zip(("mean", "std", "out"), R.norm_errors(out, gm, gs, x, ref)):
                if e > worst[key][0]:
                    worst[key] = (e, name)
    return worst


def measure():
    mel, nrm = mel_delta(), norm_delta()
    mel_worst = max(v[0] for v in mel.values())
    nrm_worst = max(v[0] for v in nrm.values())
    return {"margin": MARGIN,
            "mel_delta_stft": mel["stft"][0], "mel_delta_stft_case": mel["stft"][1],
            "mel_delta_matmul": mel["matmul"][0], "mel_delta_matmul_case": mel["matmul"][1],
            "mel_delta": mel_worst, "mel_bar": MARGIN * mel_worst,
            "floor_bar_db": R.floor_bound(MARGIN * mel_worst),
            "norm_delta_mean_u": nrm["mean"][0] / U, "norm_delta_mean_case": nrm["mean"][1],
            "norm_delta_std_u": nrm["std"][0] / U, "norm_delta_std_case": nrm["std"][1],
            "norm_delta_out_u": nrm["out"][0] / U, "norm_delta_out_case": nrm["out"][1],
            "norm_delta_u": nrm_worst / U, "norm_bar_u": MARGIN * nrm_worst / U}


def main(argv):
    res = measure()
    text = json.dumps(res, indent=1) + "\n"
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1:])
