#!/usr/bin/env python3
"""SHA-256 digests of what the LPC entry points compute, for comparing two builds of the library bit for bit on one GPU
(SA_HIP_LIB selects the build; one process per build):

    python tools/lpc_digest.py [--device cuda:0] [--out FILE]

One digest per output tensor of ops.mcadams, ops.pole_warp and ops.srcfilt_synth (its excitation by ops.srcfilt_pulses
and ops.srcfilt_excite on the batch's YIN track), each with level on and off and with its status;
ops.formant_tracks with its bandwidths; ops.formant_compare of the batch's tracks against its McAdams output's; and
ops.formant_centre with and without f0.  What tools/anon_digest.py does not see: the statuses, level off, the
bandwidths, sa_formant_compare.  The inputs: the first batch of data.synthetic_gender_dataset(3, 3); the width-16037
batch of anon_digest.inputs() with lens (1.0, 0.73, 0.5); that batch with row 0 all zero and the parameter of row 1
exactly 1; and it with the parameters at and beyond both clamp bounds of either entry point."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.anon_digest import inputs, sha  # noqa: E402
from speech_anonymization_amd import ops  # noqa: E402
from speech_anonymization_amd.pitchnorm import n_valid  # noqa: E402

TARGET_HZ = (500.0, 1500.0, 2500.0)


def cases():
    """name -> (wav [3, N], lens [3], alpha [3], q [3]) on the host"""
    named = inputs()
    syn, lens = named["synthetic_6_3"][0]       # (the first batch of (6, 3) is the first of (3, 3): one seed, in order)
    odd, cut = named["width_16037"][0]
    zero = odd.clone()
    zero[0] = 0.0
    return {"synthetic_3_3": (syn, lens, [0.8, 0.9, 1.1], [0.9, 1.1, 1.2]),
            "width_16037": (odd, cut, [0.8, 0.9, 1.1], [0.9, 1.1, 1.2]),
            "zero_row_and_one": (zero, cut, [0.8, 1.0, 1.1], [0.9, 1.0, 1.2]),
            "clamp_low": (odd, cut, [0.25, 0.2, -3.0], [0.5, 0.4, -3.0]),
            "clamp_high": (odd, cut, [2.0, 2.5, float("inf")], [2.0, 2.5, float("inf")])}


def main(argv):
    device = argv[argv.index("--device") + 1] if "--device" in argv else "cuda:0"
    torch.cuda.set_device(torch.device(device))
    res = {}

    def put(name, tensors):
        for j, t in enumerate(tensors):
            res[f"{name}/{j}"] = sha(t)

    for name, (wav, lens, alpha, q) in cases().items():
        wav = wav.to(device).contiguous()
        B, N = wav.shape
        nv = n_valid(lens, N, device).to(torch.int32)
        alpha, q = (torch.tensor(v, dtype=torch.float32, device=device) for v in (alpha, q))
        f0 = ops.yin_f0(wav)
        pos_q, period_q, count = ops.srcfilt_pulses(f0, None, nv, N=N)
        exc = ops.srcfilt_excite(f0, pos_q, period_q, count, torch.arange(B, dtype=torch.int32, device=device), nv, N=N)
        put(f"{name}/excitation", (pos_q * (torch.arange(pos_q.shape[1], device=device) < count[:, None]), count, exc))
        for level in (True, False):
            put(f"{name}/mcadams/level_{level}", ops.mcadams(wav, alpha, nv, level, return_status=True))
            put(f"{name}/pole_warp/level_{level}", ops.pole_warp(wav, q, nv, level, return_status=True))
            put(f"{name}/srcfilt_synth/level_{level}", ops.srcfilt_synth(wav, exc, nv, level, return_status=True))
        frames = (nv // 160 + 1).to(torch.int32)
        freq, status, bw = ops.formant_tracks(wav, nv, return_bw=True)
        put(f"{name}/formant_tracks", (freq, bw, status))
        deg = ops.formant_tracks(ops.mcadams(wav, alpha, nv)[0], nv)
        put(f"{name}/formant_compare", ops.formant_compare(freq, deg[0], status, deg[-1], f0, f0, frames))
        put(f"{name}/formant_centre/f0", ops.formant_centre(freq, status, f0, frames, TARGET_HZ))
        put(f"{name}/formant_centre/no_f0", ops.formant_centre(freq, status, None, frames, TARGET_HZ))
    text = json.dumps(res, indent=1, sort_keys=True) + "\n"
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
