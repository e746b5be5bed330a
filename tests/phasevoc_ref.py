"""fp64 restatement of the phase-vocoder resynthesis (ops.pv_synth and csrc/sa_phasevoc.hip) on
the CPU, on top of tests/pitch_ref.py: the phase carried through the stretch, the synthesis, the whole pitch path
with it, and the cases tools/phasevoc_delta.py reports on.  Phases are in turns (1 turn = 2 pi).  Shared by
tests/test_phasevoc_cpu.py, tests/test_phasevoc_gpu.py and tools/phasevoc_delta.py."""
import math

import torch

from tests import pitch_ref as P

NBIN = 201
OMEGA = 0.4                              # expected phase advance of bin k per hop, in turns: 160 k / 400


def theta(R):
    """R complex [B, T, K] -> its phase in turns, fp64 (atan2 of the parts: IEEE signed zeros, (0, 0) -> 0)"""
    R = torch.as_tensor(R).to(torch.complex128)
    return torch.atan2(R.imag, R.real) / (2.0 * math.pi)


def positions(T, r):
    """(T', i [T'], a [T']) of one row: the frames the stretch reads and the weight of frame i + 1"""
    Tb = P.stretched_frames(T, r)
    pos = (torch.arange(Tb, dtype=torch.float64) / float(r)).clamp(max=T - 1)
    i = pos.floor().long().clamp(max=T - 2)
    return Tb, i, pos - i


def circular(a, b):
    """the distance of two phases on the circle, in turns"""
    d = (a - b) % 1.0
    return torch.minimum(d, 1.0 - d)


def increments(th, i, form="plain"):
    """the phase advance of every output step [T', K]: theta[i + 1] - theta[i], or the textbook form Omega_k +
    wrap(theta[i + 1] - theta[i] - Omega_k) with the wrap to [-1/2, 1/2) -- equal mod 1"""
    d = th[i + 1] - th[i]
    if form == "plain":
        return d
    om = OMEGA * torch.arange(th.shape[-1], dtype=torch.float64)
    dev = d - om
    return om + (dev - torch.floor(dev + 0.5))


def pv_phase(R, r, form="plain", order="step"):
    """phi' [B, max T'_b, K] fp64, 0 from T'_b on.  order "step": the recurrence, reduced mod 1 at every step;
    "cumsum": one unreduced cumulative sum, reduced at the end (another summation order, for the spread)"""
    th = theta(R)
    B, T, K = th.shape
    rows = [positions(T, x) for x in r]
    phi = torch.zeros(B, max(tb for tb, _, _ in rows), K, dtype=torch.float64)
    for b, (Tb, i, _) in enumerate(rows):
        d = increments(th[b], i, form)
        if order == "cumsum":
            phi[b, 0] = th[b, 0] % 1.0
            phi[b, 1:Tb] = (th[b, 0] + d[:Tb - 1].cumsum(0)) % 1.0
            continue
        acc = th[b, 0] - torch.floor(th[b, 0])
        phi[b, 0] = acc
        for t in range(1, Tb):
            acc = acc + d[t - 1]
            acc = acc - torch.floor(acc)
            phi[b, t] = acc
    return phi


def pv_synth(R, r, S=None):
    """-> (C complex128 [B, max T'_b, K], phi', S' fp64, [T'_b]): S' (the caller's, or the stretch of |R|) under the
    carried phase; 0 from T'_b on"""
    R = torch.as_tensor(R).to(torch.complex128)
    phi = pv_phase(R, r)
    Sp, _, Tb = P.stretch(R.abs(), r)
    if S is not None:
        Sp = torch.as_tensor(S, dtype=torch.float64).clone()
        for b in range(len(Tb)):
            Sp[b, Tb[b]:] = 0.0
    return torch.polar(Sp, 2.0 * math.pi * phi), phi, Sp, Tb


def shift(wav, lens, r):
    """the path of PitchNormalizer.shift with phase="vocoder": STFT -> pv_synth -> ISTFT -> resampling; fp64 [B, N]"""
    wav = torch.as_tensor(wav, dtype=torch.float64)
    B, N = wav.shape
    Np = P.HOP * -(-N // P.HOP)
    C = pv_synth(P.stft(torch.nn.functional.pad(wav, (0, Np - N))), r)[0]
    return P.resample(P.istft(C), r, P.n_valid(lens, N), N)[0]


def normalize(wav, lens, target_hz=170.0, r_min=0.5, r_max=2.0, min_voiced=5, threshold=0.15):
    """wav [B, N], lens [B] -> (out [B, N] fp64, ratio, mean, voiced): pitch_ref.normalize with the phase vocoder in
    Griffin-Lim's place.  The ratio is rounded to fp32 where the kernels read it."""
    wav = torch.as_tensor(wav, dtype=torch.float64)
    r, mean, voiced = P.ratio(P.yin(wav, threshold)[0], lens, wav.shape[1], target_hz, r_min, r_max, min_voiced)
    r = r.float().double()
    return shift(wav, lens, r), r, mean, voiced


def delta_cases(target=170.0, report=None):
    """the 16 utterances of tools/pitch_norm_delta.py (4 batches of 4 of data.synthetic_gender_dataset) through
    ``normalize`` -> (worst |voiced mean - target| in Hz, smallest voiced share, largest distance in turns between the
    recurrence and the cumulative sum of step 3)"""
    from speech_anonymization_amd import data
    worst, low, spread = 0.0, 1.0, 0.0
    for batch in data.synthetic_gender_dataset(16, 4):
        wav, lens = batch.sig
        N = wav.shape[1]
        out, r, mean_in, _ = normalize(wav, lens, target_hz=target)
        mean, voiced, frames = P.voiced_mean(P.yin(out)[0], lens, N)
        share = voiced.double() / frames.double()
        R = P.stft(torch.nn.functional.pad(wav.double(), (0, P.HOP * -(-N // P.HOP) - N)))
        spread = max(spread, float(circular(pv_phase(R, r), pv_phase(R, r, order="cumsum")).max()))
        for b in range(wav.shape[0]):
            if report:
                report(f"f0 {float(mean_in[b]):7.2f} Hz, ratio {float(r[b]):.4f} -> {float(mean[b]):8.3f} Hz, "
                       f"voiced {int(voiced[b])} of {int(frames[b])}")
        worst, low = max(worst, float((mean - target).abs().max())), min(low, float(share.min()))
    return worst, low, spread
