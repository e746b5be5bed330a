"""fp64 restatement of the pitch normalisation (speech_anonymization_amd.pitchnorm and
csrc/sa_pitch.hip), on the CPU: YIN by direct sums, the ratio, the stretch of the STFT magnitudes, Griffin-Lim on
torch.stft / torch.istft in double, and the windowed-sinc resampling by direct sums.  Shared by
tests/test_pitchnorm_cpu.py, tests/test_pitchnorm_gpu.py and tools/pitch_norm_delta.py."""
import math

import numpy as np
import torch

from speech_anonymization_amd.features import _hamming

SR, HOP, W, TAU_MIN, TAU_MAX = 16000, 160, 400, 40, 266
L = W + TAU_MAX
U = 2.0 ** -24
EPS_DPRIME = (W + TAU_MAX + 8) * U       # d is a sum of W non-negative terms, c of <= tau_max: any order stays inside


# ---- (1) F0 ---------------------------------------------------------------------------------------------
def frames(wav):
    """wav [B, N] -> x [B, T, L] fp64: x[b, t, j] = wav[b, 160 t - 333 + j], zeros outside [0, N)"""
    wav = torch.as_tensor(wav, dtype=torch.float64)
    B, N = wav.shape
    T = N // HOP + 1
    left = L // 2
    right = max(0, HOP * (T - 1) - left + L - N)
    return torch.nn.functional.pad(wav, (left, right)).unfold(1, L, HOP)[:, :T]


def yin_dprime(wav):
    """d' [B, T, tau_max + 1] fp64"""
    x = frames(wav)
    d = torch.zeros(x.shape[0], x.shape[1], TAU_MAX + 1, dtype=torch.float64)
    for tau in range(1, TAU_MAX + 1):
        d[..., tau] = ((x[..., :W] - x[..., tau:tau + W]) ** 2).sum(-1)
    c = d.cumsum(-1)
    tau = torch.arange(TAU_MAX + 1, dtype=torch.float64)
    dp = torch.where(c > 0, d * tau / torch.where(c > 0, c, torch.ones_like(c)), torch.ones_like(c))
    dp[..., 0] = 1.0
    return dp


def yin_pick(dp, threshold=0.15):
    """p [B, T] int64 (0: unvoiced): the smallest tau in [tau_min, tau_max - 1] that is under the threshold, not above
    its left neighbour and below its right one"""
    c = dp[..., TAU_MIN:TAU_MAX]
    ok = (c < threshold) & (c <= dp[..., TAU_MIN - 1:TAU_MAX - 1]) & (c < dp[..., TAU_MIN + 1:TAU_MAX + 1])
    first = ok.to(torch.int64).argmax(-1) + TAU_MIN
    return torch.where(ok.any(-1), first, torch.zeros_like(first))


def interpolate(dp, p):
    """f0 [B, T] fp64 from the picks (0 stays 0)"""
    q = p.clamp(min=1)
    a = dp.gather(-1, (q - 1)[..., None])[..., 0]
    c = dp.gather(-1, q[..., None])[..., 0]
    e = dp.gather(-1, (q + 1).clamp(max=TAU_MAX)[..., None])[..., 0]
    den = a - 2 * c + e
    off = torch.where(den > 0, 0.5 * (a - e) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    return torch.where(p > 0, SR / (q.double() + off), torch.zeros_like(off))


def yin(wav, threshold=0.15):
    """-> (f0 [B, T] fp64, d' [B, T, 267], p [B, T])"""
    dp = yin_dprime(wav)
    p = yin_pick(dp, threshold)
    return interpolate(dp, p), dp, p


def stable(dp, p, threshold=0.15, eps=EPS_DPRIME):
    """[B, T] bool: no scaling of the d' by factors in [1 - eps, 1 + eps] changes the decision.  Every lag up to the
    pick (all of [tau_min, tau_max - 1] on an unvoiced frame) must keep its verdict: a rejected lag has at least one
    of its three comparisons false by a margin, the picked lag all three true by a margin; and on a voiced frame
    den >= 64 eps (a + 2 c + e)."""
    c, lft, rgt = dp[..., TAU_MIN:TAU_MAX], dp[..., TAU_MIN - 1:TAU_MAX - 1], dp[..., TAU_MIN + 1:TAU_MAX + 1]
    lo, hi = 1.0 - eps, 1.0 + eps
    surely_true = (c * hi < threshold) & (c * hi <= lft * lo) & (c * hi < rgt * lo)
    surely_false = (c * lo >= threshold) | (c * lo > lft * hi) | (c * lo >= rgt * hi)
    tau = torch.arange(TAU_MIN, TAU_MAX)
    voiced = p > 0
    before = tau < torch.where(voiced, p, torch.full_like(p, TAU_MAX))[..., None]
    at = tau == p[..., None]
    ok = (surely_false | ~before).all(-1) & ((surely_true | ~at).all(-1))
    q = p.clamp(min=1)
    a = dp.gather(-1, (q - 1)[..., None])[..., 0]
    cc = dp.gather(-1, q[..., None])[..., 0]
    e = dp.gather(-1, (q + 1).clamp(max=TAU_MAX)[..., None])[..., 0]
    return ok & (~voiced | (a - 2 * cc + e >= 64 * eps * (a + 2 * cc + e)))


def f0_bound(dp, p, eps=EPS_DPRIME):
    """first-order bound of |delta f0| [B, T] when a, c, e = d'(p - 1), d'(p), d'(p + 1) each move by eps relative:
    off = (a - e) / (2 den), den = a - 2 c + e; f0 = 16000 / (p + off)"""
    q = p.clamp(min=1)
    a = dp.gather(-1, (q - 1)[..., None])[..., 0]
    c = dp.gather(-1, q[..., None])[..., 0]
    e = dp.gather(-1, (q + 1).clamp(max=TAU_MAX)[..., None])[..., 0]
    den = (a - 2 * c + e).clamp(min=1e-300)
    g = 0.5 * (a - e) / den ** 2
    doff = eps * (a * (0.5 / den - g).abs() + c * (2 * g).abs() + e * (-0.5 / den - g).abs())
    off = 0.5 * (a - e) / den
    return SR / (q.double() + off) ** 2 * doff


# ---- (2) ratio ------------------------------------------------------------------------------------------
def n_valid(lens, N):
    return torch.round(torch.as_tensor(lens).double() * N).long().clamp(0, N)


def ratio(f0, lens, N, target_hz=170.0, r_min=0.5, r_max=2.0, min_voiced=5):
    """-> (ratio fp64 [B], mean fp64 [B], voiced int64 [B])"""
    f0 = torch.as_tensor(f0, dtype=torch.float64)
    B, T = f0.shape
    F = (n_valid(lens, N) // HOP + 1).clamp(max=T)
    r, m, v = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        row = f0[b, :int(F[b])]
        vo = row[row > 0]
        v[b] = vo.numel()
        if vo.numel():
            m[b] = vo.sum() / vo.numel()
        if vo.numel() >= min_voiced and m[b] > 0:
            r[b] = min(max(target_hz / float(m[b]), r_min), r_max)
    return r, m, v


# ---- (3) stretch ----------------------------------------------------------------------------------------
def window():
    return torch.from_numpy(_hamming(400).astype(np.float64))


def stft(y):
    """[B, N] fp64, N a multiple of 160 -> complex128 [B, N / 160 + 1, 201] (center=True, zero padding)"""
    return torch.stft(y, 400, 160, 400, window=window(), center=True, pad_mode="constant",
                      return_complex=True).transpose(1, 2)


def istft(C):
    """complex128 [B, T, 201] -> [B, (T - 1) 160]"""
    return torch.istft(C.transpose(1, 2), 400, 160, 400, window=window(), center=True,
                       length=(C.shape[1] - 1) * HOP)


def stretched_frames(Tp, r):
    return int(math.ceil((Tp - 1) * float(r))) + 1


def stretch(mag, r):
    """mag [B, T, K] fp64 (|R|), r [B] -> (S' [B, T', K] fp64, the neighbours' sum |R_i| + |R_{i+1}| per element for
    the error bound, [T'_b])"""
    mag = torch.as_tensor(mag, dtype=torch.float64)
    B, T, K = mag.shape
    Tb = [stretched_frames(T, x) for x in r]
    S = torch.zeros(B, max(Tb), K, dtype=torch.float64)
    nb = torch.zeros_like(S)
    for b in range(B):
        pos = (torch.arange(Tb[b], dtype=torch.float64) / float(r[b])).clamp(max=T - 1)
        i = pos.floor().long().clamp(max=T - 2)
        a = (pos - i)[:, None]
        S[b, :Tb[b]] = (1 - a) * mag[b, i] + a * mag[b, i + 1]
        nb[b, :Tb[b]] = mag[b, i] + mag[b, i + 1]
    return S, nb, Tb


# ---- (4) phase ------------------------------------------------------------------------------------------
def griffin_lim(S, phi, n_iter=32, momentum=0.99):
    """the loop of vocoder.GriffinLim in fp64; m = momentum / (1 + momentum) as fp32 rounds it"""
    m = float(np.float32(momentum / (1.0 + momentum)))
    S = torch.as_tensor(S, dtype=torch.float64)
    C = torch.polar(S, torch.as_tensor(phi, dtype=torch.float64))
    Tprev = torch.zeros_like(C)
    for _ in range(n_iter):
        R = stft(istft(C))
        A = R - m * Tprev
        C = S * A / (A.abs() + 1e-16)
        Tprev = R
    return istft(C)


# ---- (5) resample ---------------------------------------------------------------------------------------
def input_end(Nin, Nout, r):
    """samples of row b's input that count: (T'_b - 1) 160 of a waveform of Nout samples, at most Nin"""
    return min(Nin, HOP * int(math.ceil(-(-Nout // HOP) * float(r))))


def resample(y, r, nv, Nout):
    """y [B, Nin] fp64, r [B], nv [B] -> (out [B, Nout] fp64, sum_i |h| |y| per sample, taps per sample)"""
    y = torch.as_tensor(y, dtype=torch.float64)
    B, Nin = y.shape
    out = torch.zeros(B, Nout, dtype=torch.float64)
    mass = torch.zeros_like(out)
    taps = torch.zeros(B, Nout, dtype=torch.int64)
    for b in range(B):
        rb, n = float(r[b]), int(nv[b])
        c = min(1.0, 1.0 / rb)
        H = 16.0 / c
        end = input_end(Nin, Nout, rb)
        pos = torch.arange(n, dtype=torch.float64) * rb
        i = ((pos - H).floor().long() + 1)[:, None] + torch.arange(66)[None, :]
        u = pos[:, None] - i
        live = (u.abs() < H) & (i >= 0) & (i < end)
        h = c * torch.sinc(c * u) * (0.5 + 0.5 * torch.cos(math.pi * u / H))
        h = torch.where(live, h, torch.zeros_like(h))
        yy = y[b][i.clamp(0, Nin - 1)]
        out[b, :n] = (h * yy).sum(-1)
        mass[b, :n] = (h.abs() * yy.abs()).sum(-1)
        taps[b, :n] = live.sum(-1)
    return out, mass, taps


# ---- the whole path -------------------------------------------------------------------------------------
def normalize(wav, lens, phi_of, target_hz=170.0, n_iter=32, momentum=0.99, r_min=0.5, r_max=2.0, min_voiced=5,
              threshold=0.15):
    """wav [B, N], lens [B] -> (out [B, N] fp64, ratio, mean, voiced).  phi_of(shape) gives the starting phases.
    The ratio is rounded to fp32 where the kernels read it."""
    wav = torch.as_tensor(wav, dtype=torch.float64)
    B, N = wav.shape
    f0 = yin(wav, threshold)[0]
    r, mean, voiced = ratio(f0, lens, N, target_hz, r_min, r_max, min_voiced)
    r = r.float().double()
    Np = HOP * -(-N // HOP)
    S, _, _ = stretch(stft(torch.nn.functional.pad(wav, (0, Np - N))).abs(), r)
    y = griffin_lim(S, phi_of(S.shape), n_iter, momentum)
    return resample(y, r, n_valid(lens, N), N)[0], r, mean, voiced


def voiced_mean(f0, lens, N):
    """(mean of the voiced f0, voiced count, frames that count) per row, as the ratio step sees them"""
    _, m, v = ratio(f0, lens, N, min_voiced=0)
    return m, v, (n_valid(lens, N) // HOP + 1).clamp(max=f0.shape[1])


def harmonic_row(f, n, gen, noise=0.02):
    """one row as data.synthetic_gender_dataset makes them: 8 partials with random decaying amplitudes and phases at
    the fundamental f, plus white noise; fp64 [n]"""
    t = torch.arange(n, dtype=torch.float64) / SR
    w = noise * torch.randn(n, generator=gen, dtype=torch.float64)
    for h in range(1, 9):
        amp = 0.3 / h * (0.5 + torch.rand(1, generator=gen, dtype=torch.float64))
        ph = 2 * math.pi * torch.rand(1, generator=gen, dtype=torch.float64)
        w += amp * torch.sin(2 * math.pi * h * f * t + ph)
    return w


def yin_case(N):
    """the five rows of the GPU test of sa_yin_f0 as fp32 [5, N]: harmonic rows at 62, 395 and 150 Hz (the last with
    its tail zeroed from 0.6 N), white noise 0.1, silence"""
    g = torch.Generator().manual_seed(2002)
    rows = [harmonic_row(62.0, N, g), harmonic_row(395.0, N, g), harmonic_row(150.0, N, g),
            0.1 * torch.randn(N, generator=g, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)]
    rows[2][int(0.6 * N):] = 0.0
    return torch.stack(rows).float()
