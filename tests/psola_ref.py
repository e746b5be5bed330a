"""TD-PSOLA pitch modification (include/sa_hip.h states the algorithm): the restatement in integers
and fp64 that the kernels of csrc/sa_psola.hip are held against -- marks and plan exactly, the overlap-add within a
rounding bar -- and the fp32-accumulating variant of the overlap-add, in the header's order, that the bar is measured
with (tools/psola_delta.py).  Also the test material both use."""
import numpy as np
import torch

from tests import contour_ref as CR
from tests import pitch_ref as P

HOP, U = 160, 80
P_MIN, P_MAX = 40, 266
S_MIN, S_MAX = 30, 332
RHO_ONE = 1 << 16
EDGE = CR.EDGE


def mcap(N):
    return N // 30 + 2


def jcap(N):
    return N // 15 + 2


def frame(n, T):
    return min((n + 80) // HOP, T - 1)


def periods(f0, nv):
    """per [T] int of one row: f0 [T] (the fp32 values), nv the row's valid samples"""
    f0 = np.asarray(f0, dtype=np.float32)
    T = f0.shape[0]
    F_b = min(T, nv // HOP + 1)
    per = np.zeros(T, dtype=np.int64)
    for t in range(F_b):
        if f0[t] > 0:                                            # (a NaN is not)
            per[t] = int(min(max(np.rint(16000.0 / np.float64(f0[t])), float(P_MIN)), float(P_MAX)))
    return per


def argmax(x, lo, hi):
    """the first index of the largest sample of x[lo..hi], a NaN counting as -inf"""
    w = np.array(x[lo:hi + 1], dtype=np.float32)
    w[np.isnan(w)] = -np.inf
    return lo + int(np.argmax(w))


def marks(wav, f0, nv):
    """one row: wav [N] fp32, f0 [T], nv -> the analysis marks, a list of ints"""
    wav = np.asarray(wav, dtype=np.float32)
    N, T = wav.shape[0], len(f0)
    nv = min(max(int(nv), 0), N)
    per = periods(f0, nv)
    out = []
    lo, hi = 0, (int(per[0]) - 1 if per[0] > 0 else 0)
    while hi < nv:
        m = argmax(wav, lo, hi)
        out.append(m)
        p = int(per[frame(m, T)])
        lo, hi = (m + p - (p >> 2), m + p + (p >> 2)) if p > 0 else (m + U, m + U)
    assert len(out) <= mcap(N)
    return out


def plan(mk, f0, rho_q, nv, N):
    """one row: the marks, f0 [T], rho_q [T] ints, nv, N -> (syn_pos, syn_src), two lists; empty under 2 marks"""
    T, M = len(f0), len(mk)
    if M < 2:
        return [], []
    nv = min(max(int(nv), 0), N)
    per = periods(f0, nv)
    pos, src = [], []
    s, a, last = mk[0] << 16, 0, mk[-1] << 16
    while s <= last:
        while a + 1 < M and abs((mk[a + 1] << 16) - s) < abs((mk[a] << 16) - s):
            a += 1
        pos.append((s + (1 << 15)) >> 16)
        src.append(a)
        period = mk[a + 1] - mk[a] if a + 1 < M else mk[a] - mk[a - 1]
        t = frame(mk[a], T)
        r = min(max(int(rho_q[t]), RHO_ONE // 2), 2 * RHO_ONE) if per[t] > 0 else RHO_ONE
        s += period * (((1 << 32) + r // 2) // r)
    assert len(pos) <= jcap(N)
    return pos, src


def ola(wav, mk, pos, src, nv, fp32=False):
    """one row: the overlap-add of a plan -> out [N], fp64; fp32: the weights rounded once to fp32 and products, sums
    and quotient in fp32, grain after grain in ascending j as the header orders them (the values are then fp32's)"""
    wav32 = np.asarray(wav, dtype=np.float32)
    N = wav32.shape[0]
    nv = min(max(int(nv), 0), N)
    kind = np.float32 if fp32 else np.float64
    x = wav32.astype(kind)
    out = np.zeros(N, dtype=kind)
    M, J = len(mk), len(pos)
    if M < 2 or J < 1:
        out[:nv] = x[:nv]
        return out.astype(np.float64)
    acc, wsum = np.zeros(N, dtype=kind), np.zeros(N, dtype=kind)
    for j in range(J):
        a = src[j]
        m = mk[a]
        below = m - mk[a - 1] if a > 0 else mk[1] - m
        above = mk[a + 1] - m if a + 1 < M else below
        L, R = (below if a > 0 else above), above
        d_lo = -m if j == 0 else -(L - 1)                        # rectangular: down to source sample 0
        d_hi = nv - 1 - m if j == J - 1 else R - 1               # rectangular: up to source sample nv - 1
        d = np.arange(d_lo, d_hi + 1)
        d = d[(m + d >= 0) & (m + d < nv) & (pos[j] + d >= 0) & (pos[j] + d < nv)]
        h = np.where(d < 0, L, R).astype(np.float64)
        w = 0.5 * (1.0 + np.cos(np.pi * d.astype(np.float64) / h))
        w[d == 0] = 1.0
        if j == 0:
            w[d < 0] = 1.0
        if j == J - 1:
            w[d > 0] = 1.0
        if fp32:
            w = w.astype(np.float32)
        n = pos[j] + d
        acc[n] = acc[n] + w * x[m + d]
        wsum[n] = wsum[n] + w
    out[:nv] = (acc / np.maximum(wsum, kind(0.5)))[:nv]
    return out.astype(np.float64)


def tables(wav, f0, rho_q, nv):
    """[B, N], [B, T], [B, T], [B] -> per row (marks, syn_pos, syn_src)"""
    wav = np.asarray(torch.as_tensor(wav, dtype=torch.float32))
    f0 = np.asarray(torch.as_tensor(f0, dtype=torch.float32))
    rho_q, nv = np.asarray(rho_q), np.asarray(nv)
    rows = []
    for b in range(wav.shape[0]):
        mk = marks(wav[b], f0[b], int(nv[b]))
        rows.append((mk,) + plan(mk, f0[b], rho_q[b], int(nv[b]), wav.shape[1]))
    return rows


def psola(wav, f0, rho_q, nv, fp32=False, rows=None):
    """the whole path -> out fp64 [B, N] (a torch tensor); rows: ``tables`` of the same inputs, if at hand"""
    w = np.asarray(torch.as_tensor(wav, dtype=torch.float32))
    rows = tables(wav, f0, rho_q, nv) if rows is None else rows
    return torch.from_numpy(np.stack([ola(w[b], *rows[b], int(np.asarray(nv)[b]), fp32) for b in range(w.shape[0])]))


def constant_rho(ratio, T):
    """ratio [B] (the fp32 values) -> rho_q int64 [B, T] = rint(ratio 2^16), as PitchNormalizer forms it"""
    r = torch.as_tensor(ratio, dtype=torch.float32).double()
    return torch.round(r * RHO_ONE).long()[:, None].expand(-1, T).contiguous()


def normalize(wav, lens, target_hz=170.0, gamma=None, smooth=2, r_min=0.5, r_max=2.0, min_voiced=5):
    """PitchNormalizer(psola=True) restated: YIN -> the ratio (gamma None) or the contour's ratio per frame -> psola.
    -> (out fp64 [B, N], rho_q [B, T], f0 [B, T])"""
    wav = torch.as_tensor(wav, dtype=torch.float32)
    N = wav.shape[1]
    f0 = P.yin(wav.double())[0].float()
    if gamma is None:
        rho_q = constant_rho(P.ratio(f0, lens, N, target_hz, r_min, r_max, min_voiced)[0].float(), f0.shape[1])
    else:
        rho_q = CR.contour(f0, lens, N, target_hz, gamma, smooth, r_min, r_max, min_voiced).rho_q
    return psola(wav, f0, rho_q, P.n_valid(lens, N)), rho_q, f0


# ---- the test material ---------------------------------------------------------------------------------
N_GPU = 4000


def gpu_case():
    """the kernel test's batch: (wav fp32 [5, 4000], f0 fp32 [5, 26], rho_q int32 [5, 26], n_valid int32 [5]) -- a
    110 Hz voice in noise; a 200 -> 260 Hz glide whose frames 9..13 are marked unvoiced; noise with no voiced frame; a
    voiced row of 700 valid samples; a row of none.  rho_q: 1, 1.417, a ramp over the whole range, 0.5, and values
    outside the range (0 and 2^20) that read as its bounds."""
    g = torch.Generator().manual_seed(2424)
    N, T = N_GPU, N_GPU // HOP + 1
    wav = torch.stack([P.harmonic_row(110.0, N, g, noise=0.05),
                       CR.glide_row(lambda t: 200.0 + 60.0 * t / (N / P.SR), N, g),
                       0.1 * torch.randn(N, generator=g, dtype=torch.float64),
                       P.harmonic_row(140.0, N, g), P.harmonic_row(180.0, N, g)]).float()
    t = torch.arange(T, dtype=torch.float64)
    f0 = torch.stack([torch.full((T,), 110.0, dtype=torch.float64), 200.0 + 60.0 * t / (T - 1),
                      torch.zeros(T, dtype=torch.float64), torch.full((T,), 140.0, dtype=torch.float64),
                      torch.full((T,), 180.0, dtype=torch.float64)]).float()
    f0[1, 9:14] = 0.0
    rho_q = torch.stack([torch.full((T,), RHO_ONE), torch.full((T,), int(np.rint(1.417 * RHO_ONE))),
                         torch.round((RHO_ONE // 2) + t * (3 * RHO_ONE // 2) / (T - 1)).long(),
                         torch.full((T,), RHO_ONE // 2),
                         torch.where(t.long() % 2 == 0, 0, 1 << 20)]).to(torch.int32)
    n_valid = torch.tensor([N, N, N, 700, 0], dtype=torch.int32)
    return wav, f0, rho_q, n_valid


def short_case():
    """a row of 159 samples, one frame: (wav [1, 159], f0 [1, 1], rho_q [1, 1], n_valid [1])"""
    g = torch.Generator().manual_seed(2425)
    return (P.harmonic_row(300.0, 159, g)[None].float(), torch.full((1, 1), 300.0), torch.full((1, 1), 80000,
            dtype=torch.int32), torch.tensor([159], dtype=torch.int32))


def tie_case(N=2000):
    """every sample 0.25 under a voiced f0 of 200 Hz: every window's argmax is its first sample"""
    T = N // HOP + 1
    return (torch.full((1, N), 0.25), torch.full((1, T), 200.0), torch.full((1, T), int(1.25 * RHO_ONE),
            dtype=torch.int32), torch.tensor([N], dtype=torch.int32))


def kernel_cases():
    return {"batch": gpu_case(), "short": short_case(), "tie": tie_case()}


def gap_row():
    """a resonance row (tests/formant_ref.py's first) with 2000 samples of weak noise in its middle, and its YIN
    track: (wav fp32 [1, 8000], f0 fp32 [1, 51])"""
    from tests import formant_ref as F
    g = torch.Generator().manual_seed(2426)
    w = F.resonance_row(*F.ROWS[0]).clone()
    w[3000:5000] = 0.01 * torch.randn(2000, generator=g, dtype=torch.float64)
    w = w[None].float()
    return w, P.yin(w.double())[0].float()


def end_to_end_rows():
    """the rows the F0 and peak bars are measured on: formant_ref's three resonance rows and four harmonic rows, all
    8000 samples: fp32 [7, 8000]"""
    from tests import formant_ref as F
    g = torch.Generator().manual_seed(2427)
    return torch.cat([F.resonance_rows(), torch.stack([P.harmonic_row(f, F.ROW_SAMPLES, g)
                                                       for f in (95.0, 140.0, 210.0, 300.0)]).float()])


def voiced_mean_f0(f0, lens, N):
    """the voiced mean of a track, EDGE frames left out at either end: fp64 [B]"""
    return CR.f0_stats(f0, lens, N)[0]
