"""The WSOLA time-scale modification of include/sa_hip.h restated with Python integers and numpy fp32, step by step as
the header numbers them.  The kernels of csrc/sa_wsola.hip agree with it exactly: q, pos, count, n_out, and every bit
of out.  The algorithm is numpy and Python integers; torch only carries the rows the other restatements generate."""
import math

import numpy as np

H, W, D, Q = 160, 320, 160, 16383
ONE = 1 << 16
CANON_NAN = np.uint32(0x7FC00000)


def clamp_tempo(tempo_q):
    return min(max(int(tempo_q), ONE // 2), 2 * ONE)


def out_len(n, tempo_q):
    """step 1 before the cap"""
    tq = clamp_tempo(tempo_q)
    n = int(n)
    return ((n << 16) + tq // 2) // tq if n > 0 else 0


def lengths(n_valid, tempo_q, N, Nout):
    """(n_valid clamped, n_out, K)"""
    nv = min(max(int(n_valid), 0), N)
    n_out = min(Nout, out_len(nv, tempo_q))
    return nv, n_out, ((n_out - 1) // H + 1 if n_out else 0)


def window():
    """hann[j] = 0.5 - 0.5 cos(2 pi j / W) in fp64, rounded once"""
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * j / W) for j in range(W)], dtype=np.float64).astype(np.float32)


def quant(wav, n_valid):
    """step 2: q int16 [N]"""
    wav = np.asarray(wav, dtype=np.float32)
    N = wav.shape[0]
    nv = min(max(int(n_valid), 0), N)
    q = np.zeros(N, dtype=np.int16)
    head = wav[:nv].astype(np.float64)
    fin = np.isfinite(head)
    s = float(np.abs(head[fin]).max()) if fin.any() else 0.0
    if s > 0.0:
        q[:nv][fin] = np.rint(head[fin] * 16383.0 / s).astype(np.int16)        # (numpy's rint: ties to even)
    return q


def step_cost(qp, t, lo, hi):
    """cost(c) for c = lo..hi against the template at t, on q padded with zeros (qp: int32)"""
    tmpl = qp[t:t + W]
    cand = np.lib.stride_tricks.sliding_window_view(qp[lo:hi + W], W)
    return np.abs(cand - tmpl[None, :]).sum(axis=1, dtype=np.int64)


def choose(cost, lo, a):
    """the candidate of least cost; ties to the smallest |c - a|, then to the smaller c"""
    c = lo + np.arange(cost.shape[0], dtype=np.int64)
    key = (cost.astype(np.int64) << 34) | (np.abs(c - a) << 25) | c
    return int(c[int(np.argmin(key))])


def positions(q, n_valid, tempo_q, Nout):
    """step 3: (pos list of K ints, n_out)"""
    q = np.asarray(q)
    N = q.shape[0]
    nv, n_out, K = lengths(n_valid, tempo_q, N, Nout)
    tq = clamp_tempo(tempo_q)
    qp = np.zeros(N + 2 * W + H + 8, dtype=np.int32)
    qp[:nv] = q[:nv]
    pos = [0] * K
    for k in range(1, K):
        a = (k * H * tq + (ONE >> 1)) >> 16
        t = pos[k - 1] + H
        lo, hi = max(a - D, 0), min(a + D, max(nv - 1, 0))
        if hi <= lo:
            pos[k] = hi
            continue
        pos[k] = choose(step_cost(qp, t, lo, hi), lo, a)
    return pos, n_out


def ola(wav, pos, n_valid, n_out, Nout):
    """step 4: out fp32 [Nout]"""
    wav = np.asarray(wav, dtype=np.float32)
    N = wav.shape[0]
    nv = min(max(int(n_valid), 0), N)
    hann = window()
    x = np.zeros(N + W + H, dtype=np.float32)
    x[:nv] = wav[:nv]
    out = np.zeros(Nout, dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(len(pos)):
            m0, m1 = k * H, min(k * H + H, n_out)
            r = np.arange(m1 - m0)
            cur = x[pos[k] + r]
            if k == 0 or pos[k] == pos[k - 1] + H:
                out[m0:m1] = cur
                continue
            prev = x[pos[k - 1] + H + r]
            s = (hann[r] * cur).astype(np.float32) + (hann[r + H] * prev).astype(np.float32)
            s = s.astype(np.float32)
            s.view(np.uint32)[np.isnan(s)] = CANON_NAN
            out[m0:m1] = s
    return out


def wsola(wav, n_valid, tempo_q, Nout):
    """one row: (out fp32 [Nout], q int16 [N], pos list, K, n_out)"""
    q = quant(wav, n_valid)
    pos, n_out = positions(q, n_valid, tempo_q, Nout)
    return ola(wav, pos, n_valid, n_out, Nout), q, pos, len(pos), n_out


def jumps(pos):
    return sum(1 for k in range(1, len(pos)) if pos[k] != pos[k - 1] + H)


# ---- the kernel test's cases: name -> (wav fp32 [B, N], n_valid [B], tempo_q [B], Nout) ----
def q_of(tempo):
    return int(round(tempo * ONE))


def _voice(f, n, seed, noise=0.02):
    import torch
    from tests import pitch_ref as P
    return P.harmonic_row(f, n, torch.Generator().manual_seed(seed), noise).float().numpy()


def batch_case():
    """psola_ref.gpu_case's rows: a 110 Hz voice in noise at 0.8, a 200 -> 260 Hz glide at 1.25, noise at 0.5, a voiced
    row of 700 valid samples at 2.0, a row of none under tempo_q 0"""
    from tests import psola_ref
    wav, _, _, nv = psola_ref.gpu_case()
    return wav.numpy().copy(), [int(v) for v in nv], [q_of(0.8), q_of(1.25), q_of(0.5), q_of(2.0), 0], 8000


def edge_case(N=2400):
    """constant, all-zero, +-0 only, denormals only, NaNs and infinities of both signs in a voice, and a voice whose
    peak is its last valid sample"""
    rng = np.random.default_rng(29)
    rows = np.zeros((6, N), dtype=np.float32)
    rows[0] = 0.25
    rows[2] = np.where(rng.random(N) < 0.5, np.float32(-0.0), np.float32(0.0))
    rows[3] = (rng.integers(-400, 400, N) * np.float64(2.0 ** -149)).astype(np.float32)
    rows[4] = _voice(140.0, N, 291)
    rows[4, 100:2300:170] = np.nan
    rows[4, 150:2300:310] = np.inf
    rows[4, 175:2300:290] = -np.inf
    rows[4].view(np.uint32)[7] = 0xFFC00001                                  # (a NaN with a sign and a payload)
    rows[5] = _voice(180.0, N, 292)
    rows[5, 1999] = -3.0
    return rows, [N, N, N, N, N, 2000], [q_of(0.8), q_of(1.25), q_of(0.7), q_of(1.6), q_of(0.9), q_of(1.1)], 2 * N


def kernel_cases():
    rng = np.random.default_rng(2929)
    long_rows = np.stack([_voice(120.0, 20001, 293, 0.05), _voice(210.0, 20001, 294, 0.05),
                          0.1 * rng.standard_normal(20001).astype(np.float32)])
    return {
        "batch": batch_case(),
        "empty_fast": (np.ones((1, 4000), dtype=np.float32), [0], [1 << 20], 8000),
        "short": (_voice(300.0, 159, 295)[None], [159], [q_of(1.25)], 159),                   # K = 1
        # n_out a multiple of the hop, and that plus 1, at tempo 1 and at 0.8
        "multiple": (np.stack([_voice(150.0, 2000, 296 + i) for i in range(4)]), [1600, 1601, 1280, 1281],
                     [ONE, ONE, q_of(0.8), q_of(0.8)], 1700),
        "tiny": (np.stack([_voice(200.0, 400, 300 + i) for i in range(4)]), [200, 319, 1, 2],
                 [q_of(0.5), q_of(2.0), q_of(0.5), ONE], 700),                                 # n_valid < W
        "cap": (_voice(110.0, 4000, 304)[None], [4000], [q_of(0.5)], 3001),                    # Nout < n_out
        "low": (np.stack([_voice(62.0, 4000, 305), _voice(62.0, 4000, 306)]), [4000, 3777],
                [q_of(0.8), q_of(1.25)], 5000),                                                # period 258 > D
        "edge": edge_case(),
        # rows that start at every alignment, and widths that are no multiple of 4 or 8
        "odd": (np.stack([_voice(100.0 + 30 * i, 2999, 307 + i) for i in range(5)]), [2999, 2998, 2001, 2999, 1555],
                [q_of(0.8), q_of(1.25), q_of(0.6), ONE + 1, ONE - 1], 4003),
        # more than one staged chunk of the search and more than one partial maximum: tempo 0.5, 2 and 1.3
        "long": (long_rows, [20001, 19999, 20001], [q_of(0.5), q_of(2.0), q_of(1.3)], 40002),
    }


def reference(case):
    """per row (out, q, pos, K, n_out) of a case"""
    wav, nv, tq, Nout = case
    return [wsola(wav[b], nv[b], tq[b], Nout) for b in range(wav.shape[0])]


# ---- the rows whose F0 must stay (DESIGN section 16's resonance rows and harmonic rows at 95 to 300 Hz) ----
F0_HARMONIC = (95.0, 140.0, 210.0, 300.0)
F0_TEMPOS = (0.8, 1.25)


def f0_rows():
    """(wav fp32 torch [7, 8000], the fundamentals the rows were generated at)"""
    import torch
    from tests import formant_ref as F
    from tests import pitch_ref as P
    g = torch.Generator().manual_seed(2930)
    rows = [F.resonance_rows()] + [P.harmonic_row(f, F.ROW_SAMPLES, g)[None].float() for f in F0_HARMONIC]
    return torch.cat(rows), [f for f, _ in F.ROWS] + list(F0_HARMONIC)


def scaled(wav, tempo):
    """the restatement on every row of wav (torch [B, N]) at one tempo -> (out torch fp32 [B, n_out], n_out)"""
    import torch
    w = wav.numpy()
    n_out = out_len(w.shape[1], q_of(tempo))
    return torch.from_numpy(np.stack([wsola(row, w.shape[1], q_of(tempo), n_out)[0] for row in w])), n_out


def voiced_mean(wav):
    """the mean voiced F0 of every row by the tracker restatement (tests/pitch_ref.py), all frames counting"""
    import torch
    from tests import pitch_ref as P
    wav = torch.as_tensor(wav)
    return P.voiced_mean(P.yin(wav.double())[0], torch.ones(wav.shape[0]), wav.shape[1])[0]
