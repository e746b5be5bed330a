"""fp64 restatement of the STOI / ESTOI scorer (include/sa_hip.h, csrc/sa_stoi.hip), written from
the formulas, with numpy only.  ref, deg [B, N] (the fp32 values, 16 kHz), n_valid [B] ->

  (1) x10[m] = sum_n x[n] h[8 m - 5 n], |8 m - 5 n| <= 80, m < n10 = (5 n_valid + 7) // 8;  a sample at or beyond
      n_valid reads as 0;  h[k] = (5/8) sinc(k/8) I0(5 sqrt(1 - (k/80)^2)) / I0(5)
  (2) w[j] = 0.5 - 0.5 cos(2 pi (j + 1) / 257);  frames of 256 at hop 128;  e_t = sum_j (w[j] x10[128 t + j])^2 on
      ref;  kept: e_t > 1e-4 max_t e_t
  (3) xs = the overlap-add of the kept windowed frames, the same frames of both signals
  (4) P = |DFT_512(w . frame_m(xs))|^2;  X[j][m] = sqrt(sum_{lo_j <= k < hi_j} P[m][k])
  (5) segments of 30 frames;  STOI: the clipped, normalised correlation per band;  ESTOI: rows, then columns, made
      zero-mean and unit-norm, (1/30) sum of the product

The keyword arguments of ``stoi`` re-evaluate it with the four perturbations tools/stoi_delta.py measures."""
import math
import types

import numpy as np

SR, SR10 = 16000, 10000
UP, DOWN = 5, 8
HALF = 80                                 # taps on either side: 161 in all
BETA_KAISER = 5.0
W, H, NFFT = 256, 128, 512
NBANDS, SEG = 15, 30
RANGE = 1e-4                              # 40 dB, in the power domain
CLIP = 1.0 + 10.0 ** 0.75                 # 1 + 10^(-beta / 20), beta = -15 dB
EPS = 2.0 ** -52
U = 2.0 ** -24
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
         (87, 109), (109, 138), (138, 174), (174, 219))
MARGIN = 1e-6                             # no frame energy of a test row within 1 +- this of its threshold

# tools/stoi_delta.py on gpu_cases(): the worst |delta score| between the restatement and its four perturbed
# evaluations, per measure; the GPU test allows the kernel BAR_FACTOR x that plus 2^-24 |ref|
DELTA_MEASURED = {"stoi": 1.2801e-8, "estoi": 9.0293e-8}
BAR_FACTOR = 16.0


def band_table():
    """the 15 (lo, hi) pairs from the rule: centres 150 2^(j/3) Hz, edges at -+1/6 octave, each rounded to the
    nearest of the 257 bins of a 512-point transform at 10 kHz"""
    f = np.linspace(0.0, SR10, NFFT + 1)[:NFFT // 2 + 1]
    out = []
    for j in range(NBANDS):
        c = 150.0 * 2.0 ** (j / 3.0)
        lo, hi = c * 2.0 ** (-1.0 / 6.0), c * 2.0 ** (1.0 / 6.0)
        out.append((int(np.argmin((f - lo) ** 2)), int(np.argmin((f - hi) ** 2))))
    return tuple(out)


def taps():
    """h[k + 80], k = -80..80"""
    k = np.arange(-HALF, HALF + 1, dtype=np.float64)
    return (UP / DOWN) * np.sinc(k / DOWN) * np.i0(BETA_KAISER * np.sqrt(1.0 - (k / HALF) ** 2)) / np.i0(BETA_KAISER)


TAPS = taps()
WINDOW = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(W) + 1.0) / (W + 1.0))


def n10_of(n_valid):
    return (UP * int(n_valid) + DOWN - 1) // DOWN


def frames_of(n10):
    return (n10 - W) // H + 1 if n10 >= W else 0


def resample(x, n_valid):
    """x [N] fp64, zero from n_valid on -> x10 [n10]; every output sums its at most 33 taps in ascending n"""
    n_valid = min(max(int(n_valid), 0), x.shape[0])
    n10 = n10_of(n_valid)
    m = np.arange(n10)
    n_lo = -((HALF - DOWN * m) // UP)                       # ceil((8 m - 80) / 5)
    out = np.zeros(n10)
    for i in range(2 * HALF // UP + 1):
        n = n_lo + i
        k = DOWN * m - UP * n
        ok = (np.abs(k) <= HALF) & (n >= 0) & (n < n_valid)
        out += np.where(ok, x[np.clip(n, 0, x.shape[0] - 1)] * TAPS[np.clip(k, -HALF, HALF) + HALF], 0.0)
    return out


def frame_energies(x10, reverse=False):
    F = frames_of(x10.shape[0])
    if F == 0:
        return np.zeros(0)
    fr = np.stack([x10[H * t:H * t + W] for t in range(F)]) * WINDOW
    if not reverse:
        return (fr * fr).sum(1)
    e = np.zeros(F)
    for j in range(W - 1, -1, -1):
        e += fr[:, j] * fr[:, j]
    return e


def compact(x10, kept):
    """the overlap-add of the kept windowed frames: [128 (K + 1)]"""
    xs = np.zeros(H * (len(kept) + 1))
    for i, t in enumerate(kept):
        xs[H * i:H * i + W] += WINDOW * x10[H * t:H * t + W]
    return xs


def band_magnitudes(xs, K, direct=False):
    """-> X [15, K]"""
    if K == 0:
        return np.zeros((NBANDS, 0))
    fr = np.stack([xs[H * m:H * m + W] for m in range(K)]) * WINDOW
    if direct:                                              # a direct sum, n from the far end
        kk = np.arange(BANDS[0][0], BANDS[-1][1])
        acc = np.zeros((K, kk.shape[0]), dtype=np.complex128)
        for n in range(W - 1, -1, -1):
            acc += fr[:, n, None] * np.exp(-2j * np.pi * ((kk * n) % NFFT) / NFFT)[None, :]
        P = np.zeros((K, NFFT // 2 + 1))
        P[:, kk] = acc.real ** 2 + acc.imag ** 2
    else:
        spec = np.fft.rfft(fr, NFFT, axis=1)
        P = spec.real ** 2 + spec.imag ** 2
    return np.stack([np.sqrt(P[:, lo:hi].sum(1)) for lo, hi in BANDS])


def _unit(v, axis):
    v = v - v.mean(axis, keepdims=True)
    return v / (np.sqrt((v * v).sum(axis, keepdims=True)) + EPS)


def segment_scores(X, Y):
    """X, Y [15, K] -> (STOI summed over bands [S], ESTOI d_m [S])"""
    K = X.shape[1]
    S = K - SEG + 1 if K >= SEG else 0
    st, es = np.zeros(S), np.zeros(S)
    for s in range(S):
        x, y = X[:, s:s + SEG], Y[:, s:s + SEG]
        alpha = np.sqrt((x * x).sum(1, keepdims=True)) / (np.sqrt((y * y).sum(1, keepdims=True)) + EPS)
        yc = np.minimum(alpha * y, CLIP * x)
        st[s] = (_unit(x, 1) * _unit(yc, 1)).sum()
        es[s] = (_unit(_unit(x, 1), 0) * _unit(_unit(y, 1), 0)).sum() / SEG
    return st, es


def f32(v):
    return v.astype(np.float32).astype(np.float64)


def stoi(ref, deg, n_valid, x10_fp32=False, bands_fp32=False, direct_dft=False, reverse_energy=False):
    """-> a namespace: stoi, estoi fp64 [B], frames, segments int [B], energies (a list of [F_b]), margin [B] (the
    smallest |e_t / threshold - 1| of the row; inf where the threshold is 0 or there is no frame)"""
    ref, deg = np.asarray(ref, dtype=np.float64), np.asarray(deg, dtype=np.float64)
    B, N = ref.shape
    out = types.SimpleNamespace(stoi=np.zeros(B), estoi=np.zeros(B), frames=np.zeros(B, np.int32),
                                segments=np.zeros(B, np.int32), energies=[], margin=np.full(B, np.inf))
    for b in range(B):
        nv = min(max(int(n_valid[b]), 0), N)
        x10, y10 = resample(ref[b], nv), resample(deg[b], nv)
        if x10_fp32:
            x10, y10 = f32(x10), f32(y10)
        e = frame_energies(x10, reverse_energy)
        out.energies.append(e)
        thr = RANGE * e.max() if e.size else 0.0
        kept = np.nonzero(e > thr)[0]
        if thr > 0.0:
            out.margin[b] = float(np.abs(e / thr - 1.0).min())
        K = len(kept)
        X = band_magnitudes(compact(x10, kept), K, direct_dft)
        Y = band_magnitudes(compact(y10, kept), K, direct_dft)
        if bands_fp32:
            X, Y = f32(X), f32(Y)
        st, es = segment_scores(X, Y)
        S = st.shape[0]
        out.frames[b], out.segments[b] = K, S
        if S:
            out.stoi[b], out.estoi[b] = st.sum() / (NBANDS * S), es.sum() / S
    return out


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def harmonic_row(n, seed=0, f0=120.0, amp=0.1):
    """a modulated harmonic row: f0 with 1/h harmonics below 4.9 kHz under a 4 Hz envelope, fp64 [n]"""
    t = np.arange(n) / SR
    s = np.zeros(n)
    ph = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, 64)
    for h in range(1, int(4900.0 / f0) + 1):
        s += np.sin(2.0 * np.pi * f0 * h * t + ph[h]) / h
    return amp * (0.55 + 0.45 * np.sin(2.0 * np.pi * 4.0 * t)) * s


def white(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def at_snr(x, noise, snr_db):
    """x + noise scaled to the given signal-to-noise ratio over the whole row"""
    g = math.sqrt((x * x).sum() / (noise * noise).sum() * 10.0 ** (-snr_db / 10.0))
    return x + g * noise


def _synthetic_mcadams():
    """the first row of data.synthetic_gender_dataset and its McAdams(0.8) transform by tests/mcadams_ref.py"""
    from speech_anonymization_amd import data
    from tests import mcadams_ref as M
    wav = next(iter(data.synthetic_gender_dataset(1, 1, seed=1986))).sig[0].numpy()
    out = M.mcadams(wav, np.array([0.8], np.float32), np.array([wav.shape[1]], np.int32), True).out
    return wav, out.astype(np.float32)


_CASES = None


def gpu_cases():
    """the cases of the kernel test: [(name, ref fp32 [B, N], deg fp32 [B, N], n_valid int32 [B], the kept-frame
    counts each row is meant to have)], built once and shared: treat them as read-only.

      rows      (3, 8000): a modulated harmonic with noise (38 frames, all kept); the same with samples 3200..4800
                zeroed (six frames wholly inside the gap drop out: compaction joins frames 15 and 22); a short row
                (n_valid 6400: 30 frames, one segment).  deg = ref + white noise at 10, 0 and 20 dB.
      one       (1, 6348): n10 = 3968, F = K = 30, exactly one segment
      none      (1, 6346): K = 29, no segment
      empty     (2, 8000), n_valid (0, 8000)
      zero_deg  (2, 8000), deg all zero
      mcadams   (1, 16000): a synthetic_gender_dataset row against its own McAdams(0.8) output"""
    global _CASES
    if _CASES is not None:
        return _CASES
    N = 8000
    base = at_snr(harmonic_row(N, 1), white(N, 2), 30.0)
    gap = base.copy()
    gap[3200:4800] = 0.0
    short = at_snr(harmonic_row(N, 3, f0=150.0), white(N, 4), 30.0)
    ref = np.stack([base, gap, short]).astype(np.float32)
    deg = np.stack([at_snr(ref[0].astype(np.float64), white(N, 5), 10.0),
                    at_snr(ref[1].astype(np.float64), white(N, 6), 0.0),
                    at_snr(ref[2].astype(np.float64), white(N, 7), 20.0)]).astype(np.float32)
    cases = [("rows", ref, deg, np.array([8000, 8000, 6400], np.int32), (38, 32, 30))]
    for name, n, K in (("one", 6348, 30), ("none", 6346, 29)):
        r = at_snr(harmonic_row(n, 8), white(n, 9), 30.0)
        cases.append((name, r[None].astype(np.float32), at_snr(r, white(n, 10), 5.0)[None].astype(np.float32),
                      np.array([n], np.int32), (K,)))
    two = np.stack([base, short]).astype(np.float32)
    two_deg = np.stack([at_snr(base, white(N, 11), 10.0), at_snr(short, white(N, 12), 10.0)]).astype(np.float32)
    cases.append(("empty", two, two_deg, np.array([0, 8000], np.int32), (0, 38)))
    cases.append(("zero_deg", two, np.zeros_like(two), np.array([8000, 8000], np.int32), (38, 38)))
    wav, mc = _synthetic_mcadams()
    cases.append(("mcadams", wav, mc, np.array([wav.shape[1]], np.int32), (77,)))
    _CASES = cases
    return cases


_REF_CACHE = {}


def case_ref(name):
    """the restatement of a case, computed once and shared: treat it as read-only"""
    if name not in _REF_CACHE:
        _, ref, deg, nv, _ = next(c for c in gpu_cases() if c[0] == name)
        _REF_CACHE[name] = stoi(ref, deg, nv)
    return _REF_CACHE[name]


def bar(measure, ref_value):
    """the GPU test's allowance: 16 x the measured spread of the restatement plus the output's fp32 rounding"""
    return BAR_FACTOR * DELTA_MEASURED[measure] + U * abs(ref_value)
