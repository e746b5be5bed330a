"""fp64 restatement of the mel-cepstral distortion scorer (include/sa_hip.h), written from the
definition, with numpy only.  mel_ref [B, T_ref, n_mels], mel_deg [B, T_deg, n_mels] (the fp32 values, log-Mel power
in dB), n_ref, n_deg [B], order K, band R ->

  c_k(t) = (1 / n_mels) sum_m mel[t][m] cos(pi k (m + 1/2) / n_mels), k = 1..K       (a matrix product)
  d(i, j) = sqrt(1/2 sum_k (c_k^ref(i) - c_k^deg(j))^2)                               (the full N x M matrix)
  g(0, 0) = 2 d(0, 0);  g(i, j) = min(g(i-1, j-1) + 2 d(i, j), g(i-1, j) + d(i, j), g(i, j-1) + d(i, j)), row by row
      over the full matrix, inf where |i - j| > R
  mcd = g(N-1, M-1) / (N + M);  mcd_sync = (1 / min(N, M)) sum_{i < min(N, M)} d(i, i);  frames = N + M
  a row with N < 1, M < 1 or |N - M| > R: three zeros

``log_mel`` is the fp64 front end, written from the definitions of speech_anonymization_amd/features.py: frames of
400 samples every 160 around the sample 160 t (200 zeros before and after the row), the periodic Hamming window, the
power of the 201 bins, the 80 triangular filters on the HTK Mel scale (centre +- the left spacing), 10 log10 of the
power floored at 1e-10, and the floor at the row's largest value less 80 dB.

The keyword arguments of ``score`` and ``log_mel`` re-evaluate them with the perturbations tools/mcd_delta.py
measures.  The module also holds the GPU test's cases and its bars."""
import math
import types

import numpy as np

U = 2.0 ** -24
ORDER, BAND = 13, 16                      # the defaults of ops.mcd
MAX_ORDER, MAX_BAND = 32, 63
N_MELS, N_FFT, HOP, SR = 80, 400, 160, 16000
OUTPUTS = ("mcd", "mcd_sync")

# tools/mcd_delta.py: the worst |delta| between the restatement and its perturbed evaluations, per output, over
# gpu_cases() (four perturbations) and over wave_case() (the same four and the fp32 front end).  The GPU tests allow
# the kernel BAR_FACTOR x that plus 2^-24 |ref|.
DELTA_MEASURED = {"mcd": 7.9675e-7, "mcd_sync": 6.5334e-7}
DELTA_WAVE_MEASURED = {"mcd": 6.0508e-7, "mcd_sync": 2.1287e-7}
BAR_FACTOR = 16.0


# ---------------------------------------------------------------------------------------------------
# the scorer
# ---------------------------------------------------------------------------------------------------
def dct_matrix(n_mels, order, cos32=False):
    """[n_mels, K]: cos(pi k (m + 1/2) / n_mels), k = 1..K"""
    m = np.arange(n_mels, dtype=np.float64)[:, None]
    k = np.arange(1, order + 1, dtype=np.float64)[None, :]
    C = np.cos(np.pi * k * (m + 0.5) / n_mels)
    return C.astype(np.float32).astype(np.float64) if cos32 else C


def cepstra(mel, order, cos32=False, cep32=False):
    """mel [T, n_mels] -> c [T, K] fp64"""
    mel = np.asarray(mel, dtype=np.float64)
    c = mel @ dct_matrix(mel.shape[1], order, cos32) / mel.shape[1]
    return c.astype(np.float32).astype(np.float64) if cep32 else c


def distances(c_ref, c_deg, sum32=False, reverse=False):
    """c_ref [N, K], c_deg [M, K] -> d [N, M]: the sum over k term by term, from the far end if ``reverse``, in fp32
    if ``sum32``"""
    dt = np.float32 if sum32 else np.float64
    diff = (c_ref[:, None, :] - c_deg[None, :, :]).astype(dt)
    sq = diff * diff
    acc = np.zeros(sq.shape[:2], dtype=dt)
    for k in (range(sq.shape[2] - 1, -1, -1) if reverse else range(sq.shape[2])):
        acc = acc + sq[:, :, k]
    return np.sqrt(dt(0.5) * acc).astype(np.float64)


def dtw(d, band, sum32=False):
    """d [N, M] -> g(N-1, M-1), inf when that cell lies outside the band"""
    dt = np.float32 if sum32 else np.float64
    N, M = d.shape
    d = d.astype(dt)
    g = np.full((N, M), np.inf, dtype=dt)
    two = dt(2.0)
    for i in range(N):
        for j in range(max(0, i - band), min(M, i + band + 1)):     # the others stay inf
            if i == 0 and j == 0:
                g[0, 0] = two * d[0, 0]
                continue
            best = dt(np.inf)
            if i > 0 and j > 0:
                best = min(best, g[i - 1, j - 1] + two * d[i, j])
            if i > 0:
                best = min(best, g[i - 1, j] + d[i, j])
            if j > 0:
                best = min(best, g[i, j - 1] + d[i, j])
            g[i, j] = best
    return float(g[N - 1, M - 1])


def score(mel_ref, mel_deg, n_ref, n_deg, order=ORDER, band=BAND, cep32=False, cos32=False, sum32=False,
          reverse=False):
    """-> a namespace: mcd, mcd_sync fp64 [B], frames int32 [B]"""
    mel_ref, mel_deg = np.asarray(mel_ref, dtype=np.float64), np.asarray(mel_deg, dtype=np.float64)
    B = mel_ref.shape[0]
    out = types.SimpleNamespace(mcd=np.zeros(B), mcd_sync=np.zeros(B), frames=np.zeros(B, np.int32))
    for b in range(B):
        N = min(max(int(n_ref[b]), 0), mel_ref.shape[1])
        M = min(max(int(n_deg[b]), 0), mel_deg.shape[1])
        if N < 1 or M < 1 or abs(N - M) > band:
            continue
        d = distances(cepstra(mel_ref[b, :N], order, cos32, cep32), cepstra(mel_deg[b, :M], order, cos32, cep32),
                      sum32, reverse)
        L = min(N, M)
        diag = d[np.arange(L), np.arange(L)]
        if sum32:
            diag = diag.astype(np.float32)
        out.mcd[b] = dtw(d, band, sum32) / (N + M)
        out.mcd_sync[b] = float(diag.sum(dtype=diag.dtype)) / L
        out.frames[b] = N + M
    return out


PERTURBATIONS = {"cep32": dict(cep32=True), "cos32": dict(cos32=True), "sum32": dict(sum32=True),
                 "reverse": dict(reverse=True)}


# ---------------------------------------------------------------------------------------------------
# the front end
# ---------------------------------------------------------------------------------------------------
def mel_matrix(dt=np.float64):
    """[201, 80]: the triangular filters of features._mel_matrix, every step in ``dt``"""
    to_mel = lambda hz: 2595.0 * math.log10(1.0 + hz / 700.0)
    mel = np.linspace(to_mel(0.0), to_mel(SR / 2), N_MELS + 2).astype(dt)
    hz = (dt(700.0) * (dt(10.0) ** (mel / dt(2595.0)) - dt(1.0))).astype(dt)
    band = (hz[1:] - hz[:-1])[:-1]
    centre = hz[1:-1]
    freqs = np.linspace(0, SR // 2, N_FFT // 2 + 1).astype(dt)
    slope = (freqs[:, None] - centre[None, :]) / band[None, :]
    return np.maximum(dt(0.0), np.minimum(slope + dt(1.0), -slope + dt(1.0))).astype(dt)


def _product(a, b, in_order):
    """a [..., n] @ b [n, m]; in_order: term by term in the order of n in a's own precision, so that the fp32 variant
    gives the same bits on every machine (the fp64 path's library product moves it by 1e-16 relative at most)"""
    if not in_order:
        return a @ b
    acc = np.zeros(a.shape[:-1] + (b.shape[1],), dtype=a.dtype)
    for n in range(b.shape[0]):
        acc = acc + a[..., n, None] * b[n]
    return acc


def log_mel(wav, fp32=False):
    """wav [B, N] (the fp32 values) -> [B, N // 160 + 1, 80] fp64: the clamped log-Mel power in dB; fp32: the window,
    the transform (as products with the cosine and sine tables), the power, the filters and the logarithm in fp32"""
    dt = np.float32 if fp32 else np.float64
    wav = np.asarray(wav, dtype=np.float32).astype(dt)
    B, N = wav.shape
    T = N // HOP + 1
    wp = np.pad(wav, ((0, 0), (N_FFT // 2, N_FFT // 2)))
    n = np.arange(N_FFT, dtype=np.float64)
    win = (0.54 - 0.46 * np.cos(2.0 * np.pi * n / N_FFT)).astype(dt)
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    fr = wp[:, idx] * win                                                    # [B, T, 400]
    ang = 2.0 * np.pi * ((np.arange(N_FFT // 2 + 1)[None, :] * np.arange(N_FFT)[:, None]) % N_FFT) / N_FFT
    re, im = _product(fr, np.cos(ang).astype(dt), fp32), _product(fr, np.sin(ang).astype(dt), fp32)    # [B, T, 201]
    power = re * re + im * im
    fb = _product(power, mel_matrix(dt), fp32)
    db = dt(10.0) * np.log10(np.maximum(fb, dt(1e-10)))
    floor = db.reshape(B, -1).max(axis=1) - dt(80.0)
    out = np.maximum(db, floor[:, None, None])
    assert out.dtype == dt
    return out.astype(np.float64)


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 63, 64, 65, 130)
BANDS = (0, 1, 7, 16, 63)
ORDERS = (1, 13, 32)
ROWS_PER_BATCH = 4


def mel_field(T, seed):
    """a log-Mel-like field [T, 80] fp64 in dB: a tilted envelope with two moving ridges and per-bin noise"""
    g = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)[:, None]
    m = np.arange(N_MELS, dtype=np.float64)[None, :]
    c1 = 14.0 + 6.0 * np.sin(2.0 * np.pi * t / 23.0 + g.uniform(0, 6.28))
    c2 = 42.0 + 11.0 * np.sin(2.0 * np.pi * t / 37.0 + g.uniform(0, 6.28))
    env = -0.35 * m + 18.0 * np.exp(-0.5 * ((m - c1) / 4.0) ** 2) + 12.0 * np.exp(-0.5 * ((m - c2) / 6.0) ** 2)
    level = 6.0 * np.sin(2.0 * np.pi * t / 51.0 + g.uniform(0, 6.28))
    return env + level + 2.0 * g.standard_normal((T, N_MELS))


def warped(ref, M, seed):
    """deg [M, 80]: ref read at a wandering position, its ridges flattened, with noise of its own"""
    g = np.random.default_rng(seed)
    N = ref.shape[0]
    pos = np.arange(M, dtype=np.float64) * (N / M) + 1.5 * np.sin(2.0 * np.pi * np.arange(M) / 29.0)
    src = np.clip(np.rint(pos).astype(np.int64), 0, N - 1)
    m = np.arange(N_MELS, dtype=np.float64)[None, :]
    return 0.8 * ref[src] + 0.1 * m + 1.0 * g.standard_normal((M, N_MELS))


def case_rows(band, order):
    """the (N, M) of a (band, order) setting: N - M through -R, -1, 0, 1, R, then R + 1 (unscored) and two more rows
    of equal counts; one of the two counts walks through LENGTHS, from a start that depends on the setting, the other
    follows from the difference"""
    start = BANDS.index(band) * len(ORDERS) + ORDERS.index(order)
    rows = []
    for q, delta in enumerate((-band, -1, 0, 1, band, band + 1, 0, 0)):
        n = LENGTHS[(start + q) % len(LENGTHS)]
        rows.append((n, n - delta) if n - delta >= 1 else (n + delta, n))
    return rows


_CASES = None


def gpu_cases():
    """the cases of the kernel test: [(name, mel_ref fp32 [4, T_ref, 80], mel_deg fp32 [4, T_deg, 80], n_ref int32 [4],
    n_deg int32 [4], order, band)], two batches per (band, order), built once and shared: treat them as read-only.
    T_ref and T_deg are the batch's largest counts plus 2; the frames at or beyond a row's count hold NaN."""
    global _CASES
    if _CASES is not None:
        return _CASES
    cases, seed = [], 2300
    for band in BANDS:
        for order in ORDERS:
            rows = case_rows(band, order)
            for h in range(0, len(rows), ROWS_PER_BATCH):
                part = rows[h:h + ROWS_PER_BATCH]
                T_ref, T_deg = max(r[0] for r in part) + 2, max(r[1] for r in part) + 2
                ref = np.full((len(part), T_ref, N_MELS), np.nan, dtype=np.float32)
                deg = np.full((len(part), T_deg, N_MELS), np.nan, dtype=np.float32)
                for b, (N, M) in enumerate(part):
                    seed += 2
                    f = mel_field(N, seed)
                    ref[b, :N], deg[b, :M] = f, warped(f, M, seed + 1)
                cases.append((f"R{band}_K{order}_{h // ROWS_PER_BATCH}", ref, deg,
                              np.array([r[0] for r in part], np.int32), np.array([r[1] for r in part], np.int32),
                              order, band))
    _CASES = cases
    return cases


_REF_CACHE = {}


def case_ref(name):
    """the restatement of a case, computed once and shared: treat it as read-only"""
    if name not in _REF_CACHE:
        _, ref, deg, n_ref, n_deg, order, band = next(c for c in gpu_cases() if c[0] == name)
        _REF_CACHE[name] = score(ref, deg, n_ref, n_deg, order, band)
    return _REF_CACHE[name]


def delayed(ref, s):
    """(ref', deg) [T, 80] of the exact-alignment property: the last s + 1 frames of ref' equal, deg = ref' delayed by
    s frames with the first frame repeated"""
    ref = np.array(ref, dtype=np.float32)
    T = ref.shape[0]
    ref[T - s - 1:] = ref[T - s - 1]
    return ref, ref[np.maximum(np.arange(T) - s, 0)]


TILT_POLE, DELAY_FRAMES = 0.5, 3
_WAVE = None


def wave_case():
    """-> (wav_ref fp32 [2, 24000], wav_deg fp32 [2, 24000], n_valid int32 [2]): the glide and the vibrato row of
    tests/contour_ref.py, and a copy made on the CPU in fp64: a spectral tilt by the one-pole filter
    y[n] = x[n] + 0.5 y[n-1], scaled by 1/2, delayed by 3 frames; the second row counts up to 20000 samples"""
    global _WAVE
    if _WAVE is None:
        from tests import contour_ref as Cr
        ref = Cr.case_rows().numpy().astype(np.float32)
        x = ref.astype(np.float64)
        y = np.zeros_like(x)
        acc = np.zeros(x.shape[0])
        for n in range(x.shape[1]):
            acc = x[:, n] + TILT_POLE * acc
            y[:, n] = acc
        deg = np.zeros_like(x)
        deg[:, DELAY_FRAMES * HOP:] = 0.5 * y[:, :x.shape[1] - DELAY_FRAMES * HOP]
        _WAVE = ref, deg.astype(np.float32), np.array([x.shape[1], 20000], np.int32)
    return _WAVE


def wave_counts(n_valid, width):
    """the frames that count, as metrics.mel_cepstral_distortion takes them"""
    return np.minimum(np.asarray(n_valid) // HOP + 1, width // HOP + 1).astype(np.int32)


_WAVE_REF = {}


def wave_ref(fp32=False, **kw):
    """the restatement of wave_case() through log_mel, order 13, band 16 (the plain one computed once and shared)"""
    key = (fp32, tuple(sorted(kw.items())))
    if key not in _WAVE_REF:
        ref, deg, nv = wave_case()
        fr = wave_counts(nv, ref.shape[1])
        mel = _WAVE_REF.get(("mel", fp32))
        if mel is None:
            mel = _WAVE_REF["mel", fp32] = tuple(log_mel(w, fp32) for w in (ref, deg))
        _WAVE_REF[key] = score(mel[0], mel[1], fr, fr, ORDER, BAND, **kw)
    return _WAVE_REF[key]


def bar(output, ref_value, wave=False):
    """the GPU tests' allowance: 16 x the measured spread of the restatement plus the output's fp32 rounding"""
    return BAR_FACTOR * (DELTA_WAVE_MEASURED if wave else DELTA_MEASURED)[output] + U * abs(ref_value)
