"""fp64 restatement of the McAdams-coefficient transform (speech_anonymization_amd.mcadams and
csrc/sa_mcadams.hip), on the CPU with numpy: sqrt-Hann frames of 320 at hop 160, autocorrelation LPC of order 20,
the poles by ``numpy.roots`` (NOT by the kernel's Aberth iteration: the check is independent of the method under
test), every complex pole's angle raised to the power alpha, the frame re-synthesised from its own residual,
overlap-add, RMS level matching.  Shared by tests/test_mcadams_cpu.py, tests/test_mcadams_gpu.py and
tools/mcadams_delta.py, which swaps ``roots=`` and ``reverse_acf=`` to measure how far two equally valid fp64
evaluations lie apart (the constant C of the GPU test's bar)."""
import math
import types

import numpy as np

W, H, P = 320, 160, 20
SR = 16000
U = 2.0 ** -24
SILENCE = 1e-10
R0_LIFT = 1e-9
REAL_REL = 1e-6
ALPHA_LOW, ALPHA_HIGH = 0.25, 2.0
ABERTH_TOL, ABERTH_MAX = 1e-14, 64
OK, SILENT, FALLBACK = 0, 1, 2
# "near a decision": the frames a comparison leaves out
NEAR_IM = (1e-9, 1e-3)
NEAR_K = 1e-9
NEAR_R0 = 1e-6

# tools/mcadams_delta.py: the restatement with its own Aberth iteration / with the autocorrelation summed from the
# far end, against itself with numpy.roots: the worst |delta| / max|y| over gpu_cases().  The GPU test allows the
# kernel C_FACTOR times that on top of the fp32 roundings.
C_MEASURED = 1.43e-10
C_FACTOR = 16.0

WINDOW = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W))


def n_frames(N):
    return (int(N) + H - 1) // H + 1


def sanitize_alpha(alpha):
    """the fp32 coefficients as the kernel reads them, in fp64: the nearer bound outside [0.25, 2], 1 for a NaN"""
    a = np.asarray(alpha, dtype=np.float32).astype(np.float64)
    return np.where(np.isnan(a), 1.0, np.clip(a, ALPHA_LOW, ALPHA_HIGH))


def frames_of(x, n_valid):
    """x [N] -> the windowed frames [T, 320]: frame t covers [160 t - 160, 160 t + 160), zero outside [0, n_valid)"""
    N = x.shape[0]
    T = n_frames(N)
    xv = np.where(np.arange(N) < n_valid, x, 0.0)
    pad = np.zeros(H * (T + 1))
    pad[H:H + N] = xv
    idx = H * np.arange(T)[:, None] + np.arange(W)[None, :]
    return pad[idx] * WINDOW[None, :]


def autocorr(f, reverse=False):
    """r_k = sum_j f[j] f[j + k], k = 0..20, summed in index order (``reverse``: from the far end)"""
    r = np.zeros(P + 1)
    for k in range(P + 1):
        prod = f[:W - k] * f[k:]
        if reverse:
            prod = prod[::-1]
        s = 0.0
        for v in prod:
            s += v
        r[k] = s
    return r


def levinson(r):
    """-> (a [21] with a_0 = 1, the reflection coefficients [20], ok)"""
    a = np.zeros(P + 1)
    a[0] = 1.0
    ks = np.zeros(P)
    err = r[0]
    for m in range(1, P + 1):
        acc = r[m]
        for i in range(1, m):
            acc += a[i] * r[m - i]
        k = -acc / err
        ks[m - 1] = k
        if not abs(k) < 1.0:
            return a, ks, False
        prev = a.copy()
        for i in range(1, m):
            a[i] = prev[i] + k * prev[m - i]
        a[m] = k
        err *= 1.0 - k * k
        if not err > 0.0:
            return a, ks, False
    return a, ks, True


def aberth(a):
    """the kernel's root finder in fp64: -> (roots [20], iterations, converged)"""
    z = 0.9 * np.exp(2j * np.pi * (np.arange(P) + 0.25) / P)
    for it in range(1, ABERTH_MAX + 1):
        p = np.ones(P, dtype=complex)
        dp = np.zeros(P, dtype=complex)
        for k in range(1, P + 1):
            dp = dp * z + p
            p = p * z + a[k]
        ratio = p / dp
        diff = z[:, None] - z[None, :]
        np.fill_diagonal(diff, 1.0)
        inv = 1.0 / diff
        np.fill_diagonal(inv, 0.0)
        corr = ratio / (1.0 - ratio * inv.sum(1))
        z = z - corr
        if np.abs(corr).max() < ABERTH_TOL:
            return z, it, True
    return z, ABERTH_MAX, False


def numpy_roots(a):
    return np.roots(a), 0, True


def rebuild(z, alpha):
    """-> (a' [21], ok, the relative imaginary parts [20]): the reals kept, the upper half-plane's angles raised to
    the power alpha, the lower half-plane dropped"""
    mod = np.abs(z)
    rel = np.where(mod > 0, z.imag / np.where(mod > 0, mod, 1.0), 0.0)
    real = np.abs(rel) <= REAL_REL
    up = rel > REAL_REL
    if 2 * int(up.sum()) + int(real.sum()) != P:
        return None, False, rel
    poly = np.ones(1)
    for v in z[real].real:
        poly = np.convolve(poly, np.array([1.0, -v]))
    for v in z[up]:
        m = abs(v)
        phi = math.atan2(v.imag, v.real)
        poly = np.convolve(poly, np.array([1.0, -2.0 * m * math.cos(phi ** alpha), m * m]))
    return poly, True, rel


def filters(f, a, a2):
    """res = FIR(a) f, rec = IIR(1 / a2) res, zero history: f [320] -> rec [320]"""
    res = np.zeros(W)
    for k in range(P + 1):
        res[k:] += a[k] * f[:W - k]
    rec = np.zeros(W + P)
    for j in range(W):
        s = res[j]
        for k in range(1, P + 1):
            s -= a2[k] * rec[P + j - k]
        rec[P + j] = s
    return rec[P:]


def frame(f, alpha, roots=numpy_roots, reverse_acf=False):
    """one windowed frame -> (rec [320], status, near a decision?, root-finder iterations)"""
    r = autocorr(f, reverse_acf)
    near = abs(r[0] / SILENCE - 1.0) <= NEAR_R0
    if r[0] < SILENCE:
        return f.copy(), SILENT, near, 0
    r[0] *= 1.0 + R0_LIFT
    a, ks, ok = levinson(r)
    near = near or bool((np.abs(np.abs(ks) - 1.0) <= NEAR_K).any())
    if not ok:
        return f.copy(), FALLBACK, near, 0
    z, it, conv = roots(a)
    a2, ok, rel = rebuild(z, alpha)
    near = near or bool(((np.abs(rel) > NEAR_IM[0]) & (np.abs(rel) < NEAR_IM[1])).any())
    if not conv or not ok:
        return f.copy(), FALLBACK, near, it
    return filters(f, a, a2), OK, near, it


def mcadams(wav, alpha, n_valid, level=True, roots=numpy_roots, reverse_acf=False, copy_unity=True):
    """wav [B, N] (the fp32 values), alpha [B], n_valid [B] -> a namespace of fp64 arrays: F [B, T, 320] (the stored
    frames rec w, unrounded), y [B, N] (their overlap-add), gain [B], out [B, N], status [B, T], near [B, T] (frames
    near a decision), left_out [B, N] (samples such a frame touches), iters (largest root-finder count).
    ``copy_unity=False`` sends rows at alpha = 1 through the frames like any other (the window identity's test)."""
    x = np.asarray(wav, dtype=np.float32).astype(np.float64)
    B, N = x.shape
    T = n_frames(N)
    al = sanitize_alpha(alpha)
    nv = np.clip(np.asarray(n_valid, dtype=np.int64), 0, N)
    F = np.zeros((B, T, W))
    status = np.zeros((B, T), dtype=np.int32)
    near = np.zeros((B, T), dtype=bool)
    y = np.zeros((B, N))
    out = np.zeros((B, N))
    gain = np.ones(B)
    iters = 0
    for b in range(B):
        live = np.arange(N) < nv[b]
        if al[b] == 1.0 and copy_unity:
            y[b] = np.where(live, x[b], 0.0)
            out[b] = y[b]
            F[b] = frames_of(x[b], nv[b]) * WINDOW[None, :]
            continue
        fr = frames_of(x[b], nv[b])
        for t in range(T):
            rec, status[b, t], near[b, t], it = frame(fr[t], al[b], roots, reverse_acf)
            iters = max(iters, it)
            F[b, t] = rec * WINDOW
        n = np.arange(N)
        t0 = n // H
        y[b] = np.where(live, F[b, t0, n - H * t0 + H] + F[b, t0 + 1, n - H * t0], 0.0)
        if level:
            sx, sy = float(np.sum((x[b] * live) ** 2)), float(np.sum(y[b] ** 2))
            if sx > 0.0 and sy > 0.0:
                gain[b] = math.sqrt(sx / sy)
        out[b] = gain[b] * y[b]
    n = np.arange(N)
    t0 = n // H
    left_out = near[:, t0] | near[:, t0 + 1]
    live = n[None, :] < nv[:, None]
    rows = np.arange(B)[:, None]
    Fa = np.where(live, F[rows, t0[None, :], (n - H * t0 + H)[None, :]], 0.0)
    Fb = np.where(live, F[rows, t0[None, :] + 1, (n - H * t0)[None, :]], 0.0)
    return types.SimpleNamespace(x=x, alpha=al, n_valid=nv, F=F, Fa=Fa, Fb=Fb, y=y, gain=gain, out=out, status=status,
                                 near=near, left_out=left_out, iters=iters)


def gain_bar(ref, b, C):
    """the relative error of row b's gain, in units of u = 2^-24.  The kernel's y is the fp32 sum of two fp32-rounded
    frames: y^ = y + e with |e_n| <= u s_n + c, s = |F_a| + |F_b| + |F_a + F_b| and c = C max|y| (the fp64 evaluation's
    own spread).  Then |sum y^2 - sum y^2'| <= 2 sqrt(sum y^2) sqrt(sum (u s + c)^2) + sum (u s + c)^2 by
    Cauchy-Schwarz, g = sqrt(sum x^2 / sum y^2) takes half of that relative error to first order (the full second-order
    term is kept), the two fp64 sums of n terms add n 2^-53 each, and the square root and the division one more u
    in all when the gain is stored as fp32.  sum x^2 is exact up to its fp64 summation."""
    y = ref.y[b]
    sy = float(np.sum(y * y))
    if ref.gain[b] == 1.0 or sy == 0.0:
        return 1.0
    e = U * (np.abs(ref.Fa[b]) + np.abs(ref.Fb[b]) + np.abs(ref.Fa[b] + ref.Fb[b])) + C * np.abs(y).max()
    se = float(np.sum(e * e))
    rel = (2.0 * math.sqrt(sy * se) + se) / sy
    n = int(ref.n_valid[b])
    return (0.5 * rel + rel * rel + 2.0 * n * 2.0 ** -53) / U + 1.0


def envelope_peak_near(wav, expected_hz):
    """the local maximum of every row's mean cepstral envelope (tests/formant_ref.py's, 30 coefficients: peaks no
    closer than ~270 Hz) that lies nearest expected_hz [B], refined by the parabola through its neighbours: Hz [B]"""
    import torch
    from tests import formant_ref as FR
    from tests import pitch_ref as PR
    wav = torch.as_tensor(np.asarray(wav), dtype=torch.float64)
    B, N = wav.shape
    Np = PR.HOP * -(-N // PR.HOP)
    mag = PR.stft(torch.nn.functional.pad(wav, (0, Np - N))).abs().float()
    E = FR.envelope(mag).numpy()
    top = mag.double().amax(-1).numpy()
    out = []
    for b in range(B):
        m = E[b][top[b] > FR.SILENT_REL * top[b].max()].mean(0)
        k = np.arange(1, FR.K - 1)
        peaks = k[(m[k] >= m[k - 1]) & (m[k] > m[k + 1])]
        i = int(peaks[np.abs(40.0 * peaks - expected_hz[b]).argmin()])
        den = m[i - 1] - 2 * m[i] + m[i + 1]
        out.append(40.0 * (i + (0.5 * (m[i - 1] - m[i + 1]) / den if den < 0 else 0.0)))
    return np.array(out)


def expected_peak(F, alpha):
    """(16000 / 2 pi) phi^alpha of a resonance at F Hz"""
    return SR / (2.0 * math.pi) * (2.0 * math.pi * F / SR) ** alpha


# ---- the kernel test's inputs ---------------------------------------------------------------------------
def voiced_row(f0, formants, n, seed=0, amp=0.5):
    """a glottal pulse train at f0 through three two-pole resonances (centre, bandwidth in Hz), then white noise at
    0.02 of its peak (without a noise floor the order-20 normal equations are near singular and two fp64
    evaluations of the same frame lie 1e-8 apart), scaled to a peak of ``amp``: fp64 [n]"""
    rng = np.random.default_rng(4000 + seed)
    x = np.zeros(n)
    period = SR / f0
    k = 0
    while int(round(k * period)) < n:
        x[int(round(k * period))] = 1.0
        k += 1
    for fc, bw in formants:
        r = math.exp(-math.pi * bw / SR)
        c1, c2 = -2.0 * r * math.cos(2.0 * math.pi * fc / SR), r * r
        y = np.zeros(n + 2)
        for j in range(n):
            y[j + 2] = x[j] - c1 * y[j + 1] - c2 * y[j]
        x = y[2:]
    x = x / np.abs(x).max() + 0.02 * rng.standard_normal(n)
    return amp * x / np.abs(x).max()


FORMANTS = ((700.0, 130.0), (1220.0, 170.0), (2600.0, 250.0))


def gpu_cases():
    """the cases of the kernel test: [(name, wav fp32 [B, N], alpha fp32 [B], n_valid int32 [B])].  N = 1687 is no
    multiple of the hop; N = 50 has two frames; one row of the third case has no valid sample; the last is a row of
    data.synthetic_gender_dataset."""
    import torch
    from speech_anonymization_amd import data
    cases = []
    a = np.stack([voiced_row(120.0, FORMANTS, 1687, 0), voiced_row(210.0, FORMANTS, 1687, 1),
                  voiced_row(160.0, FORMANTS, 1687, 2)]).astype(np.float32)
    cases.append(("odd", a, np.array([0.8, 1.0, 0.5], np.float32), np.array([1687, 1687, 1000], np.int32)))
    cases.append(("two_frames", voiced_row(200.0, FORMANTS, 50, 3)[None].astype(np.float32),
                  np.array([0.8], np.float32), np.array([50], np.int32)))
    c = np.stack([voiced_row(140.0, FORMANTS, 1600, 4), voiced_row(180.0, FORMANTS, 1600, 5)]).astype(np.float32)
    cases.append(("empty_row", c, np.array([0.7, 0.9], np.float32), np.array([0, 1600], np.int32)))
    batch = next(iter(data.synthetic_gender_dataset(2, 2, seed=1986)))
    row = batch.sig[0][0, :4800].to(torch.float32).numpy().copy()
    cases.append(("synthetic", row[None], np.array([0.8], np.float32), np.array([4800], np.int32)))
    return cases


_REF_CACHE = {}


def case_ref(name, level):
    """the restatement of a case, computed once per (case, level) and shared: treat it as read-only"""
    key = (name, bool(level))
    if key not in _REF_CACHE:
        wav, alpha, nv = {c[0]: c[1:] for c in gpu_cases()}[name]
        _REF_CACHE[key] = mcadams(wav, alpha, nv, level)
    return _REF_CACHE[key]
