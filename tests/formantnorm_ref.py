"""fp64 restatement of the LPC formant normalisation (ops.pole_warp, ops.formant_centre and
csrc/sa_formant_norm.hip), on the CPU with numpy.  The pole warp shares its framing, autocorrelation, Levinson
recursion and filters with tests/mcadams_ref.py (the kernel shares them with sa_mcadams); the poles come from
``numpy.roots`` (NOT from the kernel's Aberth iteration) and the medians from a sort (NOT from the kernel's radix
select): the checks are independent of the methods under test.  Shared by tests/test_formant_norm_cpu.py,
tests/test_formant_norm_gpu.py and tools/formant_norm_delta.py, which swaps ``roots=`` and ``reverse_acf=`` to measure
how far equally valid fp64 evaluations lie apart (the constant C of the GPU test's bar)."""
import json
import math
import os
import types

import numpy as np

from tests import lpcformant_ref as LF
from tests import mcadams_ref as M

W, H, P, SR, U = M.W, M.H, M.P, M.SR, M.U
Q_LOW, Q_HIGH = 0.5, 2.0
KNEE = 0.85
OK, SILENT, FALLBACK = M.OK, M.SILENT, M.FALLBACK
NF = LF.NF
TARGET_DEFAULT = (550.0, 1650.0, 2750.0)
MIN_FRAMES = 8

# tools/formant_norm_delta.py (profiles/formant_norm_delta.json): the restatement with its own fp64 Aberth iteration
# and with the lag sums taken from the far end, against itself with numpy.roots: the worst |delta| / max|y| over
# gpu_cases().  The GPU test allows the kernel C_FACTOR times that on top of the fp32 roundings.
C_MEASURED = 1.36e-10
C_FACTOR = 16.0
DELTA_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                          "formant_norm_delta.json")
# the end-to-end cases of that tool and of the GPU test
E2E_RATIOS = (0.85, 1.15)
CLOSED_TARGET = (600.0, 1350.0, 2500.0)
CLOSED_ROWS = ((120.0, 0, 0.9), (210.0, 1, 1.12))          # (f0, seed, the scale of the three resonances)


def sanitize_q(q):
    """the fp32 ratios as the kernel reads them, in fp64: the nearer bound outside [0.5, 2], 1 for a NaN"""
    v = np.asarray(q, dtype=np.float32).astype(np.float64)
    return np.where(np.isnan(v), 1.0, np.clip(v, Q_LOW, Q_HIGH))


def knee(q):
    """phi0 = 0.85 pi min(1, 1 / q)"""
    return KNEE * math.pi * min(1.0, 1.0 / q)


def warp_angle(phi, q):
    """phi' = q phi up to the knee, from there the straight line to (pi, pi)"""
    phi0 = knee(q)
    if phi <= phi0:
        return q * phi
    return q * phi0 + (math.pi - q * phi0) * (phi - phi0) / (math.pi - phi0)


def rebuild(z, q):
    """-> (a' [21], ok, the relative imaginary parts [20], kept poles at or below the knee, above it): the reals kept,
    the upper half-plane's angles warped, the lower half-plane dropped"""
    mod = np.abs(z)
    rel = np.where(mod > 0, z.imag / np.where(mod > 0, mod, 1.0), 0.0)
    real = np.abs(rel) <= M.REAL_REL
    up = rel > M.REAL_REL
    if 2 * int(up.sum()) + int(real.sum()) != P:
        return None, False, rel, 0, 0
    poly = np.ones(1)
    for v in z[real].real:
        poly = np.convolve(poly, np.array([1.0, -v]))
    below = above = 0
    for v in z[up]:
        m = abs(v)
        phi = math.atan2(v.imag, v.real)
        below, above = below + (phi <= knee(q)), above + (phi > knee(q))
        poly = np.convolve(poly, np.array([1.0, -2.0 * m * math.cos(warp_angle(phi, q)), m * m]))
    return poly, True, rel, below, above


def frame(f, q, roots=M.numpy_roots, reverse_acf=False):
    """one windowed frame -> (rec [320], status, near a decision?, kept poles below the knee, above it)"""
    r = M.autocorr(f, reverse_acf)
    near = abs(r[0] / M.SILENCE - 1.0) <= M.NEAR_R0
    if r[0] < M.SILENCE:
        return f.copy(), SILENT, near, 0, 0
    r[0] *= 1.0 + M.R0_LIFT
    a, ks, ok = M.levinson(r)
    near = near or bool((np.abs(np.abs(ks) - 1.0) <= M.NEAR_K).any())
    if not ok:
        return f.copy(), FALLBACK, near, 0, 0
    z, _, conv = roots(a)
    a2, ok, rel, below, above = rebuild(z, q)
    near = near or bool(((np.abs(rel) > M.NEAR_IM[0]) & (np.abs(rel) < M.NEAR_IM[1])).any())
    if not conv or not ok:
        return f.copy(), FALLBACK, near, 0, 0
    return M.filters(f, a, a2), OK, near, below, above


def pole_warp(wav, q, n_valid, level=True, roots=M.numpy_roots, reverse_acf=False, copy_unity=True):
    """wav [B, N] (the fp32 values), q [B], n_valid [B] -> a namespace of fp64 arrays with the fields of
    mcadams_ref.mcadams (F, Fa, Fb, y, gain, out, status, near, left_out, n_valid; ``q`` for its alpha) and
    below, above int [B]: the kept poles of the row's transformed frames at or below the knee and above it.
    ``copy_unity=False`` sends rows at q = 1 through the frames like any other (the window identity's test)."""
    x = np.asarray(wav, dtype=np.float32).astype(np.float64)
    B, N = x.shape
    T = M.n_frames(N)
    qs = sanitize_q(q)
    nv = np.clip(np.asarray(n_valid, dtype=np.int64), 0, N)
    F = np.zeros((B, T, W))
    status = np.zeros((B, T), dtype=np.int32)
    near = np.zeros((B, T), dtype=bool)
    below, above = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    y, out, gain = np.zeros((B, N)), np.zeros((B, N)), np.ones(B)
    n = np.arange(N)
    t0 = n // H
    for b in range(B):
        live = n < nv[b]
        fr = M.frames_of(x[b], nv[b])
        if qs[b] == 1.0 and copy_unity:
            y[b] = np.where(live, x[b], 0.0)
            out[b] = y[b]
            F[b] = fr * M.WINDOW[None, :]
            continue
        for t in range(T):
            rec, status[b, t], near[b, t], lo, hi = frame(fr[t], qs[b], roots, reverse_acf)
            below[b] += lo
            above[b] += hi
            F[b, t] = rec * M.WINDOW
        y[b] = np.where(live, F[b, t0, n - H * t0 + H] + F[b, t0 + 1, n - H * t0], 0.0)
        if level:
            sx, sy = float(np.sum((x[b] * live) ** 2)), float(np.sum(y[b] ** 2))
            if sx > 0.0 and sy > 0.0:
                gain[b] = math.sqrt(sx / sy)
        out[b] = gain[b] * y[b]
    left_out = near[:, t0] | near[:, t0 + 1]
    live = n[None, :] < nv[:, None]
    rows = np.arange(B)[:, None]
    Fa = np.where(live, F[rows, t0[None, :], (n - H * t0 + H)[None, :]], 0.0)
    Fb = np.where(live, F[rows, t0[None, :] + 1, (n - H * t0)[None, :]], 0.0)
    return types.SimpleNamespace(x=x, q=qs, n_valid=nv, F=F, Fa=Fa, Fb=Fb, y=y, gain=gain, out=out, status=status,
                                 near=near, left_out=left_out, below=below, above=above)


gain_bar = M.gain_bar                    # (the derivation holds for any frames: it reads y, Fa, Fb, gain, n_valid)


def centre(freq, status, f0, frames, target_hz, q_min=0.8, q_max=1.2, min_frames=MIN_FRAMES):
    """the tracks (the fp32 values) -> a namespace: med fp32 [B, 3], q fp32 [B], q64 fp64 [B] (before its rounding),
    count int32 [B].  f0 None: every frame voiced.  A row with fewer than min_frames counted frames gets med 0, q 1,
    count 0."""
    freq = np.asarray(freq, dtype=np.float32)
    status = np.asarray(status)
    B, T, _ = freq.shape
    med, q = np.zeros((B, NF), np.float32), np.ones(B, np.float32)
    q64, count = np.ones(B), np.zeros(B, np.int32)
    for b in range(B):
        Fb = min(max(int(frames[b]), 0), T)
        ok = (np.arange(T) < Fb) & (status[b] == 0)
        if f0 is not None:
            with np.errstate(invalid="ignore"):
                ok &= np.asarray(f0, dtype=np.float32)[b] > 0
        n = int(ok.sum())
        if n < min_frames:
            continue
        count[b] = n
        for k in range(NF):
            med[b, k] = LF.lower_median(freq[b, ok, k])
        v = math.exp(sum(math.log(float(target_hz[k]) / float(med[b, k])) for k in range(NF)) / 3.0)
        q64[b] = min(max(v, float(q_min)), float(q_max))
        q[b] = np.float32(q64[b])
    return types.SimpleNamespace(med=med, q=q, q64=q64, count=count)


def geometric_distance(med, target_hz):
    """exp(mean ln(med_k / t_k)): 1 when the three medians lie on the target"""
    return math.exp(sum(math.log(float(med[k]) / float(target_hz[k])) for k in range(NF)) / 3.0)


def recorded():
    """profiles/formant_norm_delta.json, what tools/formant_norm_delta.py wrote"""
    with open(DELTA_JSON) as f:
        return json.load(f)


# ---- the kernel test's inputs ---------------------------------------------------------------------------
def gpu_cases():
    """the cases of the pole-warp test: [(name, wav fp32 [B, N], q fp32 [B], n_valid int32 [B])], on the waveforms of
    mcadams_ref.gpu_cases(): N = 1687 is no multiple of the hop, one row at q = 1 and one cut at 1000; N = 50 has two
    frames and is shorter than the window; one row of the third case has no valid sample; a row of
    data.synthetic_gender_dataset; an all-zero row next to a voiced one."""
    waves = {c[0]: (c[1], c[3]) for c in M.gpu_cases()}
    zeros = np.zeros((2, 700), np.float32)
    zeros[1] = M.voiced_row(150.0, M.FORMANTS, 700, 11)
    return [("odd", waves["odd"][0], np.array([0.85, 1.0, 1.15], np.float32), waves["odd"][1]),
            ("two_frames", waves["two_frames"][0], np.array([0.85], np.float32), waves["two_frames"][1]),
            ("empty_row", waves["empty_row"][0], np.array([1.15, 0.9], np.float32), waves["empty_row"][1]),
            ("synthetic", waves["synthetic"][0], np.array([1.2], np.float32), waves["synthetic"][1]),
            ("zero_row", zeros, np.array([0.85, 1.15], np.float32), np.array([700, 700], np.int32))]


_REF_CACHE = {}


def case_ref(name, level):
    """the restatement of a case, computed once per (case, level) and shared: treat it as read-only"""
    key = (name, bool(level))
    if key not in _REF_CACHE:
        wav, q, nv = {c[0]: c[1:] for c in gpu_cases()}[name]
        _REF_CACHE[key] = pole_warp(wav, q, nv, level)
    return _REF_CACHE[key]


def centre_case(T, seed=0):
    """given tracks for the centre test at T frames, B = 4 rows: formants drawn around row-wise scales of 700 / 1220 /
    2600 Hz, statuses 0..3 and unvoiced frames mixed in.  Row 0: every frame counted; row 1: ``frames`` below T; row
    2: ``frames`` past T; row 3: at most min(T, 5) counted frames, fewer than the default min_frames
    -> (freq fp32 [4, T, 3], status int32 [4, T], f0 fp32 [4, T], frames int32 [4])"""
    rng = np.random.default_rng(9000 + 17 * T + seed)
    B = 4
    centre_hz = np.array([700.0, 1220.0, 2600.0])
    scale = np.array([1.0, 1.1, 0.92, 1.05])[:, None, None]
    freq = (centre_hz * scale * (1.0 + 0.05 * rng.standard_normal((B, T, NF)))).astype(np.float32)
    status = rng.choice([0, 0, 0, 0, 0, 1, 2, 3], size=(B, T)).astype(np.int32)
    f0 = np.where(rng.random((B, T)) < 0.85, 100.0 + 80.0 * rng.random((B, T)), 0.0).astype(np.float32)
    status[0], f0[0] = 0, 120.0
    status[3] = np.where(np.arange(T) < 5, 0, 3)
    freq[status != 0] = 0.0                                 # as the tracks kernel leaves them
    frames = np.array([T, max(T - 3, 0), T + 5, T], np.int32)
    return freq, status, f0, frames


def closed_rows():
    """the two rows of the closed-loop figures, fp32 [2, 4800]: voiced rows whose three resonances are scaled"""
    return np.stack([M.voiced_row(f0, tuple((fc * s, bw) for fc, bw in M.FORMANTS), LF.E2E_SAMPLES, seed)
                     for f0, seed, s in CLOSED_ROWS]).astype(np.float32)


def closed_f0(T):
    """their F0 tracks as the figures take them: every frame voiced at the known fundamental, fp32 [2, T]"""
    return np.tile(np.array([f0 for f0, _, _ in CLOSED_ROWS], np.float32)[:, None], (1, T))
