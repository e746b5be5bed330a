"""fp64 restatement of the LPC formant tracks and their comparison (ops.formant_tracks,
ops.formant_compare and csrc/sa_formants.hip), on the CPU with numpy: pre-emphasised Hamming frames of 400 at hop 160
on the F0 tracks' frame grid, autocorrelation LPC of order 18, the poles by ``numpy.roots`` (NOT by the kernel's Aberth
iteration: the check is independent of the method under test), the candidates gated by frequency and bandwidth, the
three lowest as F1..F3; then lower medians by sorting.  Shared by tests/test_formant_report_cpu.py,
tests/test_formant_report_gpu.py and tools/formant_report_delta.py, which swaps ``roots=`` and ``reverse_acf=`` to
measure how far equally valid fp64 evaluations lie apart (the spread of the GPU test's bar)."""
import json
import math
import os
import types

import numpy as np

from tests import mcadams_ref as M

SR, H, W, P, NF = 16000, 160, 400, 18, 3
U = 2.0 ** -24
PREEMPH = 0.97
SILENCE = 1e-10
R0_LIFT = 1e-9
IM_REL = 1e-6
F_LOW, F_HIGH, B_HIGH = 90.0, 5500.0, 700.0
ABERTH_TOL, ABERTH_MAX = 1e-14, 64
OK, SILENT, FALLBACK, SHORT = 0, 1, 2, 3
MIN_COMMON = 8
MAX_T = (1 << 24) // H + 1
# "near a decision": the frames a comparison would have to leave out
NEAR_IM = (1e-9, 1e-3)
NEAR_K = 1e-9
NEAR_R0 = 1e-6
NEAR_GATE = 1e-6

WINDOW = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(W) / (W - 1))

# tools/formant_report_delta.py (profiles/formant_report_delta.json): the restatement with its own fp64 Aberth iteration
# and with the lag sums taken from the far end, against itself with numpy.roots: the worst |delta f| and |delta b| in Hz
# over gpu_cases().  The GPU test allows the kernel SPREAD_FACTOR times that on top of the fp32 rounding.
SPREAD_HZ = {"f": 1.96e-11, "b": 5.13e-11}
SPREAD_FACTOR = 16.0
# the same tool, end to end on the three 4800-sample voiced rows: the relative distance of the restatement's
# per-formant ratios from theory (phi^alpha / phi, and 1.15), the worst over the rows per formant, every frame counted
# as voiced (known_f0).  The GPU test allows twice that.
E2E_ROWS = ((120.0, 0), (210.0, 1), (160.0, 2))             # (f0, seed) of voiced_row(f0, FORMANTS, 4800, seed)
E2E_SAMPLES = 4800
E2E_MCADAMS = {0.8: (0.0462, 0.0126, 0.0270), 0.6: (0.0520, 0.0151, 0.0678)}
E2E_SHIFT = {1.15: (0.0735, 0.0814, 0.3619)}
DELTA_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                          "formant_report_delta.json")


def n_frames(N):
    return int(N) // H + 1


def frames_of(x, n_valid):
    """x [N] fp64 -> the windowed frames [T, 400]: e[n] = x[n] - 0.97 x[n - 1], zero outside [0, n_valid); frame t
    covers [160 t - 200, 160 t + 200)"""
    N = x.shape[0]
    T = n_frames(N)
    live = np.arange(N) < n_valid
    xv = np.where(live, x, 0.0)
    e = np.where(live, xv - PREEMPH * np.concatenate(([0.0], xv[:-1])), 0.0)
    pad = np.zeros(H * (T - 1) + W)
    pad[W // 2:W // 2 + N] = e[:pad.shape[0] - W // 2]
    idx = H * np.arange(T)[:, None] + np.arange(W)[None, :]
    return pad[idx] * WINDOW[None, :]


def autocorr(f, reverse=False):
    """r_k = sum_j f[j] f[j + k], k = 0..18, summed in index order (``reverse``: from the far end)"""
    r = np.zeros(P + 1)
    for k in range(P + 1):
        prod = f[:W - k] * f[k:]
        r[k] = np.cumsum(prod[::-1] if reverse else prod)[-1]               # (a running sum: strictly in order)
    return r


def levinson(r):
    """-> (a [19] with a_0 = 1, the reflection coefficients [18], ok)"""
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
    """the kernel's root finder in fp64: -> (roots [18], converged)"""
    z = 0.9 * np.exp(2j * np.pi * (np.arange(P) + 0.25) / P)
    for _ in range(ABERTH_MAX):
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
            return z, True
    return z, False


def numpy_roots(a):
    return np.roots(a), True


def _near_gate(v, gate):
    return abs(v / gate - 1.0) <= NEAR_GATE


def frame(f, roots=numpy_roots, reverse_acf=False):
    """one windowed frame -> (F [3], B [3], status, near a decision?), all in fp64 and Hz"""
    zero = np.zeros(NF)
    r = autocorr(f, reverse_acf)
    near = abs(r[0] / SILENCE - 1.0) <= NEAR_R0
    if r[0] < SILENCE:
        return zero, zero, SILENT, near
    r[0] *= 1.0 + R0_LIFT
    a, ks, ok = levinson(r)
    near = near or bool((np.abs(np.abs(ks) - 1.0) <= NEAR_K).any())
    if not ok:
        return zero, zero, FALLBACK, near
    z, conv = roots(a)
    if not conv:
        return zero, zero, FALLBACK, near
    mod = np.abs(z)
    rel = z.imag / np.where(mod > 0, mod, 1.0)
    near = near or bool(((np.abs(rel) > NEAR_IM[0]) & (np.abs(rel) < NEAR_IM[1])).any())
    cand = rel > IM_REL
    fz = np.arctan2(z.imag, z.real)[cand] * (SR / (2.0 * math.pi))
    bz = -np.log(mod[cand]) * (SR / math.pi)
    near = near or any(_near_gate(v, F_LOW) or _near_gate(v, F_HIGH) for v in fz) or \
        any(_near_gate(v, B_HIGH) for v in bz)
    keep = (fz >= F_LOW) & (fz <= F_HIGH) & (bz <= B_HIGH)
    fz, bz = fz[keep], bz[keep]
    if fz.shape[0] < NF:
        return zero, zero, SHORT, near
    order = np.argsort(fz, kind="stable")[:NF]
    return fz[order], bz[order], OK, near


def tracks(wav, n_valid, roots=numpy_roots, reverse_acf=False):
    """wav [B, N] (the fp32 values), n_valid [B] -> a namespace: freq, bw fp64 [B, T, 3] (unrounded), status int32
    [B, T], near bool [B, T] (frames near a decision)"""
    x = np.asarray(wav, dtype=np.float32).astype(np.float64)
    B, N = x.shape
    T = n_frames(N)
    nv = np.clip(np.asarray(n_valid, dtype=np.int64), 0, N)
    freq, bw = np.zeros((B, T, NF)), np.zeros((B, T, NF))
    status = np.zeros((B, T), dtype=np.int32)
    near = np.zeros((B, T), dtype=bool)
    for b in range(B):
        fr = frames_of(x[b], nv[b])
        for t in range(T):
            freq[b, t], bw[b, t], status[b, t], near[b, t] = frame(fr[t], roots, reverse_acf)
    return types.SimpleNamespace(freq=freq, bw=bw, status=status, near=near, n_valid=nv)


def lower_median(v):
    """the element at index (n - 1) // 2 of the sorted values"""
    return np.sort(v)[(v.shape[0] - 1) // 2]


def compare(F_ref, F_deg, st_ref, st_deg, f0_ref, f0_deg, frames, min_common=MIN_COMMON):
    """the tracks (the fp32 values) -> a namespace: med, ratio fp32 [B, 3], shift fp32 [B], common int32 [B].  A row
    with fewer than min_common counted frames gets zeros, its common included"""
    F_ref, F_deg = (np.asarray(v, dtype=np.float32) for v in (F_ref, F_deg))
    f0_ref, f0_deg = (np.asarray(v, dtype=np.float32) for v in (f0_ref, f0_deg))
    st_ref, st_deg = np.asarray(st_ref), np.asarray(st_deg)
    B, T, _ = F_ref.shape
    med, ratio = np.zeros((B, NF), np.float32), np.zeros((B, NF), np.float32)
    shift, common = np.zeros(B, np.float32), np.zeros(B, np.int32)
    for b in range(B):
        Fb = min(max(int(frames[b]), 0), T)
        with np.errstate(invalid="ignore"):
            ok = (np.arange(T) < Fb) & (st_ref[b] == 0) & (st_deg[b] == 0) & (f0_ref[b] > 0) & (f0_deg[b] > 0)
        n = int(ok.sum())
        if n < min_common:
            continue
        common[b] = n
        for k in range(NF):
            d, g = F_deg[b, ok, k], F_ref[b, ok, k]
            med[b, k] = lower_median(d)
            ratio[b, k] = lower_median((d.astype(np.float64) / g.astype(np.float64)).astype(np.float32))
        shift[b] = np.float32(math.exp(sum(math.log(float(q)) for q in ratio[b]) / 3.0))
    return types.SimpleNamespace(med=med, ratio=ratio, shift=shift, common=common)


def bar(kind, ref):
    """|kernel - ref| allowed for a frequency ("f") or a bandwidth ("b") of value ref: the fp32 rounding of what is
    returned, and SPREAD_FACTOR times the spread of two fp64 evaluations"""
    return U * abs(ref) + SPREAD_FACTOR * SPREAD_HZ[kind]


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def recorded():
    """profiles/formant_report_delta.json, what tools/formant_report_delta.py wrote"""
    with open(DELTA_JSON) as f:
        return json.load(f)


# ---- the kernel test's inputs ---------------------------------------------------------------------------
FORMANTS = M.FORMANTS
voiced_row = M.voiced_row


def synthetic_row():
    """the first 4800 samples of data.synthetic_gender_dataset(2, 2, seed=1986)'s first row, fp32"""
    import torch
    from speech_anonymization_amd import data
    batch = next(iter(data.synthetic_gender_dataset(2, 2, seed=1986)))
    return batch.sig[0][0, :4800].to(torch.float32).numpy().copy()


def gpu_cases():
    """the cases of the tracks test: [(name, wav fp32 [B, N], n_valid int32 [B])].  N = 1687 is no multiple of the hop
    and has 11 frames, one row cut at 1000; N = 50 is one frame, shorter than the window; one row of the third case has
    no valid sample; a row of data.synthetic_gender_dataset; an all-zero row."""
    a = np.stack([voiced_row(120.0, FORMANTS, 1687, 0), voiced_row(210.0, FORMANTS, 1687, 1),
                  voiced_row(160.0, FORMANTS, 1687, 2)]).astype(np.float32)
    c = np.stack([voiced_row(140.0, FORMANTS, 1600, 4), voiced_row(180.0, FORMANTS, 1600, 5)]).astype(np.float32)
    return [("odd", a, np.array([1687, 1687, 1000], np.int32)),
            ("one_frame", voiced_row(200.0, FORMANTS, 50, 3)[None].astype(np.float32), np.array([50], np.int32)),
            ("empty_row", c, np.array([0, 1600], np.int32)),
            ("synthetic", synthetic_row()[None], np.array([4800], np.int32)),
            ("zeros", np.zeros((1, 800), np.float32), np.array([800], np.int32))]


def e2e_rows():
    """the three voiced rows of the end-to-end figures, fp32 [3, 4800]"""
    return np.stack([voiced_row(f0, FORMANTS, E2E_SAMPLES, seed) for f0, seed in E2E_ROWS]).astype(np.float32)


def known_f0(T):
    """the F0 tracks of the end-to-end rows as the end-to-end figures take them: every frame voiced, at the fundamental
    the row was made with, fp32 [3, T]"""
    return np.tile(np.array([f0 for f0, _ in E2E_ROWS], np.float32)[:, None], (1, T))


_REF_CACHE = {}


def case_ref(name):
    """the restatement of a case, computed once and shared: treat it as read-only"""
    if name not in _REF_CACHE:
        wav, nv = {c[0]: c[1:] for c in gpu_cases()}[name]
        _REF_CACHE[name] = tracks(wav, nv)
    return _REF_CACHE[name]


def compare_case(T, seed=0):
    """given tracks for the comparison test at T frames, B = 4 rows: formants drawn around 700 / 1220 / 2600 Hz and
    their degraded copies at row-wise scales with jitter, mixed statuses and unvoiced frames in both, ``frames`` below
    T in row 1, row 3 without a common frame -> (F_ref, F_deg fp32 [4, T, 3], st_ref, st_deg int32 [4, T], f0_ref,
    f0_deg fp32 [4, T], frames int32 [4])"""
    rng = np.random.default_rng(7000 + 13 * T + seed)
    B = 4
    centre = np.array([700.0, 1220.0, 2600.0])
    F_ref = (centre * (1.0 + 0.05 * rng.standard_normal((B, T, NF)))).astype(np.float32)
    scale = np.array([1.0, 1.15, 0.9, 1.3])[:, None, None] * np.array([1.0, 0.97, 1.02])
    F_deg = (F_ref.astype(np.float64) * scale * (1.0 + 0.02 * rng.standard_normal((B, T, NF)))).astype(np.float32)
    st_ref = rng.choice([0, 0, 0, 0, 0, 1, 2, 3], size=(B, T)).astype(np.int32)
    st_deg = rng.choice([0, 0, 0, 0, 0, 0, 1, 3], size=(B, T)).astype(np.int32)
    f0_ref = np.where(rng.random((B, T)) < 0.85, 100.0 + 80.0 * rng.random((B, T)), 0.0).astype(np.float32)
    f0_deg = np.where(rng.random((B, T)) < 0.85, 100.0 + 80.0 * rng.random((B, T)), 0.0).astype(np.float32)
    st_ref[0], st_deg[0] = 0, 0                             # row 0: every frame scored and voiced
    f0_ref[0], f0_deg[0] = 120.0, 125.0
    F_ref[st_ref != 0], F_deg[st_deg != 0] = 0.0, 0.0       # as the tracks kernel leaves them
    f0_deg[3] = np.where(f0_ref[3] > 0, 0.0, 150.0)         # row 3: never voiced in both
    frames = np.array([T, max(T - 3, 0), T + 5, T], np.int32)
    return F_ref, F_deg, st_ref, st_deg, f0_ref, f0_deg, frames
