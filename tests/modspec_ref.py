"""fp64 numpy restatement of the modulation-spectrum smoothing (include/sa_hip.h "modulation-spectrum
smoothing", speech_anonymization_amd.modspec and csrc/sa_modspec.hip), on the CPU: the taps, sa_modspec_smooth element
by element, the class on torch.stft / torch.istft in double (tests/pitch_ref.py's), and the modulation depth the
end-to-end checks read.  Shared by tests/test_modspec_cpu.py, tests/test_modspec_gpu.py and tools/modspec_delta.py."""
import json
import math
import os

import numpy as np
import torch

from tests import pitch_ref as P

NBIN, HOP, JMAX, FRAME_RATE = 201, 160, 64, 100.0
LN10_OVER_20 = 0.11512925464970229


def taps(cutoff_hz):
    """h[0..J] fp64, J = ceil(200 / cutoff): the Hann-windowed sinc normalised to h0 + 2 sum h_j = 1.  The sine is
    taken of the argument's distance to the nearest whole number, so a whole argument gives an exact zero."""
    J = int(math.ceil(200.0 / cutoff_hz))
    j = np.arange(J + 1, dtype=np.float64)
    x = 2.0 * cutoff_hz * j / FRAME_RATE
    n = np.round(x)
    sign = np.where(n % 2 == 0, 1.0, -1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(x == 0, 1.0, sign * np.sin(np.pi * (x - n)) / (np.pi * x))
    h = sinc * (0.5 + 0.5 * np.cos(np.pi * j / (J + 1)))
    return h / (h[0] + 2.0 * h[1:].sum())


def response(h, f_hz):
    """the zero-phase response of the symmetric filter with half h at f_hz of the 100 Hz frame rate"""
    j = np.arange(1, len(h))
    return float(h[0] + 2.0 * (h[1:] * np.cos(2.0 * np.pi * f_hz * j / FRAME_RATE)).sum())


def clamp_depth(d):
    d = float(np.float32(d))
    return 0.0 if not d > 0.0 else min(d, 1.0)               # (a NaN compares false: 0)


def log_mag(R, frames, floor_rel=1e-4):
    """R complex64 [B, T, K] -> (L fp64 [B, T, K] (rows past T_b left 0), peak fp64 [B], T_b list)"""
    R = np.asarray(R, dtype=np.complex64)
    B, T, _ = R.shape
    re, im = R.real.astype(np.float64), R.imag.astype(np.float64)
    m = np.sqrt(re * re + im * im)
    L, peak, Tb = np.zeros_like(m), np.zeros(B), []
    for b in range(B):
        tb = int(min(max(int(frames[b]), 0), T))
        Tb.append(tb)
        if tb:
            peak[b] = m[b, :tb].max()
            L[b, :tb] = np.log(np.maximum(m[b, :tb], max(float(np.float32(floor_rel)) * peak[b], 1e-10)))
    return L, peak, Tb


def smoothed(L, h, far=False):
    """s [T_b, K] of L [T_b, K]: h0 L[t] + sum_j h_j (L[c(t - j)] + L[c(t + j)]), j ascending (far: from j = J down,
    the centre last -- the perturbation of tools/modspec_delta.py)"""
    Tb = L.shape[0]
    idx = np.arange(Tb)
    pair = lambda j: h[j] * (L[np.clip(idx - j, 0, Tb - 1)] + L[np.clip(idx + j, 0, Tb - 1)])   # noqa: E731
    if far:
        s = np.zeros_like(L)
        for j in range(len(h) - 1, 0, -1):
            s = s + pair(j)
        return s + h[0] * L
    s = h[0] * L
    for j in range(1, len(h)):
        s = s + pair(j)
    return s


def smooth(R, h, depth, frames, floor_rel=1e-4, max_gain_db=40.0, far=False, nudge=0):
    """sa_modspec_smooth -> (C complex64 [B, T, K], peak fp64 [B], Lout fp64 [B, T, K], bound fp64 [B, T, K]: the
    sum of magnitudes |L[t]| + sum_j |h_j| (|L[c(t - j)]| + |L[c(t + j)]|) the bar on Lout scales with).
    nudge +-1: L moved by one ulp before the sum (tools/modspec_delta.py)."""
    R = np.asarray(R, dtype=np.complex64)
    h = np.asarray(h, dtype=np.float64)
    gmax = float(np.float32(float(max_gain_db) * LN10_OVER_20))
    L, peak, Tb = log_mag(R, frames, floor_rel)
    C, Lout, bound = R.copy(), np.zeros_like(L), np.zeros_like(L)
    re, im = R.real.astype(np.float64), R.imag.astype(np.float64)
    for b, tb in enumerate(Tb):
        if tb == 0:
            continue
        d = clamp_depth(depth[b])
        Lb = L[b, :tb]
        if nudge:
            Lb = np.nextafter(Lb, np.inf if nudge > 0 else -np.inf)
        g = np.clip(d * (smoothed(Lb, h, far) - Lb), -gmax, gmax)
        Lout[b, :tb] = Lb + g
        bound[b, :tb] = np.abs(Lb) + smoothed(np.abs(Lb), np.abs(h)) - abs(h[0]) * np.abs(Lb)
        if d != 0.0:
            e = np.exp(g)
            C[b, :tb] = ((re[b, :tb] * e).astype(np.float32) + 1j * (im[b, :tb] * e).astype(np.float32))
    return C, peak, Lout, bound


def spectrum(B, T, seed):
    """the kernel tests' input, complex64 [B, T, 201]: random, about 35 dB of spread, not an STFT; with exact zeros
    (every 37th element), frame 1 (if there is one) under the floor of floor_rel 1e-4, and bin 5 constant in time"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** (rng.uniform(-35.0, 0.0, (B, T, NBIN)) / 20.0)
    ph = rng.uniform(0.0, 2.0 * np.pi, (B, T, NBIN))
    R = (mag * np.exp(1j * ph)).astype(np.complex64)
    if T > 1:
        R[:, 1, :] *= np.float32(1e-7)
    R.reshape(-1)[::37] = 0
    R[:, :, 5] = np.complex64(0.25 - 0.125j)
    return R


def bits_differ(a, b):
    """the share of fp32 components of complex64 a, b whose bits differ"""
    a = np.ascontiguousarray(a, dtype=np.complex64).view(np.uint32)
    b = np.ascontiguousarray(b, dtype=np.complex64).view(np.uint32)
    return float((a != b).mean())


# ---- the class ------------------------------------------------------------------------------------------
def n_valid(lens, N):
    return np.clip(np.round(np.asarray(lens, dtype=np.float32).astype(np.float64) * N), 0, N).astype(np.int64)


def smoother(wav, lens, cutoff_hz=10.0, depth=1.0, floor_rel=1e-4, max_gain_db=40.0, istft32=False):
    """ModulationSmoother on the CPU: wav [B, N] -> [B, N] fp64 (istft32: the inversion carried in fp32, what
    tools/modspec_delta.py's figure (b) compares)"""
    wav = np.asarray(wav, dtype=np.float32)
    B, N = wav.shape
    Np = HOP * -(-N // HOP)
    wp = np.zeros((B, Np), dtype=np.float64)
    wp[:, :N] = wav
    R = P.stft(torch.from_numpy(wp)).numpy().astype(np.complex64)
    nv = n_valid(lens, N)
    C, _, _, _ = smooth(R, taps(cutoff_hz), [depth] * B, nv // HOP + 1, floor_rel, max_gain_db)
    if istft32:
        Ct = torch.from_numpy(C).transpose(1, 2)
        y = torch.istft(Ct, 400, 160, 400, window=P.window().float(), center=True, length=Np).double().numpy()
    else:
        y = P.istft(torch.from_numpy(C.astype(np.complex128))).numpy()
    y = y[:, :N].copy()
    y[np.arange(N)[None, :] >= nv[:, None]] = 0.0
    return y


# ---- end to end ------------------------------------------------------------------------------------------
E2E_FM, E2E_CUTOFF, E2E_SECONDS = (4.0, 20.0), 10.0, 2


def e2e_rows():
    """[2, 32000] fp32: 0.1 (1 + 0.5 cos 2 pi f_m t) sum_{k = 1..19} sin(2 pi 150 k t) / k at f_m = 4 and 20 Hz"""
    t = np.arange(E2E_SECONDS * 16000, dtype=np.float64) / 16000.0
    carrier = sum(np.sin(2.0 * np.pi * 150.0 * k * t) / k for k in range(1, 20))
    return np.stack([0.1 * (1.0 + 0.5 * np.cos(2.0 * np.pi * fm * t)) * carrier for fm in E2E_FM]).astype(np.float32)


def mod_depth(x, fm):
    """2 |mean_t e(t) exp(-2 pi i fm t / 100)| of the mean-removed per-frame log energy e (frames of 400 samples every
    160, none padded; ln of the sum of squares + 1e-12), with the first and last 10 frames dropped"""
    x = np.asarray(x, dtype=np.float64)
    T = (len(x) - 400) // HOP + 1
    fr = x[np.arange(T)[:, None] * HOP + np.arange(400)[None, :]]
    e = np.log((fr * fr).sum(1) + 1e-12)[10:-10]
    e = e - e.mean()
    t = np.arange(len(e))
    return float(2.0 * abs((e * np.exp(-2j * np.pi * fm * t / FRAME_RATE)).mean()))


def e2e_ratios(out, rows=None):
    rows = e2e_rows() if rows is None else rows
    return [mod_depth(out[i], fm) / mod_depth(rows[i], fm) for i, fm in enumerate(E2E_FM)]


# ---- the kernel tests' cases, shared with tools/modspec_delta.py -------------------------------------------
DELTA_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "modspec_delta.json")
CLASS_LENS = (1.0, 0.73)                  # of the end-to-end rows where the class is compared with its restatement
E2E_WANTED = (1.0, 0.0)                   # the ideal low-pass at 10 Hz: 4 Hz passes, 20 Hz does not


def case_taps(J):
    """the half filter of a kernel case: J = 0 the identity, J = 20 the 10 Hz low-pass, any other J a raised cosine
    with a negative lobe at its end (|h| and h differ), normalised"""
    if J == 0:
        return np.ones(1)
    if J == 20:
        return taps(10.0)
    j = np.arange(J + 1, dtype=np.float64)
    h = 0.5 + 0.5 * np.cos(np.pi * j / (J + 1))
    h[-1] = -0.25 * h[-1]
    return h / (h[0] + 2.0 * h[1:].sum())


def case_shapes(tile_frames):
    """(B, T, frames): the shapes of the kernel tests; the last is one frame past two of the kernel's time tiles"""
    return [(3, 211, (211, 97, 0)), (1, 2, (2,)), (2, 67, (5, 1)), (1, 2 * tile_frames + 1, (2 * tile_frames + 1,))]


CASE_J = (0, 1, 20, 64)
CASE_DEPTH = (1.0, 0.5, 0.0)
# (name, floor_rel, max_gain_db, depth or None for CASE_DEPTH): what is run on the first shape beside the defaults
CASE_EXTRA = (("floor_1e-2", 1e-2, 40.0, None), ("gain_3dB", 1e-4, 3.0, None),
              ("depth_nan_-1_2", 1e-4, 40.0, (float("nan"), -1.0, 2.0)))


def cases(tile_frames=128):
    """every kernel case as (id, B, T, frames, J, depth, floor_rel, max_gain_db)"""
    out = []
    for B, T, frames in case_shapes(tile_frames):
        for J in CASE_J:
            out.append((f"{B}x{T}_J{J}", B, T, frames, J, CASE_DEPTH[:B], 1e-4, 40.0))
    B, T, frames = case_shapes(tile_frames)[0]
    for name, fl, gdb, depth in CASE_EXTRA:
        for J in (20, 64):
            out.append((f"{B}x{T}_J{J}_{name}", B, T, frames, J, CASE_DEPTH if depth is None else depth, fl, gdb))
    return out


def case_input(B, T):
    return spectrum(B, T, 1000 * B + T)


def load_delta():
    with open(DELTA_FILE) as f:
        return json.loads(f.read())
