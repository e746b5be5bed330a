"""fp64 / int64 restatement of the F0-contour pitch modification (ops.pitch_contour, pv_synth_map,
env_warp_frames, pitch_resample_map; csrc/sa_contour.hip) on the CPU, on top of tests/pitch_ref.py,
tests/phasevoc_ref.py and tests/formant_ref.py: the per-frame ratio, the integer time map, the stretch positions, the
synthesis, the resampling, the whole path, and the test material -- rows whose pitch MOVES, which
data.synthetic_gender_dataset's steady rows cannot show.  Shared by tests/test_contour_cpu.py,
tests/test_contour_gpu.py and tools/contour_delta.py."""
import math
import types

import numpy as np
import torch

from tests import formant_ref as F
from tests import phasevoc_ref as V
from tests import pitch_ref as P

HOP = P.HOP
RHO_ONE, Q_BITS = 1 << 16, 17
Q_ONE = 1 << Q_BITS
F_FLOOR = 60.0
SMOOTH_MAX = 8
N_CASE = 24000


def f32(x):
    """a scalar as the entry points receive it: rounded to fp32"""
    return float(np.float32(x))


# ---- (1)-(4) the ratio per frame -----------------------------------------------------------------------
def fill(f0, F_b):
    """f^ [T] fp64 of one row whose first F_b frames count and hold a voiced frame: the voiced values, linear between
    the voiced neighbours, held outside them"""
    f0 = np.asarray(f0, dtype=np.float64)
    T = f0.shape[0]
    voiced = np.flatnonzero((f0 > 0) & (np.arange(T) < F_b))
    out = np.empty(T)
    for t in range(T):
        k = int(np.searchsorted(voiced, t))
        if k < voiced.size and voiced[k] == t:
            out[t] = f0[t]
        elif k == 0:
            out[t] = f0[voiced[0]]
        elif k == voiced.size:
            out[t] = f0[voiced[-1]]
        else:
            l, n = int(voiced[k - 1]), int(voiced[k])
            out[t] = f0[l] + (f0[n] - f0[l]) * (t - l) / (n - l)
    return out


def smooth(fh, s):
    """f~[t] = sum_{|j| <= s} (s + 1 - |j|) f^[clamp(t + j)] / (s + 1)^2, j ascending"""
    T = fh.shape[0]
    idx = np.arange(T)
    acc = np.zeros(T)
    for j in range(-s, s + 1):
        acc = acc + (s + 1 - abs(j)) * fh[np.clip(idx + j, 0, T - 1)]
    return acc / float((s + 1) ** 2)


def contour(f0, lens, N, target_hz=170.0, gamma=1.0, s=2, r_min=0.5, r_max=2.0, min_voiced=5):
    """f0 [B, T] (the fp32 values), lens [B], N -> a namespace: rho_q int64 [B, T], Q int64 [B, T], Tq int64 [B], mean
    fp64 [B], voiced int64 [B], and what the decision margins are read from -- raw [B, T] = g / f~ before the clamp and
    scaled [B, T] = 2^16 rho before rint (both NaN on a row that is not moved), moved bool [B]"""
    f0 = torch.as_tensor(f0, dtype=torch.float32).double()
    B, T = f0.shape
    target, gamma, r_min, r_max = f32(target_hz), f32(gamma), f32(r_min), f32(r_max)
    _, mean, voiced = P.ratio(f0, lens, N, min_voiced=0)
    F_b = (P.n_valid(lens, N) // HOP + 1).clamp(max=T)
    rho_q = np.full((B, T), RHO_ONE, dtype=np.int64)
    raw, scaled = np.full((B, T), np.nan), np.full((B, T), np.nan)
    moved = np.zeros(B, dtype=bool)
    for b in range(B):
        if int(voiced[b]) < min_voiced or int(voiced[b]) == 0:
            continue
        moved[b] = True
        ft = smooth(fill(f0[b].numpy(), int(F_b[b])), int(s))
        g = np.maximum(F_FLOOR, target + gamma * (ft - float(mean[b])))
        raw[b] = g / ft
        scaled[b] = np.clip(raw[b], r_min, r_max) * 65536.0
        rho_q[b] = np.rint(scaled[b]).astype(np.int64)
    Q, Tq = time_map(rho_q)
    return types.SimpleNamespace(rho_q=torch.from_numpy(rho_q), Q=Q, Tq=Tq, mean=mean, voiced=voiced,
                                 raw=torch.from_numpy(raw), scaled=torch.from_numpy(scaled),
                                 moved=torch.from_numpy(moved))


def constant_tables(r, T, B=1):
    """(rho_q, Q, Tq) of a ratio r (a multiple of 2^-16) held over T frames"""
    rho_q = torch.full((B, T), int(round(float(r) * RHO_ONE)), dtype=torch.int64)
    assert float(rho_q[0, 0]) == float(r) * RHO_ONE
    return (rho_q,) + time_map(rho_q)


# ---- (5) the time map ----------------------------------------------------------------------------------
def time_map(rho_q):
    """rho_q int64 [B, T] -> (Q int64 [B, T], Tq int64 [B]): Q[0] = 0, Q[t + 1] = Q[t] + rho_q[t] + rho_q[t + 1];
    T'_b = ((Q[T - 1] + 2^17 - 1) >> 17) + 1"""
    rho_q = torch.as_tensor(rho_q, dtype=torch.int64)
    w = rho_q[:, :-1] + rho_q[:, 1:]
    Q = torch.cat([torch.zeros_like(rho_q[:, :1]), w.cumsum(1)], 1)
    return Q, ((Q[:, -1] + Q_ONE - 1) >> Q_BITS) + 1


# ---- (6) the stretch positions -------------------------------------------------------------------------
def positions(rho_q, Q):
    """one row's tables [T] -> (T', i int64 [T'], a fp64 [T'] holding the fp32 weights): output frame t' reads between
    the frames i and i + 1"""
    rho_q, Q = torch.as_tensor(rho_q, dtype=torch.int64), torch.as_tensor(Q, dtype=torch.int64)
    T = Q.shape[0]
    Tb = int((int(Q[-1]) + Q_ONE - 1) >> Q_BITS) + 1
    X = torch.arange(Tb, dtype=torch.int64) << Q_BITS
    i = (torch.searchsorted(Q[:T - 1].contiguous(), X, right=True) - 1).clamp(0, T - 2)
    w = rho_q[i] + rho_q[i + 1]
    a = ((X - Q[i]).double() / w.double()).float().double()
    end = X >= Q[-1]
    i = torch.where(end, torch.full_like(i, T - 2), i)
    a = torch.where(end, torch.ones_like(a), a)
    return Tb, i, a


# ---- (7) phase and synthesis ---------------------------------------------------------------------------
def mix(a, mp, mq, fp32):
    """(1 - a) mp + a mq; fp32: as pn_mix rounds it, fmaf(a, mq, (1 - a) mp) on fp32 values"""
    if not fp32:
        return (1.0 - a) * mp + a * mq
    a32, p32, q32 = (np.asarray(v, dtype=np.float64).astype(np.float32) for v in (a, mp, mq))
    t = ((np.float32(1.0) - a32) * p32).astype(np.float32)
    return torch.from_numpy((a32.astype(np.float64) * q32.astype(np.float64) + t.astype(np.float64))
                            .astype(np.float32).astype(np.float64))


def pv_synth_map(R, rho_q, Q, mag=None, fp32=False):
    """R complex [B, T, K], the tables [B, T] -> (C complex128 [B, max T'_b, K], phi' in turns, S' fp64, [T'_b]): the
    recurrence of phasevoc_ref.pv_phase over the map's positions.  mag [B, T, K]: the magnitudes on the input grid
    (None: |R|); fp32: they are the kernel's fp32 values and are mixed as the kernel rounds"""
    R = torch.as_tensor(R).to(torch.complex128)
    th = V.theta(R)
    B, T, K = th.shape
    mag = R.abs() if mag is None else torch.as_tensor(mag).double()
    rows = [positions(rho_q[b], Q[b]) for b in range(B)]
    Tmax = max(tb for tb, _, _ in rows)
    phi = torch.zeros(B, Tmax, K, dtype=torch.float64)
    Sp = torch.zeros_like(phi)
    for b, (Tb, i, a) in enumerate(rows):
        d = V.increments(th[b], i)
        acc = th[b, 0] - torch.floor(th[b, 0])
        phi[b, 0] = acc
        for t in range(1, Tb):
            acc = acc + d[t - 1]
            acc = acc - torch.floor(acc)
            phi[b, t] = acc
        Sp[b, :Tb] = mix(a[:, None].expand(-1, K), mag[b, i], mag[b, i + 1], fp32)
    return torch.polar(Sp, 2.0 * math.pi * phi), phi, Sp, [tb for tb, _, _ in rows]


# ---- (8) the envelope, frame by frame ------------------------------------------------------------------
def env_warp_frames(S, q, n_c=30, floor_rel=1e-4, max_gain_db=40.0):
    """S [B, T, 201] (fp32 values), q [B, T] -> formant_ref.warp's namespace with every frame a row of its own (fields
    [B T, 1, 201])"""
    S = torch.as_tensor(S)
    B, T, K = S.shape
    return F.warp(S.reshape(B * T, 1, K), torch.as_tensor(q).reshape(B * T), n_c, floor_rel, max_gain_db)


# ---- (9) resample --------------------------------------------------------------------------------------
def sample_positions(rho_q, Q, n):
    """one row's tables, n int64 [...] -> (ip int64, fr fp64, r_loc fp64): Z = 160 Q[t] + w[t] (n - 160 t)"""
    T = Q.shape[0]
    t = (n // HOP).clamp(max=T - 2)
    w = rho_q[t] + rho_q[t + 1]
    Z = HOP * Q[t] + w * (n - HOP * t)
    return Z >> Q_BITS, (Z & (Q_ONE - 1)).double() / Q_ONE, w.double() / Q_ONE


def resample_map(y, rho_q, Q, nv, Nout):
    """y [B, Nin] fp64, the tables [B, T], nv [B] -> (out [B, Nout] fp64, sum_i |h| |y| per sample, taps per sample)"""
    y = torch.as_tensor(y, dtype=torch.float64)
    rho_q, Q = torch.as_tensor(rho_q, dtype=torch.int64), torch.as_tensor(Q, dtype=torch.int64)
    B, Nin = y.shape
    out = torch.zeros(B, Nout, dtype=torch.float64)
    mass = torch.zeros_like(out)
    taps = torch.zeros(B, Nout, dtype=torch.int64)
    for b in range(B):
        n = int(nv[b])
        if n == 0:
            continue
        Tb = int((int(Q[b, -1]) + Q_ONE - 1) >> Q_BITS) + 1
        end = min(Nin, (Tb - 1) * HOP)
        ip, fr, r = sample_positions(rho_q[b], Q[b], torch.arange(n, dtype=torch.int64))
        c = torch.clamp(1.0 / r, max=1.0)[:, None]
        H = 16.0 / c
        i = (torch.floor(ip.double() + fr - H[:, 0]).long() + 1)[:, None] + torch.arange(66)[None, :]
        u = (ip[:, None] - i).double() + fr[:, None]
        live = (u.abs() < H) & (i >= 0) & (i < end)
        h = c * torch.sinc(c * u) * (0.5 + 0.5 * torch.cos(math.pi * u / H))
        h = torch.where(live, h, torch.zeros_like(h))
        yy = y[b][i.clamp(0, Nin - 1)]
        out[b, :n] = (h * yy).sum(-1)
        mass[b, :n] = (h.abs() * yy.abs()).sum(-1)
        taps[b, :n] = live.sum(-1)
    return out, mass, taps


# ---- the whole path ------------------------------------------------------------------------------------
def normalize(wav, lens, target_hz=170.0, gamma=1.0, s=2, beta=None, r_min=0.5, r_max=2.0, min_voiced=5,
              threshold=0.15, n_c=30, floor_rel=1e-4, max_gain_db=40.0):
    """the path of PitchNormalizer(phase="vocoder", contour_scale=gamma): pad -> YIN of the padded waveform -> contour
    -> STFT [-> the warp of |R| at q[b, t] = rho[b, t] / beta] -> pv_synth_map -> ISTFT -> resample_map
    -> (out [B, N] fp64, the contour namespace, f0 of the input [B, T])"""
    wav = torch.as_tensor(wav, dtype=torch.float64)
    B, N = wav.shape
    Np = HOP * -(-N // HOP)
    wp = torch.nn.functional.pad(wav, (0, Np - N))
    f0 = P.yin(wp, threshold)[0].float().double()
    c = contour(f0, lens, N, target_hz, gamma, s, r_min, r_max, min_voiced)
    R = P.stft(wp)
    mag = None
    if beta is not None:
        q = (c.rho_q.float() / np.float32(RHO_ONE * float(beta)))
        mag = env_warp_frames(R.abs().float(), q, n_c, floor_rel, max_gain_db).out.reshape(B, R.shape[1], -1)
    C = pv_synth_map(R, c.rho_q, c.Q, mag)[0]
    return resample_map(P.istft(C), c.rho_q, c.Q, P.n_valid(lens, N), N)[0], c, f0


# ---- the kernel test's inputs --------------------------------------------------------------------------
# (gamma, smooth, r_min, r_max) of the calls the GPU test makes on ``contour_rows``: the monotone voice (both clamps
# active on row 5), the additive shift unsmoothed, the floor (row 6) under the widest triangle, a compression, and
# bounds narrower than the kernels'
CONTOUR_CALLS = ((0.0, 2, 0.5, 2.0), (1.0, 0, 0.5, 2.0), (2.0, 8, 0.5, 2.0), (0.5, 2, 0.5, 2.0), (0.0, 1, 0.8, 1.25))


def contour_rows(W, seed=2):
    """hand-made f0 rows, no tracker -> (f0 fp32 [8, T], lens [8], N) with T = 2 W + 17, W the contour kernel's pass
    width, so that a row is two full passes and a partial one:
      0 an all-voiced glide, 110 -> 190 Hz          4 lens 0.6: F_b < T, with voiced frames (300 Hz) beyond the cut
      1 gaps at the start, across frame W and       5 a sweep 62 -> 395 Hz: at gamma 0 both clamps are active
        across frame 2 W to the end                 6 a sweep 80 -> 300 Hz: at gamma 2 the floor is active
      2 three voiced frames (< min_voiced)          7 voiced runs of random lengths with gaps between them, one of
      3 all unvoiced                                  them across frame W
    (The seed is one at which no decision of any call in CONTOUR_CALLS is marginal: tests/test_contour_cpu.py.)"""
    T = 2 * W + 17
    N = (T - 1) * HOP
    g = torch.Generator().manual_seed(100 + seed)
    jit = lambda n: torch.rand(n, generator=g, dtype=torch.float64)
    t = torch.arange(T, dtype=torch.float64)
    f0 = torch.zeros(8, T, dtype=torch.float64)
    f0[0] = 110.0 + 80.0 * t / (T - 1) + 0.3 * jit(T)
    f0[1] = 150.0 + 25.0 * torch.sin(2 * math.pi * t / 33.0) + 0.3 * jit(T)
    f0[1, :20] = 0.0
    f0[1, W - 6:W + 6] = 0.0
    f0[1, 2 * W - 7:] = 0.0
    f0[2, [5, W + 1, 2 * W + 3]] = torch.tensor([140.0, 150.0, 160.0], dtype=torch.float64)
    f0[4] = 130.0 + 40.0 * t / (T - 1) + 0.3 * jit(T)
    f0[4, int(0.6 * T) + 2:] = 300.0
    f0[4, 100:110] = 0.0
    f0[5] = 62.0 + 333.0 * t / (T - 1) + 0.3 * jit(T)
    f0[6] = 80.0 + 220.0 * t / (T - 1) + 0.3 * jit(T)
    pos, on = 3, True
    while pos < T:
        n = int(torch.randint(3, 40, (1,), generator=g))
        if on:
            f0[7, pos:pos + n] = 90.0 + 200.0 * jit(min(n, T - pos))
        pos, on = pos + n, not on
    f0[7, W - 3:W + 4] = 0.0
    lens = torch.ones(8)
    lens[4] = 0.6
    return f0.float(), lens, N


def contour_rows_T2():
    """T = 2, N = 160 (min_voiced 1): both frames voiced, either one, none, and values that reach the clamps"""
    f0 = torch.tensor([[150.0, 190.0], [140.0, 0.0], [0.0, 210.0], [0.0, 0.0], [70.0, 399.0], [61.5, 63.25],
                       [390.0, 380.0], [170.0, 170.0]])
    return f0, torch.ones(8), 160


def margins(c, r_min=0.5, r_max=2.0):
    """the smallest distances of a contour namespace's decisions from their thresholds -> (rint: of 2^16 rho from a
    half-integer, clamp: of g / f~ from a bound it has not passed by more than that)"""
    s = c.scaled[c.moved]
    rint = float(((s - torch.floor(s)) - 0.5).abs().min()) if s.numel() else float("inf")
    raw = c.raw[c.moved]
    d = torch.minimum((raw - f32(r_min)).abs(), (raw - f32(r_max)).abs())
    return rint, float(d.min()) if raw.numel() else float("inf")


# ---- the test material ---------------------------------------------------------------------------------
def glide_row(f_of_t, n, gen, noise=0.02):
    """pitch_ref.harmonic_row with a moving fundamental: eight partials at the multiples of the running integral of
    f_of_t (a function of the time in seconds, fp64 [n] -> Hz), random decaying amplitudes and phases, plus white
    noise; fp64 [n]"""
    t = torch.arange(n, dtype=torch.float64) / P.SR
    f = f_of_t(t)
    turns = (torch.cumsum(f, 0) - f) / P.SR                   # the integral up to sample n, in turns
    w = noise * torch.randn(n, generator=gen, dtype=torch.float64)
    for h in range(1, 9):
        amp = 0.3 / h * (0.5 + torch.rand(1, generator=gen, dtype=torch.float64))
        ph = 2 * math.pi * torch.rand(1, generator=gen, dtype=torch.float64)
        w += amp * torch.sin(2 * math.pi * h * turns + ph)
    return w


def glide_f0(t, n=N_CASE):
    """110 -> 190 Hz over the row"""
    return 110.0 + 80.0 * t / (n / P.SR)


def vibrato_f0(t):
    """150 +- 25 Hz at 3 Hz"""
    return 150.0 + 25.0 * torch.sin(2 * math.pi * 3.0 * t)


def case_rows(n=N_CASE, seed=2020):
    """fp32 [2, n]: the glide and the vibrato row"""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([glide_row(lambda t: glide_f0(t, n), n, g), glide_row(vibrato_f0, n, g)]).float()


def steady_row(f=140.0, n=N_CASE, seed=2021):
    return P.harmonic_row(f, n, torch.Generator().manual_seed(seed))[None].float()


EDGE = 3                                  # frames left out at either end of a row


def f0_stats(f0, lens, N):
    """f0 [B, T] -> (mean [B], std [B], voiced mask [B, T]) of the voiced frames among the counted ones, the first and
    the last EDGE of those left out"""
    f0 = torch.as_tensor(f0, dtype=torch.float64)
    B, T = f0.shape
    F_b = (P.n_valid(lens, N) // HOP + 1).clamp(max=T)
    idx = torch.arange(T)[None, :]
    live = (f0 > 0) & (idx >= EDGE) & (idx < (F_b - EDGE)[:, None])
    n = live.sum(1).clamp(min=1).double()
    mean = (f0 * live).sum(1) / n
    std = ((((f0 - mean[:, None]) ** 2) * live).sum(1) / n).sqrt()
    return mean, std, live


def contour_error(f0_in, f0_out, mean_in, lens, N, target, gamma):
    """worst |f0_out - (target + gamma (f0_in - mean_in))| per row over the frames voiced in both, edges left out"""
    _, _, li = f0_stats(f0_in, lens, N)
    _, _, lo = f0_stats(f0_out, lens, N)
    want = target + gamma * (torch.as_tensor(f0_in, dtype=torch.float64) - torch.as_tensor(mean_in).double()[:, None])
    err = (torch.as_tensor(f0_out, dtype=torch.float64) - want).abs() * (li & lo)
    return err.max(1).values, (li & lo).sum(1)


def delta_cases(target=170.0, gammas=(0.0, 0.5, 1.0), report=None, beta=None, path=None, tracker=None):
    """the glide and the vibrato row through ``path`` (default: this module's ``normalize``) -> {gamma: a dict of per-row
    lists}: std_in, std_out, mean_err (|voiced mean - target|), worst (the worst per-frame distance from the wanted
    contour), frames (those counted in it).  ``tracker``: wav [B, N] -> f0 [B, T] (default: the restatement's YIN)"""
    wav, lens = case_rows(), torch.ones(2)
    N = wav.shape[1]
    path = path or (lambda w, l, g: normalize(w, l, target, g, beta=beta)[0])
    track = tracker or (lambda w: P.yin(w.double())[0])
    f0_in = track(wav)
    mean_raw = P.voiced_mean(f0_in, lens, N)[0]
    mean_in, std_in, _ = f0_stats(f0_in, lens, N)
    res = {}
    for g in gammas:
        f0_out = track(torch.as_tensor(path(wav, lens, g)))
        mean_out, std_out, _ = f0_stats(f0_out, lens, N)
        worst, frames = contour_error(f0_in, f0_out, mean_raw, lens, N, target, g)
        res[g] = dict(std_in=std_in.tolist(), std_out=std_out.tolist(), mean_err=(mean_out - target).abs().tolist(),
                      worst=worst.tolist(), frames=frames.tolist())
        if report:
            for b, name in enumerate(("glide", "vibrato")):
                report(f"gamma {g:g} {name:8s} f0 std {float(std_in[b]):6.2f} -> {float(std_out[b]):6.2f} Hz, mean "
                       f"{float(mean_out[b]):8.3f} Hz, worst per-frame error {float(worst[b]):6.3f} Hz over "
                       f"{int(frames[b])} frames")
    return res
