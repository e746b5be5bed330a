"""Restatement of the Viterbi F0 tracker (speech_anonymization_amd.ops.f0_candidates / f0_viterbi
and csrc/sa_f0track.hip) in numpy and plain Python integers, on the CPU: the candidates of a d' row, the integer
decode, the refinement, and the scenario signals.  Shared by tests/test_f0_viterbi_cpu.py,
tests/test_f0_viterbi_gpu.py, tools/f0_viterbi_delta.py and tools/f0_viterbi_bench.py."""

import numpy as np
import torch

from tests import pitch_ref as P

SR, HOP, TAU_MIN, TAU_MAX = P.SR, P.HOP, P.TAU_MIN, P.TAU_MAX
K, STATES, FRAC = 8, 9, 16
ONE = 1 << FRAC
DEFAULTS = dict(voicing_cost=0.15, switch_cost=0.14, jump_cost=0.35, lag_bias=0.01)
ZERO_TRANSITIONS = dict(voicing_cost=0.15, switch_cost=0.0, jump_cost=0.0, lag_bias=0.0)
N_CASE, T_CASE = HOP * 39 + 37, 40


def log_table():
    """LOG[tau] = rint(log2(max(tau, 1)) 2^16), int32 [tau_max + 1]"""
    return np.rint(np.log2(np.maximum(np.arange(TAU_MAX + 1), 1).astype(np.float64)) * ONE).astype(np.int32)


def weights_q(voicing_cost=0.15, switch_cost=0.14, jump_cost=0.35, lag_bias=0.01):
    """the four weights as the host converts them: fp32, times 2^16, rounded to the nearest int (ties to even)"""
    return tuple(int(np.rint(np.float64(np.float32(w)) * ONE)) for w in (voicing_cost, switch_cost, jump_cost, lag_bias))


def frames_counted(lens, N, T):
    """F_b = min(T, round(lens_b N) / 160 + 1) as sa_pitch_ratio forms it (fp32 lens, fp64 product, NaN -> 0)"""
    out = []
    for v in np.asarray(lens, dtype=np.float32).reshape(-1):
        nb = np.rint(np.float64(v) * float(N))
        nb = min(max(nb, 0.0), float(N)) if nb == nb else 0.0
        out.append(min(int(T), int(nb) // HOP + 1))
    return out


# ---- (1) candidates -------------------------------------------------------------------------------------
def candidates(dp):
    """dp [B, T, 267] (fp32 values) -> (tau, q) int32 [B, T, K]: the K dips of smallest (q, tau), in ascending tau;
    unused slots tau = -1, q = 0"""
    dp = np.asarray(dp, dtype=np.float32)
    B, T, _ = dp.shape
    tau = np.full((B, T, K), -1, dtype=np.int32)
    q = np.zeros((B, T, K), dtype=np.int32)
    c = dp[..., TAU_MIN:TAU_MAX]
    dip = (c <= dp[..., TAU_MIN - 1:TAU_MAX - 1]) & (c < dp[..., TAU_MIN + 1:TAU_MAX + 1])
    cost = np.rint(np.clip(c.astype(np.float64), 0.0, 1.0) * ONE).astype(np.int64)
    for b in range(B):
        for t in range(T):
            lags = np.nonzero(dip[b, t])[0]
            keys = sorted((int(cost[b, t, i]), int(i) + TAU_MIN) for i in lags)[:K]
            for s, (tq, tt) in enumerate(sorted(keys, key=lambda e: e[1])):
                tau[b, t, s], q[b, t, s] = tt, tq
    return tau, q


# ---- (2) decode -----------------------------------------------------------------------------------------
def _clamp_tau(v):
    return -1 if v < 0 else min(max(int(v), TAU_MIN), TAU_MAX - 1)


def decode_row(tau, q, F, wq, LOG, return_costs=False):
    """tau, q [T, K] ints, the first F frames count -> path [T] (candidate index, -1 unvoiced and beyond F).  Plain
    Python integers; ties to the smaller state index at every step and at the end."""
    T = len(tau)
    vq, sq, jq, bq = wq
    LOG = [int(v) for v in LOG]
    lg = lambda x: LOG[min(max(x, 0), TAU_MAX)]
    path = [-1] * T
    prev, prev_tau, psi = None, None, []
    for t in range(F):
        taus = [_clamp_tau(v) for v in tau[t]]
        cur, psi_t = [], []
        for s in range(STATES):
            psi_s = 0
            if s < K and taus[s] < 0:
                cur.append(None)
            else:
                if s < K:
                    local = min(max(int(q[t][s]), 0), ONE) + ((bq * (lg(taus[s]) - lg(TAU_MIN))) >> FRAC)
                else:
                    local = vq
                best = 0
                if prev is not None:
                    best = None
                    for a in range(STATES):
                        if prev[a] is None:
                            continue
                        if a == K and s == K:
                            tr = 0
                        elif a == K or s == K:
                            tr = sq
                        else:
                            tr = (jq * abs(lg(prev_tau[a]) - lg(taus[s]))) >> FRAC
                        if best is None or prev[a] + tr < best:
                            best, psi_s = prev[a] + tr, a
                cur.append(local + best)
            psi_t.append(psi_s)
        psi.append(psi_t)
        prev, prev_tau = cur, taus
    final = [(c, s) for s, c in enumerate(prev) if c is not None]
    s = min(final)[1]
    for t in range(F - 1, -1, -1):
        path[t] = s if s < K else -1
        s = psi[t][s]
    if return_costs:
        return path, sorted(c for c, _ in final)
    return path


def decode(tau, q, lens, N, LOG=None, **costs):
    """tau, q [B, T, K] -> path int32 [B, T]"""
    tau, q = np.asarray(tau), np.asarray(q)
    B, T, _ = tau.shape
    LOG = log_table() if LOG is None else LOG
    wq = weights_q(**dict(DEFAULTS, **costs))
    F = frames_counted(lens, N, T)
    return np.array([decode_row(tau[b].tolist(), q[b].tolist(), F[b], wq, LOG) for b in range(B)], dtype=np.int32)


def per_frame_rule(tau, q, F, vq):
    """what the decode reduces to without transition weights and lag bias: the deepest dip (the smaller index on a
    tie) if its cost is at most the voicing cost, else unvoiced"""
    out = [-1] * len(tau)
    for t in range(F):
        live = [(min(max(int(q[t][s]), 0), ONE), s) for s in range(K) if tau[t][s] >= 0]
        if live and min(live)[0] <= vq:
            out[t] = min(live)[1]
    return out


# ---- (3) refinement -------------------------------------------------------------------------------------
def refine(dp, lag):
    """dp [B, T, 267] fp32 values, lag [B, T] (0: unvoiced) -> f0 fp32 [B, T]: 16000 / (tau + off) with the parabola
    of sa_yin_f0, fp64 from the fp32 d', rounded once"""
    dp = np.asarray(dp, dtype=np.float32).astype(np.float64)
    lag = np.asarray(lag, dtype=np.int64)
    p = np.clip(lag, 1, TAU_MAX - 1)
    a = np.take_along_axis(dp, (p - 1)[..., None], -1)[..., 0]
    c = np.take_along_axis(dp, p[..., None], -1)[..., 0]
    e = np.take_along_axis(dp, (p + 1)[..., None], -1)[..., 0]
    den = a - 2.0 * c + e
    off = np.where(den > 0.0, 0.5 * (a - e) / np.where(den > 0.0, den, 1.0), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):               # (the unvoiced frames' values are discarded)
        return np.where(lag > 0, SR / (p.astype(np.float64) + off), 0.0).astype(np.float32)


def lags_of(tau, path):
    """the lag each path entry names (0: unvoiced)"""
    tau, path = np.asarray(tau), np.asarray(path)
    pick = np.take_along_axis(tau, np.clip(path, 0, K - 1)[..., None], -1)[..., 0]
    return np.where(path >= 0, np.clip(pick, TAU_MIN, TAU_MAX - 1), 0).astype(np.int64)


def track(dp, lens, N, LOG=None, **costs):
    """dp [B, T, 267] fp32 values -> (f0 fp32 [B, T], path int32 [B, T], tau, q)"""
    tau, q = candidates(dp)
    path = decode(tau, q, lens, N, LOG, **costs)
    return refine(dp, lags_of(tau, path)), path, tau, q


def yin_f0(dp, threshold=0.15):
    """first-dip YIN on the same fp32 d' -> (f0 fp32 [B, T], lag [B, T])"""
    d = torch.from_numpy(np.asarray(dp, dtype=np.float32)).double()
    p = P.yin_pick(d, threshold)
    return refine(dp, p.numpy()), p.numpy()


def dprime32(wav):
    """fp64 d' of tests/pitch_ref.py rounded to fp32, as numpy [B, T, 267]"""
    return P.yin_dprime(torch.as_tensor(np.asarray(wav), dtype=torch.float64)).float().numpy()


# ---- the scenario signals -------------------------------------------------------------------------------
def _time(N):
    return np.arange(N, dtype=np.float64) / SR


def weak_fundamental(N=N_CASE):
    """a1 sin(2 pi 100 n) + sin(2 pi 200 n + 0.7), a1 = 0.2 on samples 2400 < i < 4000, else 1"""
    n, i = _time(N), np.arange(N)
    a1 = np.where((i > 2400) & (i < 4000), 0.2, 1.0)
    return a1 * np.sin(2 * np.pi * 100.0 * n) + np.sin(2 * np.pi * 200.0 * n + 0.7)


def noise_burst(N=N_CASE):
    """sum_{k=1..5} sin(2 pi 140 k n + k) / k, plus 0.5 z on samples 3000 < i < 3200; z the first standard_normal(N) of
    numpy.random.default_rng(0)"""
    n, i = _time(N), np.arange(N)
    x = sum(np.sin(2 * np.pi * 140.0 * k * n + k) / k for k in range(1, 6))
    z = np.random.default_rng(0).standard_normal(N)
    return x + np.where((i > 3000) & (i < 3200), 0.5 * z, 0.0)


def glide(N=N_CASE):
    """five partials / k on a fundamental that moves linearly from 100 to 200 Hz over the row"""
    n = _time(N)
    phase = 2 * np.pi * (100.0 * n + 0.5 * (100.0 / (N / SR)) * n * n)
    return sum(np.sin(k * phase) / k for k in range(1, 6))


def harmonic_320(N=N_CASE):
    return P.harmonic_row(320.0, N, torch.Generator().manual_seed(2101), noise=0.02).numpy()


def white_noise(N=N_CASE):
    return 0.1 * np.random.default_rng(1).standard_normal(N)


SCENARIOS = (("weak fundamental", weak_fundamental), ("noise burst", noise_burst), ("glide", glide),
             ("320 Hz row", harmonic_320), ("white noise", white_noise), ("silence", lambda N=N_CASE: np.zeros(N)))


def scenario_rows(N=N_CASE):
    """the six rows as fp32 [6, N]"""
    return torch.from_numpy(np.stack([f(N) for _, f in SCENARIOS])).float()


def check_scenarios(f0_v, f0_y, report=None):
    """the scenario claims on the six rows' tracks (fp32 / fp64 arrays [6, 40]), asserted; shared by the CPU test (on
    the restatement) and the GPU test (on pitchnorm.f0_track)"""
    f0_v, f0_y = np.asarray(f0_v, dtype=np.float64), np.asarray(f0_y, dtype=np.float64)
    assert f0_v.shape == f0_y.shape == (6, T_CASE)
    mid = slice(2, 39)
    if report:
        for b, (name, _) in enumerate(SCENARIOS):
            report(f"{name}: yin     " + " ".join(f"{v:.0f}" for v in f0_y[b]))
            report(f"{name}: viterbi " + " ".join(f"{v:.0f}" for v in f0_v[b]))
    assert bool((np.abs(f0_v[0, mid] - 100.0) <= 1.0).all())
    assert int((f0_y[0] >= 190.0).sum()) >= 5
    assert bool((f0_v[1, mid] >= 100.0).all())
    assert bool(((f0_y[1] > 0.0) & (f0_y[1] < 80.0)).any())
    for b in (2, 3):
        voiced = f0_y[b] > 0.0
        assert int(voiced.sum()) >= 30
        assert bool((f0_v[b][voiced] == f0_y[b][voiced]).all())
    for b in (4, 5):
        assert bool((f0_v[b] == 0.0).all()) and bool((f0_y[b] == 0.0).all())


# ---- random integer candidates (the decode's own tests) --------------------------------------------------
def random_candidates(B, T, seed, absent=0.25, tie_runs=True):
    """host-made candidates [B, T, K] in ascending lag: random slots absent, frame T // 2 of every row without any
    candidate, and (tie_runs) stretches in which every present candidate has the same cost, so that the transition
    and the final choice fall to the tie rule"""
    g = np.random.default_rng(seed)
    tau = np.sort(np.stack([g.choice(np.arange(TAU_MIN, TAU_MAX), K, replace=False) for _ in range(B * T)]),
                  axis=-1).reshape(B, T, K).astype(np.int32)
    q = g.integers(0, ONE // 4, size=(B, T, K)).astype(np.int32)
    if tie_runs:
        for b in range(B):
            for start in range(3, T - 8, 37):
                q[b, start:start + 6] = int(g.integers(0, ONE // 8))
                tau[b, start:start + 6] = tau[b, start]
            q[b, T - 3:] = 5000
    gone = g.random((B, T, K)) < absent
    tau[gone], q[gone] = -1, 0
    tau[:, T // 2], q[:, T // 2] = -1, 0
    return tau, q
