"""fp64 restatement of the pitch-correlation scorer (include/sa_hip.h, csrc/sa_prosody.hip), written
from the formulas, with numpy only.  f0_ref, f0_deg [B, T] (the fp32 values, Hz, 0 or less: unvoiced), frames [B] ->

  v_ref[t] = (t < F_b and f0_ref[t] > 0), v_deg the same;  per lag l in [-Lg, Lg] over the frames t with t and t + l in
  [0, F_b) that are voiced in ref at t and in deg at t + l:  x = f0_ref[t], y = f0_deg[t + l], the means, then
  s_xx, s_yy, s_xy of the centred values;  valid when n >= m, s_xx > 0, s_yy > 0;  rho = s_xy / sqrt(s_xx s_yy)
  l* = the first lag of the walk 0, -1, +1, ..., -Lg, +Lg whose rho is strictly above every earlier valid one
  at l*:  e = 12 log2(y / x), its mean (shift_st) and standard deviation (dev_st), common = n, voicing = the share of
  the overlap's frames on which v_ref[t] = v_deg[t + l*];  no valid lag: zeros, voicing taken at lag 0

The keyword arguments of ``compare`` re-evaluate it with the four perturbations tools/prosody_delta.py measures.  The
module also holds the kernel test's cases, the bar, and the end-to-end figures of the delta tool."""
import math
import types

import numpy as np

U = 2.0 ** -24
MAX_LAG, MIN_COMMON = 8, 8                # the defaults of ops.f0_compare
OUTPUTS = ("rho", "shift_st", "dev_st", "voicing")
RHO_MARGIN = 1e-6                         # the winning lag of a test row leads every other valid lag by more
S_MARGIN = 1e-9                           # no s_xx, s_yy of a test row within this (relative) of 0, unless exactly 0

# tools/prosody_delta.py on gpu_cases(): the worst |delta| between the restatement and its four perturbed
# evaluations, per output; the GPU test allows the kernel BAR_FACTOR x that plus 2^-24 |ref|
DELTA_MEASURED = {"rho": 1.2213e-15, "shift_st": 5.3291e-15, "dev_st": 8.8818e-16, "voicing": 0.0}
BAR_FACTOR = 16.0

# tools/prosody_delta.py, the glide and the vibrato row of tests/contour_ref.py through the fp64 path (contour_ref.
# normalize, pitch_ref.yin, this module): {gamma: {figure: [glide, vibrato]}} without the envelope warp, and four
# times the worst distance of the path's fp32 variant from it (rho at gamma 1, dev_st at gamma 1 and 0: what the
# end-to-end tests assert; the variant ends, as the kernel does, with the outputs rounded to fp32)
E2E_MEASURED = {"1": {"rho": [0.9999777074993457, 0.9967057312959493],
                      "dev_st": [0.3266464429425289, 0.26979050293589596]},
                "0.5": {"rho": [0.9999338016063103, 0.9957780663783604],
                        "dev_st": [1.5091916736753435, 1.1100733483922396]},
                "0": {"rho": [-0.016951617699983147, 0.6224518595975408],
                      "dev_st": [2.671143502068598, 1.9657563612006834]}}
E2E_MARGIN = {"rho": 8.1632e-8, "dev_st": 2.5636e-7}


def walk(max_lag):
    """the lags in the order they are compared: 0, -1, +1, ..., -Lg, +Lg"""
    out = [0]
    for k in range(1, int(max_lag) + 1):
        out += [-k, k]
    return out


def _sum(v, dtype, reverse):
    """the sum of a vector: numpy's, or term by term from the far end"""
    v = np.asarray(v, dtype=dtype)
    if v.size == 0:
        return dtype(0.0)
    return np.cumsum(v[::-1], dtype=dtype)[-1] if reverse else v.sum(dtype=dtype)


def lag_terms(x, y, F, lag):
    """one row's tracks, the frames that count, a lag -> (x, y of the common frames in order, agree, overlap)"""
    t = np.arange(max(0, -lag), min(F, F - lag))
    if t.size == 0:
        return x[:0], y[:0], 0, 0
    xs, ys = x[t], y[t + lag]
    vx, vy = xs > 0, ys > 0
    both = vx & vy
    return xs[both], ys[both], int((vx == vy).sum()), int(t.size)


def compare(f0_ref, f0_deg, frames, max_lag=MAX_LAG, min_common=MIN_COMMON, reverse=False, longdouble=False,
            natural_log=False, ulp=False):
    """-> a namespace: rho, shift_st, dev_st, voicing fp64 [B], lag, common int32 [B], lags (per row a dict
    lag -> (n, s_xx, s_yy, sum x^2, sum y^2, rho or None when the lag is not valid))"""
    dt = np.longdouble if longdouble else np.float64
    f0_ref, f0_deg = np.asarray(f0_ref, dtype=np.float32), np.asarray(f0_deg, dtype=np.float32)
    B, T = f0_ref.shape
    out = types.SimpleNamespace(rho=np.zeros(B), shift_st=np.zeros(B), dev_st=np.zeros(B), voicing=np.zeros(B),
                                lag=np.zeros(B, np.int32), common=np.zeros(B, np.int32), lags=[])
    for b in range(B):
        F = min(max(int(frames[b]), 0), T)
        x, y = f0_ref[b].astype(dt), f0_deg[b].astype(dt)
        per, best = {}, None
        for lag in walk(max_lag):
            xs, ys, agree, overlap = lag_terms(x, y, F, lag)
            n = xs.size
            sxx = syy = sxy = dt(0.0)
            if n:
                dx, dy = xs - _sum(xs, dt, reverse) / dt(n), ys - _sum(ys, dt, reverse) / dt(n)
                sxx, syy, sxy = _sum(dx * dx, dt, reverse), _sum(dy * dy, dt, reverse), _sum(dx * dy, dt, reverse)
            valid = n >= min_common and sxx > 0 and syy > 0
            rho = sxy / np.sqrt(sxx * syy) if valid else None
            per[lag] = (n, float(sxx), float(syy), float((xs * xs).sum()), float((ys * ys).sum()),
                        None if rho is None else float(rho))
            if valid and (best is None or rho > best[1]):
                best = (lag, rho, xs, ys, agree, overlap)
        out.lags.append(per)
        if best is None:
            _, _, agree, overlap = lag_terms(x, y, F, 0)
            out.voicing[b] = agree / overlap if overlap else 0.0
            continue
        lag, rho, xs, ys, agree, overlap = best
        q = ys / xs
        e = dt(12.0) * (np.log(q) / np.log(dt(2.0)) if natural_log else np.log2(q))
        if ulp:                                             # every e moved by 2 ulp, the sign alternating
            step = np.where(np.arange(e.size) % 2 == 0, 2.0, -2.0).astype(dt)
            e = e + step * np.spacing(np.abs(e))
        n = dt(e.size)
        mean = _sum(e, dt, reverse) / n
        d = e - mean
        out.rho[b], out.lag[b], out.common[b] = float(rho), lag, e.size
        out.shift_st[b], out.dev_st[b] = float(mean), float(np.sqrt(_sum(d * d, dt, reverse) / n))
        out.voicing[b] = agree / overlap
    return out


PERTURBATIONS = {"reverse": dict(reverse=True), "longdouble": dict(longdouble=True),
                 "natural_log": dict(natural_log=True), "ulp": dict(ulp=True)}


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def contour_row(T, seed, base=150.0):
    """a contour that moves at several rates, so that neighbouring lags differ: fp64 [T], within 80..260 Hz"""
    t = np.arange(T, dtype=np.float64)
    g = np.random.default_rng(seed)
    ph = g.uniform(0.0, 2.0 * np.pi, 3)
    return (base + 28.0 * np.sin(2.0 * np.pi * t / 47.0 + ph[0]) + 14.0 * np.sin(2.0 * np.pi * t / 11.0 + ph[1])
            + 7.0 * np.sin(2.0 * np.pi * t / 4.3 + ph[2]) + 2.0 * g.standard_normal(T))


def shifted(row, lag, fill=0.0):
    """deg with deg[t + lag] = row[t]: delayed by lag frames (advanced when lag < 0), ``fill`` where nothing arrives"""
    T = row.shape[0]
    out = np.full(T, fill, dtype=np.float64)
    if lag >= 0:
        out[lag:] = row[:T - lag]
    else:
        out[:T + lag] = row[-lag:]
    return out


def gapped(T=61, seed=1):
    """the T = 61 row of the property tests: a moving contour with two unvoiced gaps"""
    row = contour_row(T, seed)
    row[10:14] = 0.0
    row[30:33] = 0.0
    return row


def period4(T=61):
    return np.array([100.0, 140.0, 120.0, 180.0])[np.arange(T) % 4]


def period8(T=61):
    """-> (ref, deg): a period-8 pattern and its own half-period shift, by indexing"""
    p = np.array([100.0, 150.0, 120.0, 180.0, 110.0, 160.0, 135.0, 170.0])
    t = np.arange(T)
    return p[t % 8], p[(t + 4) % 8]


_CASES = None


def gpu_cases():
    """the cases of the kernel test: [(name, f0_ref fp32 [B, T], f0_deg fp32 [B, T], frames int32 [B], max_lag,
    min_common)], built once and shared: treat them as read-only.

      rows      (3, 61), frames (61, 40, 0), Lg 8: a gapped contour against its delayed, scaled, noisy copy with a gap
                of its own; the same advanced by 2 with NaN and 300 Hz from frame 40 on; a row of which nothing counts
      one       (1, 1): one common frame, under min_common
      shrink    (1, 9), Lg 8: the overlap shrinks to one frame at lag +-8; only 0 and +-1 reach min_common
      wide      (2, 1030), Lg 32: every thread of a 1024-thread workgroup has a frame, some have two, all 65 lags are
                walked; the winners are -20 and +32, the last lag of the walk
      inverted  (1, 300), Lg 0: 300 - ref
      flat      (1, 61): a constant deg: s_yy is exactly 0 at every lag, nothing is scored
      tie4      (1, 61): a period-4 pattern against itself: exactly 1 at 0, +-4, +-8; 0 wins
      tie8      (1, 61): a period-8 pattern against its half-period shift: exactly 1 at -4 and +4; -4 wins"""
    global _CASES
    if _CASES is not None:
        return _CASES
    f = lambda *rows: np.stack(rows).astype(np.float32)
    g = np.random.default_rng(22)
    r0 = gapped()
    d0 = shifted(1.1 * r0, 3) + np.where(shifted(r0, 3) > 0, 1.5 * g.standard_normal(61), 0.0)
    d0[45:48] = 0.0
    r1 = gapped(seed=2)
    d1 = shifted(0.9 * r1, -2) + np.where(shifted(r1, -2) > 0, 1.5 * g.standard_normal(61), 0.0)
    r1[40:], d1[40:] = 300.0, 300.0
    r1[44:50], d1[50:55] = np.nan, np.nan
    r2 = gapped(seed=3)
    cases = [("rows", f(r0, r1, r2), f(d0, d1, 1.05 * r2), np.array([61, 40, 0], np.int32), 8, 8)]
    cases.append(("one", f([150.0]), f([160.0]), np.array([1], np.int32), 8, 8))
    r = contour_row(9, 4)
    cases.append(("shrink", f(r), f(shifted(r, 1, fill=140.0) + 1.0 * g.standard_normal(9)), np.array([9], np.int32),
                  8, 8))
    w0, w1 = contour_row(1030, 5), contour_row(1030, 6, base=200.0)
    w0[100:130], w1[500:520] = 0.0, 0.0
    e0 = shifted(1.2 * w0, -20) + np.where(shifted(w0, -20) > 0, 2.0 * g.standard_normal(1030), 0.0)
    e1 = shifted(0.8 * w1, 32) + np.where(shifted(w1, 32) > 0, 2.0 * g.standard_normal(1030), 0.0)
    e0[700:710] = 0.0
    cases.append(("wide", f(w0, w1), f(e0, e1), np.array([1030, 1030], np.int32), 32, 8))
    v = contour_row(300, 7)
    cases.append(("inverted", f(v), f(300.0 - v.astype(np.float32).astype(np.float64)), np.array([300], np.int32), 0,
                  8))
    cases.append(("flat", f(gapped(seed=8)), f(np.full(61, 150.0)), np.array([61], np.int32), 8, 8))
    cases.append(("tie4", f(period4()), f(period4()), np.array([61], np.int32), 8, 8))
    p, q = period8()
    cases.append(("tie8", f(p), f(q), np.array([61], np.int32), 8, 8))
    _CASES = cases
    return cases


TIE_CASES = {"tie4": (0, (-8, -4, 0, 4, 8)), "tie8": (-4, (-4, 4))}     # the winner, the lags at exactly 1.0
_REF_CACHE = {}


def case_ref(name):
    """the restatement of a case, computed once and shared: treat it as read-only"""
    if name not in _REF_CACHE:
        _, ref, deg, frames, Lg, m = next(c for c in gpu_cases() if c[0] == name)
        _REF_CACHE[name] = compare(ref, deg, frames, Lg, m)
    return _REF_CACHE[name]


def margins(res, skip=()):
    """a compare() namespace -> (the smallest lead of a row's winning rho over its other valid lags, ``skip`` left
    out; the smallest s_xx / sum x^2 or s_yy / sum y^2 that is not exactly 0, over the lags with n >= 2)"""
    lead, rel = math.inf, math.inf
    for b, per in enumerate(res.lags):
        for lag, (n, sxx, syy, xx, yy, rho) in per.items():
            if n >= 2:
                rel = min([rel] + [s / q for s, q in ((sxx, xx), (syy, yy)) if s != 0.0])
            if rho is not None and lag != int(res.lag[b]) and lag not in skip and int(res.common[b]) > 0:
                lead = min(lead, float(res.rho[b]) - rho)
    return lead, rel


def bar(output, ref_value):
    """the GPU test's allowance: 16 x the measured spread of the restatement plus the output's fp32 rounding"""
    return BAR_FACTOR * DELTA_MEASURED[output] + U * abs(ref_value)
