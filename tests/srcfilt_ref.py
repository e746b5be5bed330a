"""Integer / fp64 restatement of the LPC source-filter resynthesis (include/sa_hip.h carries the
definition; speech_anonymization_amd.sourcefilter and csrc/sa_srcfilt.hip), on the CPU with numpy.  The pulse table is
integer arithmetic on one correctly rounded fp64 quotient per frame, the noise is uint32 arithmetic, and the excitation
is ``np.float32`` operations rounded one by one: all three are compared with the kernels bit for bit.  The synthesis
reuses tests/mcadams_ref.py's framing, ``autocorr``, ``levinson`` and level code; it has a rounding bar, whose constant C
tools/srcfilt_delta.py measures on this file by re-running it with the lag sums and the excitation energy summed from
the far end and the filter's taps accumulated in the opposite order.  Shared by tests/test_srcfilt_cpu.py,
tests/test_srcfilt_gpu.py and tools/srcfilt_delta.py."""
import json
import math
import os
import types

import numpy as np

from tests import mcadams_ref as M

W, H, P, SR = M.W, M.H, M.P, M.SR
U = M.U
ONE = 1 << 16
TMIN, TMAX = 40, 266
KDIV = 40
NO_EXC = 1e-20
OK, SILENT, FALLBACK, UNEXCITED = 0, 1, 2, 3
NEAR_FLOOR = 1e-6                        # r_0 or Ee within 1 +- this of its floor: near a decision
NEAR_K = M.NEAR_K
C_FACTOR = 16.0
SEED_MASK = 0x7fffffff
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA_FILE = os.path.join(ROOT, "profiles", "srcfilt_delta.json")


def frames_of_track(N, padded=False):
    """the two frame counts the entry points take: N // 160 + 1, or ceil(N / 160) + 1 of the padded waveform"""
    return (-(-int(N) // H) if padded else int(N) // H) + 1


def kcap(N):
    return int(N) // KDIV + 2


def frame(n, T):
    return min((n + H // 2) // H, T - 1)


def voiced(f0):
    """[...] bool of the fp32 values: 0 < f0 < inf (a NaN is unvoiced)"""
    f = np.asarray(f0, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (f > 0) & (f < np.inf)


def periods(f0, rho_q=None):
    """f0 [T] fp32, rho_q [T] int or None -> P_q [T] int64 in units of 2^-16 samples, 0 where unvoiced"""
    f = np.asarray(f0, dtype=np.float32)
    rho = np.full(f.shape, ONE, np.int64) if rho_q is None else np.clip(np.asarray(rho_q, np.int64), ONE // 2, 2 * ONE)
    v = voiced(f)
    den = np.where(v, f.astype(np.float64) * rho.astype(np.float64), 1.0)          # exact: 24 by 18 bits
    with np.errstate(over="ignore"):
        q = np.rint(np.float64(16000.0 * 2.0 ** 32) / den)                         # one rounding, then half to even
    q = np.clip(q, float(TMIN * ONE), float(TMAX * ONE))
    return np.where(v, q.astype(np.int64), 0)


def pulses_row(f0, rho_q, n_valid, N):
    """one row -> (pos_q list, period_q list): the walk of the definition, in Python integers"""
    T = len(f0)
    nv = min(max(int(n_valid), 0), int(N))
    pq = periods(f0, rho_q)
    pos, per = [], []
    s = 0
    while (s >> 16) < nv:
        t = frame(s >> 16, T)
        if pq[t] > 0:
            pos.append(s)
            per.append(int(pq[t]))
            s += int(pq[t])
        elif t == T - 1:
            break
        else:
            s = (H * t + H // 2) << 16
    return pos, per


def pulses(f0, rho_q, n_valid, N):
    """f0 [B, T] fp32, rho_q [B, T] or None, n_valid [B] -> (pos_q int64 [B, Kcap], period_q int32 [B, Kcap], count
    int32 [B]); entries past a row's count are -1 here and mean nothing in the kernel's tables"""
    f0 = np.asarray(f0, dtype=np.float32)
    B = f0.shape[0]
    K = kcap(N)
    pos_q = np.full((B, K), -1, np.int64)
    period_q = np.full((B, K), -1, np.int32)
    count = np.zeros(B, np.int32)
    for b in range(B):
        pos, per = pulses_row(f0[b], None if rho_q is None else np.asarray(rho_q)[b], n_valid[b], N)
        assert len(pos) <= K - 1, (len(pos), K)
        count[b] = len(pos)
        pos_q[b, :len(pos)] = pos
        period_q[b, :len(per)] = per
    return pos_q, period_q, count


def mix(x):
    """the 32-bit finaliser of the definition on uint32 values held in uint64 (so that no product wraps early)"""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    return x


def noise(seed, N):
    """u_n fp32 [N] in [-1, 1), exact: ((h >> 8) - 2^23) 2^-23 with h = mix(n ^ mix(uint32(seed)))"""
    k = mix(np.uint64(int(seed) & 0xffffffff))
    h = mix(np.arange(N, dtype=np.uint64) ^ k)
    return ((h >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -23)


def draw_seeds(seed, drawn, B):
    """the noise seeds SourceFilter(seed=seed) hands to the B utterances after ``drawn`` earlier ones: int32 [B],
    mix((drawn + b) ^ mix(seed)) with the top bit cleared"""
    k = mix(np.uint64(int(seed) & 0xffffffff))
    return (mix(np.arange(drawn, drawn + B, dtype=np.uint64) ^ k) & np.uint64(SEED_MASK)).astype(np.int32)


def excite(f0, pos_q, period_q, count, seed, n_valid, N, aspiration):
    """-> exc fp32 [B, N]: every operation an ``np.float32`` one, rounded on its own"""
    f0 = np.asarray(f0, dtype=np.float32)
    B, T = f0.shape
    exc = np.zeros((B, N), np.float32)
    fr = np.minimum((np.arange(N) + H // 2) // H, T - 1)
    one = np.float32(1.0)
    for b in range(B):
        nv = min(max(int(n_valid[b]), 0), N)
        c = np.where(voiced(f0[b])[fr], np.float32(aspiration), one).astype(np.float32)
        e = (c * noise(seed[b], N)).astype(np.float32)
        for k in range(int(count[b])):
            s = int(pos_q[b, k])
            n, frac = s >> 16, s & (ONE - 1)
            A = np.float32(math.sqrt(float(int(period_q[b, k])) * 2.0 ** -16))
            phi = np.float32(frac) * np.float32(2.0 ** -16)
            if n < nv:
                e[n] = np.float32(e[n] + np.float32(A * np.float32(one - phi)))
            if frac > 0 and n + 1 < nv:
                e[n + 1] = np.float32(e[n + 1] + np.float32(A * phi))
        exc[b, :nv] = e[:nv]
    return exc


def iir(a, x, reverse_taps=False):
    """rec[j] = x[j] - sum_k a[k] rec[j - k] from zero history; the taps k = 1..20 in order (``reverse_taps``: from 20
    down)"""
    rec = np.zeros(W + P)
    order = range(P, 0, -1) if reverse_taps else range(1, P + 1)
    for j in range(W):
        s = x[j]
        for k in order:
            s -= a[k] * rec[P + j - k]
        rec[P + j] = s
    return rec[P:]


def ordered_sum(v, reverse=False):
    s = 0.0
    for x in (v[::-1] if reverse else v):
        s += x
    return s


def synth_frame(f, ex, reverse_acf=False, reverse_ee=False, reverse_taps=False):
    """one windowed frame and its windowed excitation -> (rec [320], status, near a decision?)"""
    r = M.autocorr(f, reverse_acf)
    near = abs(r[0] / M.SILENCE - 1.0) <= NEAR_FLOOR
    if r[0] < M.SILENCE:
        return f.copy(), SILENT, near
    r[0] *= 1.0 + M.R0_LIFT
    a, ks, ok = M.levinson(r)
    near = near or bool((np.abs(np.abs(ks) - 1.0) <= NEAR_K).any())
    if not ok:
        return f.copy(), FALLBACK, near
    E = r[0]
    for k in ks:
        E *= 1.0 - k * k
    Ee = ordered_sum(ex * ex, reverse_ee)
    near = near or abs(Ee / NO_EXC - 1.0) <= NEAR_FLOOR
    if Ee < NO_EXC:
        return np.zeros(W), UNEXCITED, near
    g = math.sqrt(E / Ee)
    return iir(a, g * ex, reverse_taps), OK, near


def synth(wav, exc, n_valid, level=True, reverse_acf=False, reverse_ee=False, reverse_taps=False):
    """wav, exc [B, N] (the fp32 values), n_valid [B] -> a namespace of fp64 arrays in tests/mcadams_ref.py's layout
    (so that its ``gain_bar`` applies): F [B, T, 320], Fa, Fb, y [B, N], gain [B], out [B, N], status [B, T], near
    [B, T], left_out [B, N], n_valid"""
    x = np.asarray(wav, dtype=np.float32).astype(np.float64)
    e = np.asarray(exc, dtype=np.float32).astype(np.float64)
    B, N = x.shape
    T = M.n_frames(N)
    nv = np.clip(np.asarray(n_valid, dtype=np.int64), 0, N)
    F = np.zeros((B, T, W))
    status = np.zeros((B, T), dtype=np.int32)
    near = np.zeros((B, T), dtype=bool)
    y, out, gain = np.zeros((B, N)), np.zeros((B, N)), np.ones(B)
    n = np.arange(N)
    t0 = n // H
    for b in range(B):
        live = n < nv[b]
        fr, er = M.frames_of(x[b], nv[b]), M.frames_of(e[b], nv[b])
        for t in range(T):
            rec, status[b, t], near[b, t] = synth_frame(fr[t], er[t], reverse_acf, reverse_ee, reverse_taps)
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
    return types.SimpleNamespace(x=x, n_valid=nv, F=F, Fa=Fa, Fb=Fb, y=y, gain=gain, out=out, status=status, near=near,
                                 left_out=left_out)


def srcfilt(wav, f0, rho_q, seed, n_valid, aspiration=0.3, level=True, **perturb):
    """the three steps in a row -> (the namespace of ``synth`` with pos_q, period_q, count and exc added)"""
    N = np.asarray(wav).shape[1]
    pos_q, period_q, count = pulses(f0, rho_q, n_valid, N)
    exc = excite(f0, pos_q, period_q, count, seed, n_valid, N, aspiration)
    ref = synth(wav, exc, n_valid, level, **perturb)
    ref.pos_q, ref.period_q, ref.count, ref.exc = pos_q, period_q, count, exc
    return ref


# ---- the kernel tests' inputs ---------------------------------------------------------------------------
FORMANTS = M.FORMANTS
TARGET_HZ = 170.0


def waves():
    """{name: (wav fp32 [B, N], n_valid int32 [B], the nominal F0 of every row)}: N = 1687 is no multiple of the hop and
    its third row ends at 1000; N = 50 has two synthesis frames; the first row of the third case has no valid sample;
    the last is 4800 samples, 19 tiles of the excitation kernel and two chunks of the level sums"""
    v = M.voiced_row
    return {
        "odd": (np.stack([v(120.0, FORMANTS, 1687, 0), v(210.0, FORMANTS, 1687, 1),
                          v(160.0, FORMANTS, 1687, 2)]).astype(np.float32),
                np.array([1687, 1687, 1000], np.int32), (120.0, 210.0, 160.0)),
        "two_frames": (v(200.0, FORMANTS, 50, 3)[None].astype(np.float32), np.array([50], np.int32), (200.0,)),
        "empty_row": (np.stack([v(140.0, FORMANTS, 1600, 4), v(180.0, FORMANTS, 1600, 5)]).astype(np.float32),
                      np.array([0, 1600], np.int32), (140.0, 180.0)),
        "long": (v(160.0, FORMANTS, 4800, 6)[None].astype(np.float32), np.array([4800], np.int32), (160.0,)),
    }


_YIN = {}


def yin_track(name, T):
    """the fp32 track of tests/pitch_ref.py's YIN on a case's waveform, cut or padded with zeros to T frames"""
    if name not in _YIN:
        import torch
        from tests import pitch_ref as PR
        _YIN[name] = PR.yin(torch.as_tensor(waves()[name][0], dtype=torch.float64))[0].numpy().astype(np.float32)
    f0 = _YIN[name]
    out = np.zeros((f0.shape[0], T), np.float32)
    out[:, :min(T, f0.shape[1])] = f0[:, :T]
    return out


def track(name, T):
    """f0 fp32 [B, T] of a case: constant 120 Hz; 210 Hz with an unvoiced gap; 160 Hz with a NaN, -1, +inf, 30 Hz (the
    period clamped at 266) and 900 Hz (clamped at 40) entry, voiced from frame 6 on so that its last pulse falls at
    sample 900 and the frame over [960, 1280) keeps no pulse; constant 200 Hz; a voiced and an all-unvoiced row; the
    YIN track of the row itself"""
    wav, nv, nominal = waves()[name]
    f0 = np.tile(np.array(nominal, np.float32)[:, None], (1, T))
    if name == "odd":
        f0[1, 4:6] = 0.0
        f0[2, 1:6] = np.array([np.nan, -1.0, np.inf, 30.0, 900.0], np.float32)
    elif name == "empty_row":
        f0[1] = 0.0
    elif name == "long":
        f0 = yin_track(name, T)
    return f0


def rho_variants(name, T):
    """{label: rho_q int32 [B, T] or None}: NULL; one ratio per utterance that brings its nominal F0 to 170 Hz; per-frame
    values that hold 1 and 2^30 (clamped to 2^15 and 2^17 where they are read)"""
    nominal = np.array(waves()[name][2])
    to_target = np.tile(np.rint(TARGET_HZ / nominal * ONE).astype(np.int32)[:, None], (1, T))
    wild = to_target.copy()
    wild[:, 0::3] = 1
    wild[:, 1::3] = 1 << 30
    return {"null": None, "to_170": to_target, "clamped": wild}


CASE_SEEDS = {"odd": (11, -5, 2 ** 31 - 1), "two_frames": (0,), "empty_row": (7, 8), "long": (1986,)}
# the cases of the synthesis test: (case, aspiration).  With aspiration 0 the frame of "odd" row 2 over [960, 1280) has
# neither noise nor a pulse: status 3
SYNTH_CASES = (("odd", 0.3), ("odd", 0.0), ("two_frames", 0.3), ("empty_row", 0.3), ("long", 0.3))

_REF_CACHE = {}


def case_inputs(name, padded=False):
    wav, nv, _ = waves()[name]
    N = wav.shape[1]
    return wav, nv, track(name, frames_of_track(N, padded)), np.array(CASE_SEEDS[name], np.int32)


def case_ref(name, aspiration, **perturb):
    """the restatement of a synthesis case (rho_q NULL, level on), computed once per key and shared: read-only"""
    key = (name, float(aspiration), tuple(sorted(perturb.items())))
    if key not in _REF_CACHE:
        wav, nv, f0, seed = case_inputs(name)
        _REF_CACHE[key] = srcfilt(wav, f0, None, seed, nv, aspiration, True, **perturb)
    return _REF_CACHE[key]


PERTURBATIONS = ({"reverse_acf": True}, {"reverse_ee": True}, {"reverse_taps": True})


def measure_c():
    """the worst |delta| / max|y| of the three perturbed evaluations against the plain one over SYNTH_CASES, per
    perturbation -> {name: value}"""
    worst = {}
    for p in PERTURBATIONS:
        label = next(iter(p))
        w = 0.0
        for name, asp in SYNTH_CASES:
            base, other = case_ref(name, asp), case_ref(name, asp, **p)
            assert (base.status == other.status).all()
            for b in range(base.y.shape[0]):
                top = np.abs(base.y[b]).max()
                if top > 0:
                    w = max(w, float(np.abs(other.y[b] - base.y[b]).max() / top))
        worst[label] = w
    return worst


# ---- end to end -----------------------------------------------------------------------------------------
E2E_PEAK_HZ = 1220.0
E2E_SEED = 1


def e2e_rows():
    """the three 4800-sample resonance rows (tests/lpcformant_ref.py's: 120, 210 and 160 Hz), fp32 [3, 4800]"""
    from tests import lpcformant_ref
    return lpcformant_ref.e2e_rows()


def e2e_measure(wav, out, target_hz):
    """(|voiced-mean F0 of out / want - 1| per row, |envelope peak near 1220 Hz of out - that of wav| in Hz per row);
    want: target_hz, or with None the voiced-mean F0 of wav itself"""
    from tests import formant_ref as FR
    f_in, f_out = FR.voiced_f0(np.asarray(wav))[0].numpy(), FR.voiced_f0(np.asarray(out))[0].numpy()
    want = f_in if target_hz is None else np.full_like(f_in, target_hz)
    near = np.full(len(f_in), E2E_PEAK_HZ)
    p_in = M.envelope_peak_near(np.asarray(wav, np.float64), near)
    p_out = M.envelope_peak_near(np.asarray(out, np.float64), near)
    return np.abs(f_out / want - 1.0), np.abs(p_out - p_in), f_out, p_in, p_out


def e2e_restatement(target_hz, aspiration=0.3):
    """SourceFilter(target_hz, aspiration, seed=1) on the three rows, restated: tests/pitch_ref.py's YIN track and ratio,
    rho_q = rint(ratio 2^16), the first draw of seeds -> (wav, out fp64 [3, 4800])"""
    import torch
    from tests import pitch_ref as PR
    wav = e2e_rows()
    B, N = wav.shape
    f0 = PR.yin(torch.as_tensor(wav, dtype=torch.float64))[0]
    rho_q = None
    if target_hz is not None:
        r = PR.ratio(f0.float().double(), torch.ones(B), N, target_hz)[0]
        rho_q = np.tile(np.rint(r.float().double().numpy() * ONE).astype(np.int32)[:, None], (1, f0.shape[1]))
    ref = srcfilt(wav, f0.numpy().astype(np.float32), rho_q, draw_seeds(E2E_SEED, 0, B), np.full(B, N, np.int32),
                  aspiration, True)
    return wav, ref.out


def load_delta():
    with open(DELTA_FILE) as f:
        return json.load(f)
