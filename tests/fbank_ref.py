"""fp64 restatement of the feature front end (csrc/sa_fbank.hip), written out as formulas.

The arbiter of tests/test_frontend_gpu.py: the Fbank kernel and the normalisation kernels are compared
with these functions per element.  Nothing here calls the package under test or torch.stft.  What the
kernels RECEIVE in fp32 -- the waveform, the periodic Hamming window, the speechbrain Mel matrix built in
fp32, the 1e-10 literals, the lengths -- is widened exactly; everything computed from there on is fp64.
tests/test_fbank_ref_cpu.py checks this module against oracle.features in fp64, the direct DFT, the
reference's normalizer pin and hand values, and shows that the GPU test's metrics and bars tell
deliberately wrong variants of these formulas from the right ones.

  frames         x[t*160 - 200 + i], i = 0..399, zero outside the waveform (center=True, pad_mode "constant")
  power          |sum_i frame[i] w[i] e^(-2 pi j k i / 400)|^2, k = 0..200, a direct DFT
  mel_energies   power @ fb[201, 80]                              T = 1 + N // 160
  raw_db         10 log10(max(M, 1e-10f))
  floors         max over the utterance (or over the batch) - 80
  norm_stats     n = round-half-even(fl32(len * T)) clipped to T; mean and unbiased std over the first n
                 frames, std floored at 1e-10f; both averaged over the batch
  norm_sequence  the running state [count, glob_mean, glob_std] through a list of calls

n = 1: speechbrain takes torch.std of one frame, which is NaN, and the NaN poisons glob_std for good.  The
kernel gives such an utterance the floor 1e-10 instead (variance 0), and this restatement follows the
kernel.  n = 0 is NaN on both sides (mean of nothing) and is not covered.
"""
import math

import numpy as np
import torch

N_FFT, HOP, NBIN, NMEL = 400, 160, 201, 80
TILE = 32                                   # frames per workgroup of sa_fbank_kernel
CHUNKS = 16                                 # frame chunks per utterance of sa_fbank_utt_partial_kernel
TOP_DB = 80.0
AMIN = float(np.float32(1e-10))             # the kernels' 1e-10f, widened
DB = 10.0 / math.log(10.0)                  # dB per unit of relative error


def _t(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.detach().cpu().double()


# ---------------------------------------------------------------------------------------------
def window():
    """periodic Hamming 0.54 - 0.46 cos(2 pi i / 400), rounded to fp32 as the kernel's table, widened"""
    i = np.arange(N_FFT, dtype=np.float64)
    return torch.from_numpy((0.54 - 0.46 * np.cos(2.0 * np.pi * i / N_FFT)).astype(np.float32)).double()


def mel_matrix32(n_mels=NMEL, n_fft=N_FFT, sample_rate=16000):
    """speechbrain's triangular Filterbank [201, 80] (HTK mel scale, centre +- the left mel spacing) in
    fp32, in the published operation order: the matrix the kernel's two bf16 planes are split from"""
    to_mel = lambda hz: 2595.0 * math.log10(1.0 + hz / 700.0)
    mel = torch.linspace(to_mel(0.0), to_mel(sample_rate / 2), n_mels + 2)
    hz = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    band = (hz[1:] - hz[:-1])[:-1]
    centre = hz[1:-1]
    n_stft = n_fft // 2 + 1
    freqs = torch.linspace(0, sample_rate // 2, n_stft)
    slope = (freqs[None, :] - centre[:, None]) / band[:, None]
    fb = torch.max(torch.zeros(1), torch.min(slope + 1.0, -slope + 1.0))
    return fb.t().contiguous()


def mel_matrix():
    return mel_matrix32().double()


def frames(wav):
    """[B, N] -> [B, T, 400]: frame t holds samples t*160 - 200 .. t*160 + 199, zeros outside 0..N-1"""
    w = _t(wav)
    B, N = w.shape
    T = 1 + N // HOP
    idx = (torch.arange(T) * HOP - N_FFT // 2)[:, None] + torch.arange(N_FFT)[None, :]
    inside = (idx >= 0) & (idx < N)
    return torch.where(inside[None], w[:, idx.clamp(0, N - 1)], torch.zeros((), dtype=torch.float64))


_DFT = None


def dft_tables():
    """cos, sin(2 pi k i / 400) as [400, 201]; the angle is reduced exactly (k i mod 400) first"""
    global _DFT
    if _DFT is None:
        ki = (torch.arange(N_FFT)[:, None] * torch.arange(NBIN)[None, :]) % N_FFT
        ang = 2.0 * math.pi * ki.double() / N_FFT
        _DFT = torch.cos(ang), torch.sin(ang)
    return _DFT


def power(windowed):
    """windowed frames [B, T, 400] -> power spectrum [B, T, 201]"""
    c, s = dft_tables()
    x = _t(windowed)
    return (x @ c) ** 2 + (x @ s) ** 2


def mel_energies(wav):
    """[B, N] waveform -> Mel energies [B, 1 + N // 160, 80], before the 1e-10 clamp"""
    return power(frames(wav) * window()) @ mel_matrix()


def raw_db(M):
    return 10.0 * torch.log10(_t(M).clamp(min=AMIN))


def floors(raw, mode):
    """[B]: the utterance's (mode "utterance") or the batch's (mode "batch") largest value, minus 80"""
    raw = _t(raw)
    if mode == "utterance":
        return raw.amax(dim=(1, 2)) - TOP_DB
    assert mode == "batch"
    return (raw.max() - TOP_DB).expand(raw.shape[0]).clone()


def clamped(raw, mode):
    raw = _t(raw)
    return torch.maximum(raw, floors(raw, mode)[:, None, None])


# ---------------------------------------------------------------------------------------------
def frame_counts(lens, T):
    """n[b] = round-half-even of the fp32 product len * T, clipped to T"""
    prod = np.asarray(lens, dtype=np.float32) * np.float32(T)           # rounded to fp32 as the kernel's
    return np.minimum(np.rint(prod.astype(np.float64)).astype(np.int64), T)


def norm_stats(x, lens):
    """x [B, T, 80], lens [B] -> (mean [80], std [80]): per utterance over its first n frames (std
    unbiased, 0 at n = 1, floored at 1e-10f), then the plain mean over the batch"""
    x = _t(x)
    B, T, _ = x.shape
    means, stds = [], []
    for b, n in enumerate(frame_counts(lens, T)):
        v = x[b, :int(n)]
        m = v.sum(0) / int(n)
        var = ((v - m) ** 2).sum(0) / (int(n) - 1) if n > 1 else torch.zeros_like(m)
        means.append(m)
        stds.append(torch.sqrt(var).clamp(min=AMIN))
    return torch.stack(means).sum(0) / B, torch.stack(stds).sum(0) / B


def norm_sequence(xs, lens, calls, update_until_epoch=4, state=None, pad_multiple=36, stats=norm_stats):
    """The running normaliser through ``calls`` = [(training, epoch), ...]; call i sees xs[i % len(xs)].
    state: None (fresh: count 0) or (count, glob_mean [80], glob_std [80]).
      training, count == 0           : glob = the batch statistics
      training, epoch < until        : glob = (1 - w) glob + w batch,  w = 1 / (count + 1)
      training, epoch >= until       : glob unchanged
      training                       : count += 1            eval: nothing changes
      out = (x - glob_mean) / glob_std, zero rows appended up to the next multiple of pad_multiple
    -> [(out [B, Tp, 80], count, glob_mean, glob_std)] after each call."""
    count, gm, gs = (0, None, None) if state is None else (int(state[0]), _t(state[1]), _t(state[2]))
    res = []
    for i, (training, epoch) in enumerate(calls):
        x = _t(xs[i % len(xs)])
        cm, cs = stats(x, lens)
        if training:
            if count == 0:
                gm, gs = cm, cs
            elif epoch < update_until_epoch:
                w = 1.0 / (count + 1)
                gm, gs = (1.0 - w) * gm + w * cm, (1.0 - w) * gs + w * cs
            count += 1
        B, T, F = x.shape
        Tp = T if not pad_multiple or T % pad_multiple == 0 else T + pad_multiple - T % pad_multiple
        out = torch.zeros(B, Tp, F, dtype=torch.float64)
        out[:, :T] = (x - gm) / gs
        res.append((out, count, gm.clone(), gs.clone()))
    return res


# ---------------------------------------------------------------------------------------------
# metrics of the GPU test (and of tools/fbank_delta.py, and of the sensitivity test)
def mel_error(raw_got, M_ref):
    """Per element e = |max(M_got, 1e-10) - max(M_ref, 1e-10)| / (max(M_ref, 1e-10) + 2^-20 Fmax), M_got =
    10^(raw / 10) from dB features, Fmax the frame's largest reference energy: the spectrum's error scales
    with the frame's energy, not the bin's, and the clamp on both sides makes a flip across 1e-10 harmless."""
    Mg = (10.0 ** (_t(raw_got) / 10.0)).clamp(min=AMIN)
    Mr = _t(M_ref)
    return (Mg - Mr.clamp(min=AMIN)).abs() / (Mr.clamp(min=AMIN) + 2.0 ** -20 * Mr.amax(dim=2, keepdim=True))


def floor_bound(bar):
    """dB: the largest element is the largest of its own frame, so its denominator is M (1 + 2^-20)"""
    return DB * bar * (1.0 + 2.0 ** -20)


def norm_errors(out, gm, gs, x, ref):
    """(mean, std, output) errors against ref = (out_64, count, gm_64, gs_64), each a plain number:
         max |gm - gm_64| / (|gm_64| + gs_64),  max |gs - gs_64| / gs_64,
         max |out - out_64| gs_64 / (|x| + |gm_64| + gs_64)   over the T real frames"""
    out64, _, gm64, gs64 = ref
    x = _t(x)
    T = x.shape[1]
    em = ((_t(gm) - gm64).abs() / (gm64.abs() + gs64)).max()
    es = ((_t(gs) - gs64).abs() / gs64).max()
    eo = ((_t(out)[:, :T] - out64[:, :T]).abs() * gs64 / (x.abs() + gm64.abs() + gs64)).max()
    return float(em), float(es), float(eo)


# ---------------------------------------------------------------------------------------------
# the cases of the GPU test
FBANK_N = (1, 159, 160, 161, 399, 400, 401, 4960, 5119, 5120, 10239, 10240, 11360)
SIGNALS = ("synthetic", "silence_tail", "tone_on_bin", "tone_off_bin", "dc", "impulse", "scaled_1e-5",
           "scaled_1e-6", "loud_then_quiet")


def _synthetic(B, N, seed):
    """oracle.features.synthetic_wave restated: 0.1 randn + 220 / 1000 / 3400 Hz, clipped to [-1, 1]"""
    rs = np.random.RandomState(seed)
    t = np.arange(N, dtype=np.float64) / 16000.0
    w = 0.1 * rs.standard_normal((B, N))
    for f, a in ((220.0, 0.2), (1000.0, 0.1), (3400.0, 0.05)):
        w = w + a * np.sin(2 * np.pi * f * t)[None, :]
    return np.clip(w, -1.0, 1.0)


def signal_rows(N):
    """[9, N] fp32, one row per entry of SIGNALS"""
    t = np.arange(N, dtype=np.float64) / 16000.0
    syn = _synthetic(1, N, 8886)[0]
    tail = syn.copy()
    tail[N - N // 3:] = 0.0                                         # digital silence
    imp = np.zeros(N)
    imp[N // 2] = 1.0
    loud = syn.copy()
    loud[N // 2:] *= 1e-5
    rows = [syn, tail, np.sin(2 * np.pi * 1000.0 * t), 0.9 * np.sin(2 * np.pi * 1017.3 * t), np.full(N, 0.5), imp,
            syn * 1e-5, syn * 1e-6, loud]
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def zero_middle(N):
    """[3, N] fp32: synthetic rows with an all-zero row between them"""
    w = _synthetic(3, N, 77)
    w[1] = 0.0
    w[2] *= 0.25
    return torch.from_numpy(w.astype(np.float32))


_CASES = None


def gpu_cases():
    """{name: waveform fp32 [B, N]}: for every N of FBANK_N the nine signals as one batch ("rows-N") and the
    B = 3 batch with the all-zero middle row ("zero-N").  Built once and shared: treat as read-only."""
    global _CASES
    if _CASES is None:
        _CASES = {}
        for N in FBANK_N:
            _CASES[f"rows-{N}"] = signal_rows(N)
            _CASES[f"zero-{N}"] = zero_middle(N)
    return _CASES


_REF = {}


def case_ref(name):
    """Mel energies [B, T, 80] of a case by the restatement, computed once and shared: read-only"""
    if name not in _REF:
        _REF[name] = mel_energies(gpu_cases()[name])
    return _REF[name]


# ---- normalisation ---------------------------------------------------------------------------
CALLS = ((True, 1), (True, 1), (True, 5), (False, 1))       # first, running, frozen (until = 4), eval
LOAD_CALL = ((True, 1),)                                    # after load_state_dict of loaded_state()
UNTIL = 4


def loaded_state():
    g = torch.Generator().manual_seed(3)
    return 5, -30.0 + torch.randn(80, generator=g), 8.0 + torch.rand(80, generator=g)


def _feats(B, T, seed, kind="normal"):
    g = torch.Generator().manual_seed(seed)
    if kind == "offset":                                     # cancellation in sq - s * m
        return -80.0 + 0.05 * torch.randn(B, T, 80, generator=g)
    return -30.0 + 12.0 * torch.randn(B, T, 80, generator=g)


def _lens(B, head, seed):
    """head, then lengths in [0.3, 1] for the remaining rows"""
    g = torch.Generator().manual_seed(seed)
    rest = 0.3 + 0.7 * torch.rand(B, generator=g)
    return torch.cat([torch.tensor(head, dtype=torch.float32), rest[len(head):]])[:B]


_NORM = None


def norm_cases():
    """{name: (xs, lens)}: xs two fp32 [B, T, 80] tensors that successive calls alternate between, lens fp32
    [B].  Every B of {1, 2, 3, 8, 9, 17, 32} and every T of {2, 15, 16, 17, 33, 72, 73, 75} occurs.
      T = 16 is the one T of the list at which chunk 15 holds a frame (16 chunks of ceil(T / 16) frames);
      T = 1001 (one row) is the long row: chunk 15 holds 56 frames there."""
    global _NORM
    if _NORM is not None:
        return _NORM
    c = {}

    def add(name, B, T, head, kind="normal", edit=None):
        xs = [_feats(B, T, 100 * B + T + k, kind) for k in (0, 1)]
        if edit:
            for x in xs:
                edit(x)
        c[name] = (xs, _lens(B, head, B + T))

    add("B1-T2-n2", 1, 2, [1.0])                                        # n = 2: one degree of freedom
    add("B2-T15-n1", 2, 15, [1.0, 0.07])                                # 0.07 * 15 = 1.05 -> n = 1
    add("B3-T16-n2", 3, 16, [1.0, 0.5, 0.125])                          # n = 16 (chunk 15), 8, 2
    add("B8-T17-tie", 8, 17, [0.5, 1.0, 1.04])                          # 8.5 -> 8; 17.68 -> 18, clipped to 17
    add("B9-T33-tie", 9, 33, [0.5, 1.0])                                # 16.5 -> 16
    add("B17-T72-quarter", 17, 72, [0.25, 1.0, 1.01])                   # n = 18: chunk 3 partial, 4..15 empty; 72.72 -> 72
    add("B32-T73-tie", 32, 73, [0.5, 1.0])                              # 36.5 -> 36
    add("B3-T75-tie", 3, 75, [0.5, 1.0, 0.9])                           # 37.5 -> 38
    add("B9-T72-offset", 9, 72, [1.0, 0.61], kind="offset")
    add("B17-T33-offset", 17, 33, [1.0], kind="offset")
    add("B2-T17-constcol", 2, 17, [1.0, 0.8], edit=lambda x: x[:, :, 11].fill_(-30.25))
    add("B3-T33-constrow", 3, 33, [1.0, 1.0, 0.7], edit=lambda x: x[1].fill_(-30.25))
    add("B32-T16-full", 32, 16, [1.0] * 32)
    add("B1-T1001-long", 1, 1001, [1.0])
    _NORM = c
    return c


_NORM_REF = {}


def norm_case_ref(name):
    """(results of CALLS from a fresh state, results of LOAD_CALL from loaded_state()): computed once, read-only"""
    if name not in _NORM_REF:
        xs, lens = norm_cases()[name]
        _NORM_REF[name] = (norm_sequence(xs, lens, CALLS, UNTIL), norm_sequence(xs, lens, LOAD_CALL, UNTIL, loaded_state()))
    return _NORM_REF[name]
