"""Waveform augmentation of the gender-classifier recipes: the reference's ``env_corrupt``
(additive noise, clean and noisy batch concatenated) and ``TimeDomainSpecAugment`` (speed perturbation, frequency
drop, chunk drop) restated from speechbrain 0.5.x processing/speech_augmentation.py -- parity unpinned -- and run
as three launches of csrc/sa_augment.hip per step.  OpenRIR noise and reverberation are not built: the noise is
white, drawn on the device; the kernels take it as a tensor.

Every other draw is made on the host from a ``torch.Generator`` the module owns and travels to the device as one
PLAN: the resampling table, the composed 101-tap filter, the per-row chunk intervals and the per-utterance SNR, in
one buffer of 32-bit words copied asynchronously from pinned memory.  Tables and taps are computed in fp64 and
rounded once.  Nothing here reads device memory or synchronises.

Plan words: first [S_out] int | w [S_out][W] float | h [101] float | chunks [R][1 + 2 MAX_CHUNKS] int (count,
then start, end pairs, end exclusive) | snr [B] float.
"""
import functools
import math
import types

import torch

from . import _lib as L

TAPS = 101
HALO = TAPS // 2
MAX_ROWS = 65535          # rows of the augmented batch: a grid extent of the kernels that take it
_TILE = _MAXC = None

DEFAULTS = dict(sample_rate=16000, speeds=(95, 100, 105), noise=True, snr_low=0.0, snr_high=15.0,
                drop_freq_low=1e-14, drop_freq_high=1.0, drop_freq_count_low=0, drop_freq_count_high=3,
                drop_freq_width=0.05, drop_chunk_count_low=0, drop_chunk_count_high=5,
                drop_chunk_length_low=1000, drop_chunk_length_high=2000)


def tile():
    """output samples per workgroup of sa_wav_augment (the library's constant)"""
    global _TILE
    if _TILE is None:
        _TILE = L.load().sa_wav_augment_tile()
    return _TILE


def max_chunks():
    """dropped intervals per row that a plan can carry (the library's constant)"""
    global _MAXC
    if _MAXC is None:
        _MAXC = L.load().sa_wav_augment_max_chunks()
    return _MAXC


def __getattr__(name):                  # augment.TILE / augment.MAX_CHUNKS: read from the library on first use
    if name == "TILE":
        return tile()
    if name == "MAX_CHUNKS":
        return max_chunks()
    raise AttributeError(name)


def settings(cfg=None, **over):
    """DEFAULTS overlaid with a mapping (the YAML block) or an object's attributes, then keywords"""
    out = dict(DEFAULTS)
    if cfg is not None:
        src = cfg if isinstance(cfg, dict) else vars(cfg)
        unknown = [k for k in src if k not in DEFAULTS]
        if unknown:
            raise ValueError(f"unknown augmentation setting {unknown[0]!r}")
        out.update(src)
    out.update(over)
    out["speeds"] = tuple(int(s) for s in out["speeds"])
    return types.SimpleNamespace(**out)


# ---- the tables (fp64) ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resample_table(orig_freq, new_freq, width=6):
    """Kaldi-style windowed-sinc resampling orig_freq -> new_freq: (S_in, S_out, W, first [S_out] int64,
    w [S_out, W] fp64).  Output q S_out + i = sum_j w[i][j] x[q S_in + first[i] + j].  Cached: do not write to them."""
    if new_freq == orig_freq:
        return 1, 1, 1, torch.zeros(1, dtype=torch.int64), torch.ones(1, 1, dtype=torch.float64)
    g = math.gcd(orig_freq, new_freq)
    s_in, s_out = orig_freq // g, new_freq // g
    cutoff = 0.99 * 0.5 * min(orig_freq, new_freq)
    ww = width / (2 * cutoff)
    t = torch.arange(s_out, dtype=torch.float64) / new_freq
    first = torch.ceil((t - ww) * orig_freq)
    last = torch.floor((t + ww) * orig_freq)
    W = int((last - first + 1).max())
    d = (first[:, None] + torch.arange(W, dtype=torch.float64)) / orig_freq - t[:, None]
    win = torch.where(d.abs() < ww, 0.5 * (1 + torch.cos(2 * math.pi * cutoff / width * d)), torch.zeros_like(d))
    safe = torch.where(d == 0, torch.ones_like(d), d)
    sinc = torch.where(d == 0, torch.full_like(d, 2 * cutoff), torch.sin(2 * math.pi * cutoff * safe) / (math.pi * safe))
    return s_in, s_out, W, first.long(), win * sinc / orig_freq


def resampled_length(n, orig_freq, new_freq):
    """samples the resampler gives for n input samples (speechbrain's Resample._output_samples)"""
    if new_freq == orig_freq:
        return n
    tick = orig_freq * new_freq // math.gcd(orig_freq, new_freq)
    interval = n * tick // orig_freq
    per = tick // new_freq
    out = interval // per
    if interval % per == 0:
        out -= 1
    return out + 1


def notch(f, width=0.05):
    """speechbrain's notch_filter(f, 101, width): low-pass at f plus high-pass at f + 2 width, fp64 [101]"""
    x = torch.arange(-HALO, HALO + 1, dtype=torch.float64)
    n = torch.arange(TAPS, dtype=torch.float64)
    bw = 0.42 - 0.5 * torch.cos(2 * math.pi * n / TAPS) + 0.08 * torch.cos(4 * math.pi * n / TAPS)

    def sinc(a):
        safe = torch.where(a == 0, torch.ones_like(a), a)
        return torch.where(a == 0, torch.ones_like(a), torch.sin(safe) / safe)

    lp = sinc(3 * f * x) * bw
    lp = lp / lp.sum()
    hp = sinc(3 * (f + 2 * width) * x) * bw
    hp = hp / -hp.sum()
    hp[HALO] += 1
    return lp + hp


def compose_taps(centres, width=0.05):
    """the delta at tap 50 convolved with notch(f) for every centre, each product cut back to 101 taps; fp64"""
    h = torch.zeros(TAPS, dtype=torch.float64)
    h[HALO] = 1.0
    for f in centres:
        g = notch(float(f), width)
        full = torch.nn.functional.conv1d(h.view(1, 1, -1), g.flip(0).view(1, 1, -1), padding=TAPS - 1).view(-1)
        h = full[HALO:HALO + TAPS].clone()
    return h


# ---- the plan ----------------------------------------------------------------------------------------------
class Plan:
    """one step's draws and tables.  B, L: the input batch; R, Lp: rows and width of the output; speed; S_in,
    S_out, W, first (int32 [S_out]), w (fp32 [S_out, W]); centres, h (fp32 [101]); snr (fp32 [B]; None without
    noise rows); chunks: R lists of (start, end), end = start + length, not clipped."""

    def words(self):
        """the plan buffer (int32, pinned where a GPU is present), laid out as the module docstring says"""
        mc = max_chunks()
        rows = []
        for r, iv in enumerate(self.chunks):
            if len(iv) > mc:
                raise L.SaHipError(f"a plan carries at most {mc} dropped chunks per row, row {r} has {len(iv)}")
            flat = [int(v) for se in iv for v in se]
            rows.append([len(iv)] + flat + [0] * (2 * mc - len(flat)))
        table = torch.tensor(rows, dtype=torch.int32)
        snr = self.snr if self.snr is not None else torch.zeros(self.B, dtype=torch.float32)
        parts = [self.first.to(torch.int32), self.w.reshape(-1).view(torch.int32), self.h.view(torch.int32),
                 table.reshape(-1), snr.to(torch.float32).view(torch.int32)]
        n = sum(p.numel() for p in parts)
        buf = torch.empty(n, dtype=torch.int32, pin_memory=torch.cuda.is_available())
        torch.cat(parts, out=buf)
        self.snr_offset = n - self.B
        return buf


def make_plan(B, L, speed=100, centres=(), chunks=None, snr=None, cfg=None):
    """a plan from given draws (tests build edge cases with it; draw_plan draws and calls it).  snr: [B] values
    -> noise rows (R = 2 B); None -> R = B.  chunks: R lists of (start, length)."""
    c = settings(cfg)
    p = Plan()
    p.B, p.L, p.speed = int(B), int(L), int(speed)
    p.R = 2 * p.B if snr is not None else p.B
    new = c.sample_rate * p.speed // 100
    p.S_in, p.S_out, p.W, first, w = resample_table(c.sample_rate, new)
    p.first, p.w = first.to(torch.int32), w.to(torch.float32)
    p.Lp = resampled_length(p.L, c.sample_rate, new)
    p.centres = [float(f) for f in centres]
    p.h = compose_taps(p.centres, c.drop_freq_width).to(torch.float32)
    p.snr = None if snr is None else torch.as_tensor(snr, dtype=torch.float32).reshape(p.B).clone()
    chunks = chunks if chunks is not None else [[] for _ in range(p.R)]
    if len(chunks) != p.R:
        raise ValueError(f"chunks: one list per output row ({p.R}), got {len(chunks)}")
    p.chunks = [[(int(s), int(s) + int(n)) for s, n in row] for row in chunks]
    return p


def draw_plan(gen, lens, L, cfg=None):
    """one step's plan from the host generator ``gen``; lens: the CPU relative lengths [B] the loader made.
    Draw order: speed index, notch count, centres, SNRs, then per output row chunk count, lengths, starts."""
    c = settings(cfg)
    lens = torch.as_tensor(lens, dtype=torch.float32, device="cpu")
    B = lens.numel()
    ri = lambda lo, hi, n=1: torch.randint(int(lo), int(hi) + 1, (n,), generator=gen)
    speed = c.speeds[int(ri(0, len(c.speeds) - 1))]
    count = int(ri(c.drop_freq_count_low, c.drop_freq_count_high))
    u = torch.rand(count, generator=gen, dtype=torch.float64)
    centres = (c.drop_freq_low + u * (c.drop_freq_high - c.drop_freq_low)).tolist()
    snr = None
    if c.noise:
        snr = (c.snr_low + torch.rand(B, generator=gen, dtype=torch.float64) * (c.snr_high - c.snr_low)).float()
    R = 2 * B if c.noise else B
    Lp = resampled_length(int(L), c.sample_rate, c.sample_rate * speed // 100)
    chunks = []
    for r in range(R):
        k = int(ri(c.drop_chunk_count_low, c.drop_chunk_count_high))
        if k == 0:
            chunks.append([])
            continue
        length = ri(c.drop_chunk_length_low, c.drop_chunk_length_high, k)
        len_r = int(float(lens[r % B]) * Lp)
        start = ri(0, max(0, len_r - int(length.max())), k)
        chunks.append(list(zip(start.tolist(), length.tolist())))
    return make_plan(B, L, speed, centres, chunks, snr, cfg)


# ---- launches --------------------------------------------------------------------------------------------------
def apply_plan(wavs, lens, plan, noise=None):
    """wavs [B, L] (device, fp32), lens [B] (device; read by the noise scales only) -> [R, Lp].  One asynchronous
    copy of the plan, then sa_wav_augment alone (R = B) or sa_wav_abs_sums, sa_noise_scales, sa_wav_augment."""
    from . import ops
    B, Lw = wavs.shape if wavs.dim() == 2 else (0, 0)
    if (B, Lw) != (plan.B, plan.L):
        raise L.SaHipError(f"the plan was drawn for a batch [{plan.B}, {plan.L}], got {tuple(wavs.shape)}")
    if plan.R > MAX_ROWS:
        raise L.SaHipError(f"augmentation: {plan.R} rows exceed the {MAX_ROWS} a launch takes")
    words = plan.words().to(wavs.device, non_blocking=True)
    scales = None
    if plan.R == 2 * plan.B:
        if noise is None:
            raise L.SaHipError("a plan with noise rows needs the noise tensor [B, L]")
        snr = words[plan.snr_offset:].view(torch.float32)
        scales = ops.noise_scales(ops.wav_abs_sums(wavs, noise), lens, snr, plan.L)
    else:
        noise = None
    return ops.wav_augment(wavs, noise, scales, words, plan.R, plan.Lp, plan.S_in, plan.S_out, plan.W,
                           int(plan.first.min()), int(plan.first.max()))


class TrainAugment(torch.nn.Module):
    """both augmentations fused: ``(wavs, lens) -> (wavs', lens', repeat)``, wavs' [repeat B, L'], lens'
    = lens repeated, repeat = 2 with noise rows (labels are repeated by the caller) else 1.  ``host_lens``: the
    CPU lengths the loader made (chunk starts need them); without them lens is copied back, which synchronises.
    reseed(epoch) -- the brain calls it at every TRAIN stage start -- reseeds both generators from (seed, epoch),
    so a run resumed at an epoch boundary draws what an uninterrupted run draws."""

    def __init__(self, seed=1986, **cfg):
        super().__init__()
        self.cfg = settings(cfg)
        self.seed = int(seed)
        self.gen = torch.Generator()
        self._dev_gen = None
        self.last_plan = None
        self.reseed(0)
        check_settings(self.cfg)

    def reseed(self, epoch):
        self._seed_now = self.seed * 100003 + int(epoch or 0)
        self.gen.manual_seed(self._seed_now)
        if self._dev_gen is not None:
            self._dev_gen.manual_seed(self._seed_now)

    def _noise(self, wavs):
        if self._dev_gen is None or self._dev_gen.device != wavs.device:
            self._dev_gen = torch.Generator(device=wavs.device)
            self._dev_gen.manual_seed(self._seed_now)
        return torch.randn(wavs.shape, device=wavs.device, dtype=torch.float32, generator=self._dev_gen)

    def forward(self, wavs, lens, host_lens=None):
        if not torch.is_tensor(wavs) or not wavs.is_cuda:
            raise L.SaHipError("augmentation runs on the GPU only (no CPU fallback)")
        repeat = 2 if self.cfg.noise else 1
        if wavs.shape[0] * repeat > MAX_ROWS:
            raise L.SaHipError(f"augmentation: {wavs.shape[0] * repeat} rows exceed the {MAX_ROWS} a launch takes")
        if host_lens is None:
            host_lens = lens.cpu() if lens.is_cuda else lens
        lens = lens.to(wavs.device)
        plan = self.last_plan = draw_plan(self.gen, host_lens, wavs.shape[1], self.cfg)
        out = apply_plan(wavs, lens, plan, self._noise(wavs) if self.cfg.noise else None)
        return out, (lens.repeat(2) if repeat == 2 else lens), repeat


def check_settings(c, batch_size=None):
    """what the kernels cannot run, one line each"""
    if not c.speeds or any(s < 75 or s > 400 for s in c.speeds):
        raise SystemExit(f"augment: speeds {list(c.speeds)} -- a speed is a percentage from 75 to 400")
    for s in c.speeds:
        _, s_out, W, _, _ = resample_table(c.sample_rate, c.sample_rate * s // 100)
        if s_out > 128 or W > 32 or s_out * W > 2048:
            raise SystemExit(f"augment: speed {s} needs a {s_out} x {W} resampling table; the kernel holds 128 x 32 "
                             "and 2048 weights")
    if c.drop_chunk_count_high > 8 or c.drop_chunk_count_low < 0 or c.drop_chunk_count_low > c.drop_chunk_count_high:
        raise SystemExit(f"augment: drop_chunk_count {c.drop_chunk_count_low}..{c.drop_chunk_count_high} -- a row "
                         "carries 0 to 8 dropped chunks")
    if c.drop_chunk_length_low < 0 or c.drop_chunk_length_low > c.drop_chunk_length_high:
        raise SystemExit("augment: drop_chunk_length_low must lie in 0..drop_chunk_length_high")
    if c.drop_freq_count_low < 0 or c.drop_freq_count_low > c.drop_freq_count_high:
        raise SystemExit("augment: drop_freq_count_low must lie in 0..drop_freq_count_high")
    if c.snr_low > c.snr_high:
        raise SystemExit("augment: snr_low must not exceed snr_high")
    if batch_size is not None and int(batch_size) * (2 if c.noise else 1) > MAX_ROWS:
        raise SystemExit(f"augment: batch_size {batch_size} with noise rows is {2 * int(batch_size)} rows; "
                         f"the train path takes at most {MAX_ROWS}")


# ---- speechbrain's two classes, for YAML users ---------------------------------------------------------------------
class TimeDomainSpecAugment(torch.nn.Module):
    """speechbrain.lobes.augment.TimeDomainSpecAugment's constructor; ``(wavs, lens) -> wavs'`` [B, L'] (speed
    perturbation, frequency drop, chunk drop in one launch).  The probabilities must be 1 and the chunk noise
    factor 0: the reference's values, and the only ones built."""

    def __init__(self, perturb_prob=1.0, drop_freq_prob=1.0, drop_chunk_prob=1.0, speeds=(95, 100, 105),
                 sample_rate=16000, drop_freq_count_low=0, drop_freq_count_high=3, drop_chunk_count_low=0,
                 drop_chunk_count_high=5, drop_chunk_length_low=1000, drop_chunk_length_high=2000,
                 drop_chunk_noise_factor=0, seed=1986):
        super().__init__()
        if (perturb_prob, drop_freq_prob, drop_chunk_prob, drop_chunk_noise_factor) != (1.0, 1.0, 1.0, 0):
            raise ValueError("TimeDomainSpecAugment: only probabilities of 1 and drop_chunk_noise_factor 0 are built")
        self.inner = TrainAugment(seed=seed, noise=False, speeds=speeds, sample_rate=sample_rate,
                                  drop_freq_count_low=drop_freq_count_low, drop_freq_count_high=drop_freq_count_high,
                                  drop_chunk_count_low=drop_chunk_count_low,
                                  drop_chunk_count_high=drop_chunk_count_high,
                                  drop_chunk_length_low=drop_chunk_length_low,
                                  drop_chunk_length_high=drop_chunk_length_high)

    def forward(self, waveforms, lengths):
        return self.inner(waveforms, lengths)[0]


class AddNoise(torch.nn.Module):
    """speechbrain.processing.speech_augmentation.AddNoise's constructor; ``(wavs, lens) -> noisy wavs`` [B, L].
    Without csv_file speechbrain adds white noise, which is what is built; a csv_file (recorded noise) is refused."""

    def __init__(self, csv_file=None, csv_keys=None, sorting="random", num_workers=0, snr_low=0, snr_high=0,
                 pad_noise=False, mix_prob=1.0, start_index=None, normalize=False, replacements=None,
                 noise_sample_rate=16000, clean_sample_rate=16000, seed=1986):
        super().__init__()
        if csv_file is not None:
            raise ValueError("AddNoise: noise files (csv_file) are not built; the noise is white")
        if mix_prob != 1.0 or normalize:
            raise ValueError("AddNoise: only mix_prob 1 without normalize is built")
        self.inner = TrainAugment(seed=seed, noise=True, snr_low=snr_low, snr_high=snr_high, speeds=(100,),
                                  drop_freq_count_low=0, drop_freq_count_high=0, drop_chunk_count_low=0,
                                  drop_chunk_count_high=0)

    def forward(self, waveforms, lengths):
        out = self.inner(waveforms, lengths)[0]
        return out[waveforms.shape[0]:]
