"""LPC source-filter resynthesis: the classic LPC vocoder as an anonymiser.  Every other waveform
transform here keeps the speaker's own excitation -- jitter, shimmer, breathiness and the glottal pulse shape all sit
in the LPC residual.  This one throws the residual away: each frame keeps its order-20 all-pole envelope and its
energy, and the filter is driven by a synthetic excitation, pulses at the F0 track where the frame is voiced and
uniform noise elsewhere.  The pulses are laid down at whatever period is asked for, so the same pass normalises the
pitch exactly.  The path, all on the GPU:

    f0 = pitchnorm.f0_track(wav)                                sa_yin_f0 [-> sa_f0_candidates -> sa_f0_viterbi]
    r_b = clamp(target / mean voiced f0), rho_q = rint(r_b 2^16)   sa_pitch_ratio (with a target only)
    pulses every 16000 / (f0 rho) samples                       sa_srcfilt_pulses
    exc = noise + interpolated pulses                           sa_srcfilt_excite
    out = frame-wise 1 / A(z) driven by exc, overlap-add, level sa_srcfilt_synth

No STFT, no phase, no pitch marks, no iteration and no device-to-host copy.

The default ``aspiration`` of 0.3 puts a voiced frame's noise at 0.3^2 / 3 of its pulses' power, about -15 dB.  It is
a convention and has not been validated on speech."""
import torch

from . import ops
from .pitchnorm import (R_HIGH, R_LOW, TARGET_HIGH, TARGET_LOW, check_f0_option, check_pitch_target, f0_settings,
                        f0_track, gpu_only, n_valid, refuse_run_modes)

ASPIRATION_DEFAULT = 0.3
SEED_MAX = 2 ** 31 - 1
FLAGS = ("resynth", "resynth_pitch_hz", "aspiration")      # the mode's own flags (--f0_method and --seed are shared)


def _aspiration(who, value, error):
    try:
        a = float(value)
    except (TypeError, ValueError):
        a = float("nan")
    if isinstance(value, bool) or not 0.0 <= a <= 1.0:
        raise error(f"{who} {value}: the level between 0 and 1 of the noise under a voiced frame's pulses, relative to "
                    "an unvoiced frame's noise")
    return a


def _mul32(x, c):
    """x c mod 2^32 on int64 tensors holding uint32 values, without leaving int64"""
    return (x * (c & 0xffff) + (((x * (c >> 16)) & 0xffff) << 16)) & 0xffffffff


def _mix(x):
    """sa_srcfilt_excite's 32-bit mix on an int64 tensor of uint32 values"""
    x = x & 0xffffffff
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7feb352d)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846ca68b)
    return x ^ (x >> 16)


def _seed(who, value, error):
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= SEED_MAX:
        raise error(f"{who} {value}: a whole number from 0 to {SEED_MAX}, the seed of the excitation's noise")
    return value


class SourceFilter:
    """wavs [B, N] (device), relative lengths [B] -> wavs of the same shape: every frame's LPC envelope and energy
    under a pulse/noise excitation; samples from round(lens_b N) on are zero.  ``pitch_target_hz`` None keeps every
    utterance's own F0 track; a target moves the mean of its voiced F0 there (ops.pitch_ratio's ratio, clamped to
    [r_min, r_max], 1 under ``min_voiced`` voiced frames).  ``aspiration``: the noise under the pulses of a voiced
    frame.  One noise seed per utterance is drawn from a generator the object owns (deterministic in ``seed`` and the
    number of calls so far).  ``level``: the RMS of every utterance is brought back to its input's.  ``last``: (f0
    fp32 [B, T], rho_q int32 [B, T], pulse count int32 [B], gain fp32 [B], counts int64 [B, 4] of resynthesised /
    silent / fallback / unexcited frames) of the last batch, on the device."""

    def __init__(self, pitch_target_hz=None, aspiration=ASPIRATION_DEFAULT, seed=1, f0_method="yin", level=True,
                 r_min=0.5, r_max=2.0, min_voiced=5, threshold=0.15):
        def error(text):
            return ValueError("SourceFilter: " + text)

        if pitch_target_hz is not None and (isinstance(pitch_target_hz, bool) or
                                            not TARGET_LOW <= float(pitch_target_hz) <= TARGET_HIGH):
            raise error(f"pitch_target_hz {pitch_target_hz} in {TARGET_LOW:g}..{TARGET_HIGH:g} (or None: the "
                        "utterance's own pitch) expected")
        self.pitch_target_hz = None if pitch_target_hz is None else float(pitch_target_hz)
        self.aspiration = _aspiration("aspiration", aspiration, error)
        self.seed = _seed("seed", seed, error)
        self.f0_method, _ = f0_settings("SourceFilter", f0_method, None)
        if not R_LOW <= float(r_min) <= float(r_max) <= R_HIGH:
            raise error(f"{R_LOW} <= r_min {r_min} <= r_max {r_max} <= {R_HIGH} expected")
        if isinstance(min_voiced, bool) or int(min_voiced) != min_voiced or int(min_voiced) < 1:
            raise error(f"min_voiced {min_voiced}: a count of frames, 1 or more")
        self.r_min, self.r_max, self.min_voiced = float(r_min), float(r_max), int(min_voiced)
        self.level, self.threshold = bool(level), float(threshold)
        self.drawn = 0
        self.calls = 0
        self.last = None

    def draw(self, B, device):
        """the noise seeds int32 [B] on the device for the next batch: a counter-based generator, the noise's own
        32-bit mix of (utterances drawn so far + b) ^ mix(seed) with the top bit cleared -- deterministic in ``seed``
        and the calls so far, formed on the device, and restated by tests/srcfilt_ref.py"""
        i = torch.arange(self.drawn, self.drawn + B, dtype=torch.int64, device=device)
        self.drawn += B
        return (_mix(i ^ int(_mix(torch.tensor(self.seed, dtype=torch.int64)))) & SEED_MAX).to(torch.int32)

    @torch.no_grad()
    def __call__(self, wavs, lens):
        gpu_only("SourceFilter", wavs)
        B, N = wavs.shape
        wavs = wavs.contiguous()
        lens = lens.to(wavs.device, torch.float32).contiguous()
        f0 = f0_track(wavs, self.threshold, self.f0_method, lens)
        T = f0.shape[1]
        if self.pitch_target_hz is None:
            rho_q = torch.full((B, T), ops.SRCFILT_RHO_ONE, dtype=torch.int32, device=wavs.device)
        else:
            ratio, _, _ = ops.pitch_ratio(f0, lens, N, self.pitch_target_hz, self.r_min, self.r_max, self.min_voiced)
            rho_q = torch.round(ratio.double() * ops.SRCFILT_RHO_ONE).to(torch.int32)[:, None].expand(B, T)
            rho_q = rho_q.contiguous()
        seeds = self.draw(B, wavs.device)
        self.calls += 1
        out, gain, count, status = ops.srcfilt(wavs, f0, rho_q, seeds, n_valid(lens, N, wavs.device).to(torch.int32),
                                               self.aspiration, self.level, return_status=True)
        counts = torch.stack([(status == k).sum(1) for k in range(4)], 1)
        self.last = (f0, rho_q, count, gain, counts)
        return out


def check_resynth_options(settings, block=None):
    """the settings of a recipe's ``resynth_options:`` block (if any) under the top-level overrides (--resynth_pitch_hz
    X, --aspiration A, --f0_method M) -> the keyword arguments of ``SourceFilter``, each refusal one line.  The noise
    seed is the block's (anonymize.py passes its own --seed)."""
    block = settings.get("resynth_options") if block is None else block
    block = block or {}
    flag = settings.get("resynth")
    if flag is not None and not isinstance(flag, bool):
        raise SystemExit(f"--resynth {flag}: true or false")

    def pick(key, name):
        return settings[key] if settings.get(key) is not None else block.get(name)

    out = {"level": bool(block.get("level", True))}
    target = pick("resynth_pitch_hz", "pitch_target_hz")
    if target is not None:
        if isinstance(target, bool):
            raise SystemExit(f"--resynth_pitch_hz {target}: a target between {TARGET_LOW:g} and {TARGET_HIGH:g} Hz, "
                             "the range the F0 tracker covers")
        try:
            target = float(target)
        except (TypeError, ValueError):
            target = float("nan")
        try:
            target = check_pitch_target(target)
        except SystemExit as e:
            raise SystemExit(str(e).replace("--pitch_target_hz", "--resynth_pitch_hz")) from None
    out["pitch_target_hz"] = target
    asp = pick("aspiration", "aspiration")
    out["aspiration"] = _aspiration("--aspiration", ASPIRATION_DEFAULT if asp is None else asp, SystemExit)
    out["seed"] = _seed("resynth_options: seed", block.get("seed", 1), SystemExit)
    r_min, r_max = block.get("r_min", R_LOW), block.get("r_max", R_HIGH)
    if not R_LOW <= float(r_min) <= float(r_max) <= R_HIGH:
        raise SystemExit(f"resynth_options: {R_LOW} <= r_min {r_min} <= r_max {r_max} <= {R_HIGH} expected, the ratios "
                         "the kernels take")
    out["r_min"], out["r_max"] = float(r_min), float(r_max)
    mv = block.get("min_voiced", 5)
    if isinstance(mv, bool) or not isinstance(mv, int) or mv < 1:
        raise SystemExit(f"resynth_options: min_voiced {mv}: a count of frames, 1 or more")
    out["min_voiced"] = mv
    out["f0_method"] = check_f0_option(settings, block).get("f0_method", "yin")
    return out


def check_recipe_options(settings, run_opts, environ=None):
    """what gender_classifier_train_resynth.py refuses before anything touches a GPU, one line each"""
    opts = check_resynth_options(settings)
    refuse_run_modes("gender_classifier_train_resynth", settings, run_opts, environ)
    return opts
