"""LPC formant normalisation: every utterance's vocal-tract resonances brought to one place, the
way pitchnorm.PitchNormalizer brings every F0 to one target.  The utterance's formants are tracked
(ops.formant_tracks) on its voiced frames (pitchnorm.f0_track), their medians give the ratio q that moves their
geometric mean onto the target's (ops.formant_centre), and every complex LPC pole's angle is scaled by q inside
sa_mcadams's analysis/synthesis framing (ops.pole_warp): a vocal-tract-length warp of the poles themselves.  Pitch and
timing stay.  All on the GPU, no model, no phase reconstruction and no device-to-host copy.

The default target, (550, 1650, 2750) Hz, is the neutral-vowel resonances of a 15.9 cm tube closed at one end
(c / 4L = 550 Hz and its odd multiples), between the usual male and female figures.  It is a convention and has not
been validated on speech.

Measured on the fp64 restatement and not repaired: for q > 1 the poles above the map's knee are
squeezed towards pi with their moduli kept and the output gains a resonance at the top of the band -- beyond q of
about 1.05 most of its energy lies above 6.5 kHz and an F0 tracker finds no voiced frame in it.  q < 1 has no such
effect."""
import torch

from . import ops
from .pitchnorm import check_f0_option, f0_settings, f0_track, gpu_only, n_valid

TARGET_DEFAULT = (550.0, 1650.0, 2750.0)
Q_LOW, Q_HIGH = 0.8, 1.2                     # what this layer accepts (the kernel itself takes 0.5..2)
F_LOW, F_HIGH = ops.FORMANT_F_LOW, ops.FORMANT_F_HIGH        # the tracker's gate: where a target may lie
MIN_FRAMES = 8
FLAGS = ("formant_norm", "formant_target", "formant_norm_ratio", "formant_q_min", "formant_q_max")


def _target(who, value, error):
    try:
        t = tuple(float(v) for v in (value.replace(",", " ").split() if isinstance(value, str) else value))
    except (TypeError, ValueError):
        t = ()
    if len(t) != 3 or not F_LOW <= t[0] < t[1] < t[2] <= F_HIGH:
        raise error(f"{who} {value}: three frequencies F1,F2,F3 in Hz, {F_LOW:g} <= F1 < F2 < F3 <= {F_HIGH:g}")
    return t


def _ratio(who, value, error, low=Q_LOW, high=Q_HIGH):
    try:
        q = float(value)
    except (TypeError, ValueError):
        q = float("nan")
    if isinstance(value, bool) or not low <= q <= high:
        raise error(f"{who} {value}: a ratio between {low:g} and {high:g} by which the pole angles are scaled")
    return q


class FormantNormalizer:
    """wavs [B, N] (device), relative lengths [B] -> wavs of the same shape whose three lowest resonances have the
    geometric mean of ``target_hz``; samples from round(lens_b N) on are zero.  The steps: the F0 track
    (``f0_method``), ops.formant_tracks, ops.formant_centre (q in [q_min, q_max]; a row with fewer than ``min_frames``
    scored and voiced frames keeps q = 1 and is copied), ops.pole_warp.  ``ratio=X`` skips the first three: q is X for
    every row.  ``level``: the RMS of every utterance is brought back to its input's.  ``last``: (q fp32 [B], med
    fp32 [B, 3], count int32 [B], gain fp32 [B], counts int64 [B, 3] of transformed / silent / fallback frames) of
    the last batch, on the device; with ``ratio`` med and count are zeros."""

    def __init__(self, target_hz=TARGET_DEFAULT, ratio=None, q_min=Q_LOW, q_max=Q_HIGH, min_frames=MIN_FRAMES,
                 f0_method="yin", level=True, threshold=0.15):
        def error(text):
            return ValueError("FormantNormalizer: " + text)

        self.target_hz = _target("target_hz", target_hz, error)
        self.ratio = None if ratio is None else _ratio("ratio", ratio, error)
        self.q_min, self.q_max = _ratio("q_min", q_min, error, Q_LOW, 1.0), _ratio("q_max", q_max, error, 1.0, Q_HIGH)
        if isinstance(min_frames, bool) or int(min_frames) != min_frames or int(min_frames) < 1:
            raise error(f"min_frames {min_frames}: a count of frames, 1 or more")
        self.min_frames = int(min_frames)
        self.f0_method, _ = f0_settings("FormantNormalizer", f0_method, None)
        self.level, self.threshold = bool(level), float(threshold)
        self.last = None

    def centre(self, wavs, lens):
        """-> (med [B, 3], q [B], count [B]) of wavs: where its formants lie and the ratio to the target"""
        B, N = wavs.shape
        nv = n_valid(lens, N, wavs.device)
        f0 = f0_track(wavs, self.threshold, self.f0_method, lens)
        freq, status = ops.formant_tracks(wavs, nv.to(torch.int32))
        frames = (torch.floor(nv / ops.YIN_HOP) + 1).clamp(max=f0.shape[1]).to(torch.int32)
        frames = torch.where(nv > 0, frames, torch.zeros_like(frames))
        return ops.formant_centre(freq, status, f0, frames, self.target_hz, self.q_min, self.q_max, self.min_frames)

    @torch.no_grad()
    def __call__(self, wavs, lens):
        gpu_only("FormantNormalizer", wavs)
        B, N = wavs.shape
        wavs = wavs.contiguous()
        lens = lens.to(wavs.device, torch.float32).contiguous()
        if self.ratio is None:
            med, q, count = self.centre(wavs, lens)
        else:
            q = torch.full((B,), self.ratio, dtype=torch.float32, device=wavs.device)
            med = torch.zeros(B, ops.FORMANTS, dtype=torch.float32, device=wavs.device)
            count = torch.zeros(B, dtype=torch.int32, device=wavs.device)
        out, gain, status = ops.pole_warp(wavs, q, n_valid(lens, N, wavs.device).to(torch.int32), self.level,
                                          return_status=True)
        counts = torch.stack([(status == k).sum(1) for k in range(3)], 1)
        self.last = (q, med, count, gain, counts)
        return out


def check_formant_norm_options(settings, block=None):
    """the settings of a recipe's ``formant_norm:`` block (if any) under the top-level overrides (--formant_target
    F1,F2,F3, --formant_norm_ratio X, --formant_q_min A, --formant_q_max B, --f0_method M) -> the keyword arguments of
    ``FormantNormalizer``, each refusal one line"""
    flag = settings.get("formant_norm")
    if isinstance(flag, dict):                               # (a recipe's block; on a command line the key is the flag)
        block, flag = (flag if block is None else block), None
    block = block or {}
    if flag is not None and not isinstance(flag, bool):
        raise SystemExit(f"--formant_norm {flag}: true or false")
    if flag is False and settings.get("formant_norm_ratio") is not None:
        raise SystemExit("--formant_norm false and --formant_norm_ratio X exclude each other: the ratio implies the "
                         "mode")

    def pick(key, name):
        return settings[key] if settings.get(key) is not None else block.get(name)

    out = {"level": bool(block.get("level", True))}
    target, ratio = pick("formant_target", "target_hz"), pick("formant_norm_ratio", "ratio")
    if settings.get("formant_norm_ratio") is not None and settings.get("formant_target") is not None:
        raise SystemExit("--formant_norm_ratio X and --formant_target F1,F2,F3 exclude each other: one ratio for all, "
                         "or one per utterance from its own formants")
    if settings.get("formant_norm_ratio") is not None:
        target = None                                        # (a flag outranks the block's target)
    elif settings.get("formant_target") is not None:
        ratio = None
    if ratio is not None and target is not None:
        raise SystemExit("formant_norm: ratio and target_hz exclude each other: one ratio for all, or one per "
                         "utterance from its own formants")
    if ratio is not None:
        out["ratio"] = _ratio("--formant_norm_ratio", ratio, SystemExit)
    out["target_hz"] = TARGET_DEFAULT if target is None else _target("--formant_target", target, SystemExit)
    lo, hi = pick("formant_q_min", "q_min"), pick("formant_q_max", "q_max")
    if ratio is not None and (settings.get("formant_q_min") is not None or settings.get("formant_q_max") is not None):
        raise SystemExit("--formant_q_min A and --formant_q_max B bound the ratio an utterance's own formants give: "
                         "--formant_norm_ratio X leaves nothing to bound")
    out["q_min"] = _ratio("--formant_q_min", Q_LOW if lo is None else lo, SystemExit, Q_LOW, 1.0)
    out["q_max"] = _ratio("--formant_q_max", Q_HIGH if hi is None else hi, SystemExit, 1.0, Q_HIGH)
    mf = block.get("min_frames", MIN_FRAMES)
    if isinstance(mf, bool) or not isinstance(mf, int) or mf < 1:
        raise SystemExit(f"formant_norm: min_frames {mf}: a count of frames, 1 or more")
    out["min_frames"] = mf
    out["f0_method"] = check_f0_option(settings, block).get("f0_method", "yin")
    return out


def check_recipe_options(settings, run_opts, environ=None):
    """what gender_classifier_train_formant_norm.py refuses before anything touches a GPU, one line each -> (the
    keyword arguments of ``FormantNormalizer``, those of the PSOLA ``PitchNormalizer`` behind it or None)"""
    from . import pitchnorm
    block = settings.get("formant_norm") if isinstance(settings.get("formant_norm"), dict) else {}
    opts = check_formant_norm_options(settings, block)
    pitch = None
    flag = settings.get("pitch_norm", block.get("pitch_norm", False))
    if not isinstance(flag, bool):
        raise SystemExit(f"--pitch_norm {flag}: true or false")
    if flag:
        target = settings.get("pitch_target_hz", block.get("pitch_target_hz", 170.0))
        pitch = {"target_hz": pitchnorm.check_pitch_target(target), "psola": True, "f0_method": opts["f0_method"]}
    pitchnorm.refuse_run_modes("gender_classifier_train_formant_norm", settings, run_opts, environ)
    return opts, pitch
