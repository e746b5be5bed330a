"""McAdams-coefficient anonymisation: VoicePrivacy's signal-processing baseline (B2; B1.b with a
random coefficient per utterance).  Every frame's LPC filter is fitted, the angle phi of each of its complex poles
is raised to the power alpha, and the frame is re-synthesised from its own residual: pitch and timing stay, every
formant moves by its own amount (phi = 1 rad, 2546 Hz, is the fixed point; below it a formant moves up for
alpha < 1).  One library call, sa_mcadams, all on the GPU, no phase reconstruction and no device-to-host copy."""
import torch

from . import ops
from .pitchnorm import gpu_only, n_valid, refuse_run_modes

ALPHA_LOW, ALPHA_HIGH = 0.5, 1.2             # what this layer accepts (the kernel itself takes 0.25..2)
ALPHA_DEFAULT = 0.8


def _alpha(who, value):
    try:
        a = float(value)
    except (TypeError, ValueError):
        a = float("nan")
    if not ALPHA_LOW <= a <= ALPHA_HIGH:
        raise ValueError(f"{who}: alpha {value} in {ALPHA_LOW}..{ALPHA_HIGH} expected")
    return a


class McAdams:
    """wavs [B, N] (device), relative lengths [B] -> wavs of the same shape, McAdams-transformed with coefficient
    ``alpha``, or with one coefficient per utterance drawn uniformly from ``alpha_range`` = (lo, hi) by a generator
    the object owns (deterministic in ``seed`` and the number of calls so far).  ``level``: the RMS of every
    utterance is brought back to its input's.  Samples from round(lens_b N) on are zero.  ``last``: (alpha fp32 [B],
    gain fp32 [B], counts int64 [B, 3] of transformed / silent / fallback frames) of the last batch, on the
    device."""

    def __init__(self, alpha=ALPHA_DEFAULT, alpha_range=None, seed=1, level=True):
        if alpha_range is not None:
            if len(tuple(alpha_range)) != 2:
                raise ValueError(f"McAdams: alpha_range {alpha_range}: (lo, hi) expected")
            lo, hi = (_alpha("McAdams", v) for v in alpha_range)
            if lo > hi:
                raise ValueError(f"McAdams: alpha_range {alpha_range}: lo is above hi")
            self.alpha_range = (lo, hi)
        else:
            self.alpha_range = None
        self.alpha = _alpha("McAdams", alpha)
        self.seed, self.level = int(seed), bool(level)
        self.gen = None
        self.calls = 0
        self.last = None

    def draw(self, B, device):
        """alpha fp32 [B] on the device for the next batch"""
        if self.alpha_range is None:
            return torch.full((B,), self.alpha, dtype=torch.float32, device=device)
        if self.gen is None:                                 # one generator for the object's life, on its first device
            self.gen = torch.Generator(device=device)
            self.gen.manual_seed(self.seed)
        lo, hi = self.alpha_range
        u = torch.rand(B, generator=self.gen, dtype=torch.float32, device=device)
        return (lo + (hi - lo) * u).clamp_(lo, hi)

    @torch.no_grad()
    def __call__(self, wavs, lens):
        gpu_only("McAdams", wavs)
        B, N = wavs.shape
        alpha = self.draw(B, wavs.device)
        self.calls += 1
        out, gain, status = ops.mcadams(wavs.contiguous(), alpha, n_valid(lens, N, wavs.device).to(torch.int32),
                                        self.level, return_status=True)
        counts = torch.stack([(status == k).sum(1) for k in range(3)], 1)
        self.last = (alpha, gain, counts)
        return out


def check_mcadams_options(settings, block=None):
    """the McAdams settings of a recipe's ``mcadams_options:`` block (if any) under the top-level overrides
    (--mcadams A, or --mcadams_min LO --mcadams_max HI) -> the keyword arguments of ``McAdams`` (alpha or
    alpha_range, seed, level), each refusal one line"""
    block = settings.get("mcadams_options") if block is None else block
    block = block or {}
    a = settings.get("mcadams")
    if a is None and settings.get("mcadams_min") is None:
        a = block.get("alpha")
    given = a is not None and settings.get("mcadams") is not None     # a flag outranks the block's range
    lo = settings.get("mcadams_min", None if given else block.get("alpha_min"))
    hi = settings.get("mcadams_max", None if given else block.get("alpha_max"))

    def coefficient(flag, value):
        try:
            v = float(value)
        except (TypeError, ValueError):
            v = float("nan")
        if isinstance(value, bool) or not ALPHA_LOW <= v <= ALPHA_HIGH:
            raise SystemExit(f"{flag} {value}: a McAdams coefficient between {ALPHA_LOW:g} and {ALPHA_HIGH:g}")
        return v

    if (lo is None) != (hi is None):
        raise SystemExit("--mcadams_min LO and --mcadams_max HI go together: the range one coefficient per "
                         "utterance is drawn from")
    out = {"seed": int(block.get("seed", 1)), "level": bool(block.get("level", True))}
    if lo is not None:
        if settings.get("mcadams") is not None:
            raise SystemExit("--mcadams A and --mcadams_min LO --mcadams_max HI exclude each other: one coefficient "
                             "for all, or one drawn per utterance")
        lo, hi = coefficient("--mcadams_min", lo), coefficient("--mcadams_max", hi)
        if lo > hi:
            raise SystemExit(f"--mcadams_min {lo:g} is above --mcadams_max {hi:g}")
        out["alpha_range"] = (lo, hi)
    else:
        out["alpha"] = coefficient("--mcadams", ALPHA_DEFAULT if a is None else a)
    return out


def check_recipe_options(settings, run_opts, environ=None):
    """what gender_classifier_train_mcadams.py refuses before anything touches a GPU, one line each"""
    opts = check_mcadams_options(settings)
    refuse_run_modes("gender_classifier_train_mcadams", settings, run_opts, environ)
    return opts
