"""Modulation-spectrum smoothing: the one waveform transform here that acts between frames.  Every
other one changes what a frame holds -- its pitch, its envelope, its excitation -- and leaves how the voice moves from
frame to frame alone.  The rate and depth at which each band's level fluctuates (articulation speed, rhythm, onset
sharpness) is a speaker cue of its own.  This one low-pass filters every STFT bin's log-magnitude trajectory along
time, keeps the input's phases and inverts once.  The path, all on the GPU:

    R = STFT(wav)                                               pitchnorm.padded_stft
    L = ln max(|R|, floor), s = FIR_t(L), C = R exp(depth (s - L))    sa_modspec_smooth
    out = ISTFT(C)                                              sa_gl_istft

No model, no tracker, no Griffin-Lim, no random numbers and no device-to-host copy.  The modified STFT is not a
consistent one, so the inversion gives back some of the modulation that was removed.

The default cutoff of 10 Hz is a convention and has not been validated on speech."""
import torch

from . import ops, vocoder
from .pitchnorm import gpu_only, n_valid, padded_stft, refuse_run_modes

CUTOFF_DEFAULT, DEPTH_DEFAULT = 10.0, 1.0
CUTOFF_LOW, CUTOFF_HIGH = ops.MODSPEC_CUTOFF_LOW, ops.MODSPEC_CUTOFF_HIGH


def _real(value):
    try:
        return float("nan") if isinstance(value, bool) else float(value)
    except (TypeError, ValueError):
        return float("nan")


def _cutoff(who, value, error):
    c = _real(value)
    if not CUTOFF_LOW <= c <= CUTOFF_HIGH:
        raise error(f"{who} {value}: a cutoff between {CUTOFF_LOW:g} and {CUTOFF_HIGH:g} Hz of the 100 Hz frame rate "
                    "(the filter has at most 64 taps a side; at 50 Hz nothing is removed)")
    return c


def _depth(who, value, error):
    d = _real(value)
    if not 0.0 <= d <= 1.0:
        raise error(f"{who} {value}: the share between 0 and 1 of the smoothing that is applied (0 leaves the "
                    "waveform's STFT as it is)")
    return d


def _envelope(who, floor_rel, max_gain_db, error):
    f, g = _real(floor_rel), _real(max_gain_db)
    if not 0.0 < f < 1.0:
        raise error(f"{who}floor_rel {floor_rel} in (0, 1) expected, the floor under the log magnitudes relative to "
                    "the utterance's peak")
    if not g > 0.0:
        raise error(f"{who}max_gain_db {max_gain_db} > 0 expected, the bound on what a bin is raised or lowered by")
    return f, g


class ModulationSmoother:
    """wavs [B, N] (device), relative lengths [B] -> wavs of the same shape: every STFT bin's log magnitude low-pass
    filtered along time at ``cutoff_hz`` (ops.modspec_taps), the phases kept, one inversion; samples from
    round(lens_b N) on are zero.  ``depth`` in [0, 1]: the share of the smoothing applied.  ``floor_rel``: the floor
    under the magnitudes relative to the utterance's peak; ``max_gain_db``: the bound on a bin's gain.  ``last``:
    (peak fp64 [B], frames int32 [B]) of the last batch, on the device."""

    def __init__(self, cutoff_hz=CUTOFF_DEFAULT, depth=DEPTH_DEFAULT, floor_rel=1e-4, max_gain_db=40.0):
        def error(text):
            return ValueError("ModulationSmoother: " + text)

        self.cutoff_hz = _cutoff("cutoff_hz", cutoff_hz, error)
        self.depth = _depth("depth", depth, error)
        self.floor_rel, self.max_gain_db = _envelope("", floor_rel, max_gain_db, error)
        self.J = ops._modspec_half(self.cutoff_hz)[1]         # the filter's taps a side
        self.last = None

    @torch.no_grad()
    def __call__(self, wavs, lens):
        gpu_only("ModulationSmoother", wavs)
        B, N = wavs.shape
        dev = wavs.device
        _, R = padded_stft(wavs)
        nv = n_valid(lens, N, dev)
        frames = (torch.div(nv, ops.YIN_HOP, rounding_mode="floor") + 1).to(torch.int32)
        taps, _ = ops.modspec_taps(self.cutoff_hz, dev)
        depth = torch.full((B,), self.depth, dtype=torch.float32, device=dev)
        C, peak = ops.modspec_smooth(R, taps, depth, frames, self.floor_rel, self.max_gain_db)
        w, tw, _ = vocoder.tables(dev)
        y = ops.gl_istft(C, w, tw)[:, :N]
        self.last = (peak, frames)
        live = torch.arange(N, device=dev)[None, :] < nv[:, None]
        return torch.where(live, y, torch.zeros((), dtype=y.dtype, device=dev)).contiguous()


def check_modspec_options(settings, block=None):
    """the settings of a recipe's ``modspec_options:`` block (if any) under the top-level overrides
    (--modspec_cutoff_hz X, --modspec_depth D) -> the keyword arguments of ``ModulationSmoother``, each refusal one
    line"""
    block = settings.get("modspec_options") if block is None else block
    block = block or {}
    cutoff = settings.get("modspec_cutoff_hz")
    depth = settings.get("modspec_depth")
    if cutoff is None and depth is not None and block.get("cutoff_hz") is None:
        raise SystemExit("--modspec_depth goes with --modspec_cutoff_hz X: the depth is the share of that smoothing "
                         "that is applied")
    if cutoff is None:
        cutoff = block.get("cutoff_hz", CUTOFF_DEFAULT)
    if depth is None:
        depth = block.get("depth", DEPTH_DEFAULT)
    out = {"cutoff_hz": _cutoff("--modspec_cutoff_hz", cutoff, SystemExit),
           "depth": _depth("--modspec_depth", depth, SystemExit)}
    out["floor_rel"], out["max_gain_db"] = _envelope("modspec_options: ", block.get("floor_rel", 1e-4),
                                                     block.get("max_gain_db", 40.0), SystemExit)
    return out


def check_recipe_options(settings, run_opts, environ=None):
    """what gender_classifier_train_modspec.py refuses before anything touches a GPU, one line each"""
    opts = check_modspec_options(settings)
    refuse_run_modes("gender_classifier_train_modspec", settings, run_opts, environ)
    return opts
