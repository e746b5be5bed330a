"""WSOLA time-scale modification: the one waveform transform here that changes how fast an
utterance is spoken.  Windows of 20 ms are copied from the input to the output at a hop of 10 ms, and each window is cut
within +-10 ms of where the tempo says it should be, at the place that continues the previous window best (the least
sum of absolute differences of a 14-bit copy of the waveform).  The samples are moved, not altered: pitch and spectral
envelope stay by construction, the duration becomes n / tempo.  One library call, sa_wsola, all on the GPU: no STFT, no
phase, no iteration and no random number in the transform.

The output's width depends on the tempo, so the tempo of every utterance is known on the host: a drawn tempo comes from
a host generator, and with the relative lengths given on the CPU (as the loaders give them) a call copies nothing from
the device to the host."""
import torch

from . import ops
from .pitchnorm import gpu_only, n_valid, refuse_run_modes

TEMPO_LOW, TEMPO_HIGH = 0.5, 2.0
TEMPO_DEFAULT = 1.0


def _tempo(who, value, error=ValueError):
    try:
        v = float("nan") if isinstance(value, bool) else float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not TEMPO_LOW <= v <= TEMPO_HIGH:
        raise error(f"{who} {value}: a tempo between {TEMPO_LOW:g} and {TEMPO_HIGH:g} (above 1 is faster, a shorter "
                    "output)")
    return v


def tempo_to_q(tempo):
    """rint(tempo 2^16), ties to even: the tempo as the kernels take it"""
    return int(round(float(tempo) * ops.WSOLA_ONE))


class TimeScaler:
    """wavs [B, N] (device), relative lengths [B] -> (out [B, Nout] on the device, lens_out [B] on it): every
    utterance played at ``tempo`` times its speed, or at one tempo per utterance drawn uniformly from ``tempo_range`` =
    (lo, hi) by a host generator the object owns (deterministic in ``seed`` and the number of calls so far).  Row b
    has n_out_b = ops.wsola_out_len(round(lens_b N), tempo_q_b) samples, Nout is the largest of them, samples from
    n_out_b on are zero and lens_out = n_out / Nout.  ``last``: (tempo_q int32 [B], n_out int32 [B], count int32 [B],
    jumps int64 [B]: the windows that do not continue their predecessor) of the last batch, on the device."""
    host_lengths = True        # GenderBrain's hook hands it the loader's CPU lengths: Nout then needs no device read

    def __init__(self, tempo=TEMPO_DEFAULT, tempo_range=None, seed=1):
        if tempo_range is not None:
            try:
                pair = tuple(tempo_range)
            except TypeError:
                pair = ()
            if len(pair) != 2:
                raise ValueError(f"TimeScaler: tempo_range {tempo_range}: (lo, hi) expected")
            lo, hi = (_tempo("TimeScaler: tempo_range", v) for v in pair)
            if lo > hi:
                raise ValueError(f"TimeScaler: tempo_range {tempo_range}: lo is above hi")
            self.tempo_range = (lo, hi)
        else:
            self.tempo_range = None
        self.tempo = _tempo("TimeScaler: tempo", tempo)
        self.seed = int(seed)
        self.gen = None
        self.calls = 0
        self.last = None

    def draw(self, B):
        """tempo_q of the next batch: a list of B host integers"""
        if self.tempo_range is None:
            return [tempo_to_q(self.tempo)] * B
        if self.gen is None:                                 # one host generator for the object's life
            self.gen = torch.Generator(device="cpu")
            self.gen.manual_seed(self.seed)
        lo, hi = self.tempo_range
        u = torch.rand(B, generator=self.gen, dtype=torch.float64).tolist()
        return [tempo_to_q(min(max(lo + (hi - lo) * v, lo), hi)) for v in u]

    @torch.no_grad()
    def __call__(self, wavs, lens):
        gpu_only("TimeScaler", wavs)
        B, N = wavs.shape
        dev = wavs.device
        tq = self.draw(B)
        self.calls += 1
        nv_host = n_valid(lens, N, "cpu").to(torch.int64).tolist()      # (lengths on the device: the one copy back)
        n_out = [ops.wsola_out_len(n, t) for n, t in zip(nv_host, tq)]
        Nout = max(max(n_out), 1)
        # (from pinned memory and asynchronous: a pageable host-to-device copy waits for the stream)
        host = torch.tensor([tq, nv_host], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        tempo_q, nv = host[0], host[1]
        out, n_out_dev, pos, count = ops.wsola(wavs.contiguous(), tempo_q, nv, Nout, return_pos=True)
        k = torch.arange(1, pos.shape[1], device=dev)[None, :]
        moved = (pos[:, 1:] != pos[:, :-1] + ops.WSOLA_H) & (k < count[:, None])
        self.last = (tempo_q, n_out_dev, count, moved.sum(1))
        # (the quotient formed on the host in fp64 and rounded once: the device divides by a rounded reciprocal)
        lens_out = (torch.tensor(n_out, dtype=torch.float64) / float(Nout)).float().pin_memory()
        return out, lens_out.to(dev, non_blocking=True)


def check_tempo_options(settings, block=None):
    """the settings of a recipe's ``tempo_options:`` block (if any) under the top-level overrides (--tempo X, or
    --tempo_min LO --tempo_max HI) -> the keyword arguments of ``TimeScaler`` (tempo or tempo_range, seed), each
    refusal one line"""
    block = settings.get("tempo_options") if block is None else block
    block = block or {}
    x = settings.get("tempo")
    if x is None and settings.get("tempo_min") is None:
        x = block.get("tempo")
    given = x is not None and settings.get("tempo") is not None      # a flag outranks the block's range
    lo = settings.get("tempo_min", None if given else block.get("tempo_min"))
    hi = settings.get("tempo_max", None if given else block.get("tempo_max"))
    if (lo is None) != (hi is None):
        raise SystemExit("--tempo_min LO and --tempo_max HI go together: the range one tempo per utterance is drawn "
                         "from")
    out = {"seed": int(block.get("seed", 1))}
    if lo is not None:
        if settings.get("tempo") is not None:
            raise SystemExit("--tempo X and --tempo_min LO --tempo_max HI exclude each other: one tempo for all, or "
                             "one drawn per utterance")
        lo, hi = _tempo("--tempo_min", lo, SystemExit), _tempo("--tempo_max", hi, SystemExit)
        if lo > hi:
            raise SystemExit(f"--tempo_min {lo:g} is above --tempo_max {hi:g}")
        out["tempo_range"] = (lo, hi)
    else:
        out["tempo"] = _tempo("--tempo", TEMPO_DEFAULT if x is None else x, SystemExit)
    return out


def check_recipe_options(settings, run_opts, environ=None):
    """what gender_classifier_train_tempo.py refuses before anything touches a GPU, one line each"""
    opts = check_tempo_options(settings)
    refuse_run_modes("gender_classifier_train_tempo", settings, run_opts, environ)
    return opts
