"""Pitch normalisation: every utterance's pitch is scaled so that the mean of its voiced F0
becomes ``target_hz`` -- the signal-processing baseline the learned anonymisers are compared against (the
reference's gender_classifier_train_pitch_norm.py, which does it with WORLD).  The path, all on the GPU:

    f0 = YIN(wav)                                   sa_yin_f0
    r_b = clamp(target / mean voiced f0, r_min, r_max), 1 under min_voiced voiced frames     sa_pitch_ratio
    S' = |STFT(wav)| resampled along time to r_b times as many frames                        sa_pitch_stretch_mag
    y' = Griffin-Lim(S')                            vocoder.GriffinLim, unchanged
    out[n] = windowed-sinc read of y' at n r_b      sa_pitch_resample

Stretching by r_b and reading r_b times as fast keeps the duration and multiplies every frequency -- pitch and
formants alike -- by r_b.  The one device-to-host copy of the path is the B ratios, which size the stretched
spectrogram."""
import math

import torch

from . import _lib as L
from . import vocoder
from .features import HOP

SAMPLE_RATE, W, TAU_MIN, TAU_MAX = 16000, 400, 40, 266
R_LOW, R_HIGH = 0.5, 2.0                     # what the kernels take
TARGET_LOW, TARGET_HIGH = 60.0, 400.0        # the tracker's range: 16000 / tau_max .. 16000 / tau_min


def f0_track(wav, threshold=0.15):
    """wav [B, N] (device, fp32) -> f0 [B, N // 160 + 1] in Hz, one value per Fbank frame, 0 where unvoiced"""
    from . import ops
    return ops.yin_f0(wav, threshold)


def stretched_frames(Tp, ratio):
    """T'_b = ceil((T_p - 1) r_b) + 1, from the fp32 ratio in fp64 as the kernel forms it"""
    return int(math.ceil((int(Tp) - 1) * float(ratio))) + 1


class PitchNormalizer:
    """wavs [B, N] (device), relative lengths [B] -> wavs of the same shape whose voiced F0 has mean ~ target_hz;
    samples from round(lens_b N) on are zero.  ``last``: (ratio, mean f0, voiced frames) of the last batch, on
    the device."""

    def __init__(self, target_hz=170.0, n_iter=32, momentum=0.99, seed=1, r_min=0.5, r_max=2.0, min_voiced=5,
                 threshold=0.15):
        if not TARGET_LOW <= float(target_hz) <= TARGET_HIGH:
            raise ValueError(f"PitchNormalizer: target_hz {target_hz} in {TARGET_LOW:g}..{TARGET_HIGH:g} expected")
        if not R_LOW <= float(r_min) <= float(r_max) <= R_HIGH:
            raise ValueError(f"PitchNormalizer: {R_LOW} <= r_min {r_min} <= r_max {r_max} <= {R_HIGH} expected")
        self.target_hz, self.r_min, self.r_max = float(target_hz), float(r_min), float(r_max)
        self.min_voiced, self.threshold = int(min_voiced), float(threshold)
        self.gl = vocoder.GriffinLim(n_iter=n_iter, momentum=momentum, seed=seed)
        self.last = None

    @torch.no_grad()
    def __call__(self, wavs, lens):
        from . import ops
        if not torch.is_tensor(wavs) or not wavs.is_cuda:
            raise L.SaHipError("PitchNormalizer runs on the GPU only (no CPU fallback)")
        lens = lens.to(wavs.device, torch.float32).contiguous()
        f0 = ops.yin_f0(wavs, self.threshold)
        self.last = ops.pitch_ratio(f0, lens, wavs.shape[1], self.target_hz, self.r_min, self.r_max, self.min_voiced)
        return self.shift(wavs, lens, self.last[0])

    @torch.no_grad()
    def shift(self, wavs, lens, ratio):
        """the stretch, the phase reconstruction and the resampling with a given ratio (fp32 [B], device)"""
        from . import ops
        if not torch.is_tensor(wavs) or not wavs.is_cuda:
            raise L.SaHipError("PitchNormalizer runs on the GPU only (no CPU fallback)")
        B, N = wavs.shape
        host = ratio.detach().cpu().tolist()                 # the path's one synchronisation: T' is a shape
        if not all(R_LOW <= r <= R_HIGH for r in host):
            raise L.SaHipError(f"PitchNormalizer.shift: ratios in [{R_LOW}, {R_HIGH}] expected, got {host}")
        Np = HOP * -(-N // HOP)
        wp = torch.nn.functional.pad(wavs, (0, Np - N)) if Np != N else wavs
        R = vocoder.stft(wp.contiguous())
        Tout = max(stretched_frames(R.shape[1], r) for r in host)
        y = self.gl(ops.pitch_stretch_mag(R, ratio, Tout))
        n_valid = torch.round(lens.to(wavs.device).double() * N).clamp(0, N).to(torch.int32)
        return ops.pitch_resample(y, ratio, n_valid, N)


def check_pitch_target(value):
    target = float(value)
    if not TARGET_LOW <= target <= TARGET_HIGH:
        raise SystemExit(f"--pitch_target_hz {target:g}: a target between {TARGET_LOW:g} and {TARGET_HIGH:g} Hz, "
                         "the range the F0 tracker covers")
    return target


def check_pitch_options(settings, run_opts, environ=None):
    """what gender_classifier_train_pitch_norm.py refuses before anything touches a GPU, one line each"""
    import os
    environ = os.environ if environ is None else environ
    pn = settings.get("pitch_norm") or {}
    target = check_pitch_target(settings.get("pitch_target_hz", pn.get("target_hz", 170.0)))
    r_min, r_max = float(pn.get("r_min", R_LOW)), float(pn.get("r_max", R_HIGH))
    if r_min < R_LOW or r_max > R_HIGH:
        raise SystemExit(f"pitch_norm: r_min {r_min:g} and r_max {r_max:g} must lie in [{R_LOW}, {R_HIGH}], the "
                         "ratios the kernels take")
    if r_min > r_max:
        raise SystemExit(f"pitch_norm: r_min {r_min:g} is above r_max {r_max:g}")
    if run_opts.get("distributed_launch") or int(environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("gender_classifier_train_pitch_norm runs on one GPU: data parallelism is not implemented "
                         "for it")
    if run_opts.get("hip_graph") or settings.get("hip_graph"):   # (from the command line it arrives as a setting)
        raise SystemExit("gender_classifier_train_pitch_norm does not support --hip_graph")
    return dict(pn, target_hz=target, r_min=r_min, r_max=r_max)
