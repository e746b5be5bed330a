"""Griffin-Lim inversion: normalised 80-bin log-Mel frames -- what the anonymisers'
``reconstruct`` returns -- back to a 16 kHz waveform, so that anonymised speech can be heard and handed to any
evaluator that takes audio.  The path: de-normalise -> Mel pseudo-inverse -> fast Griffin-Lim (Perraudin et al.,
momentum 0.99) on the front end's own STFT (n_fft 400, hop 160, periodic Hamming window, center=True with zero
padding).  Three kernels of csrc/sa_vocoder.hip, 2 n_iter + 1 launches for the loop and one for the Mel inverse.

The starting phases are drawn on the host from a ``torch.Generator`` the module owns (the project's plan convention:
no device RNG, nothing copied back).  Tables are made in fp64 and rounded once."""
import collections
import functools

import numpy as np
import torch

from . import _lib as L
from .features import HOP, N_FFT, NBIN, _hamming, _mel_matrix

N_MELS = 80
PINV_RCOND = 1e-3


def n_samples(T):
    """samples of T frames (center=True: T = 1 + N // 160, and N is a multiple of the hop)"""
    T = int(T)
    if T < 2:
        raise ValueError(f"the inversion needs at least 2 frames, got {T}")
    return (T - 1) * HOP


@functools.lru_cache(maxsize=None)
def mel_pinv():
    """M [80, 201] fp64: the pseudo-inverse of the project's own filterbank fb [201, 80] with singular values under
    1e-3 of the largest cut (76 of 80 kept; max |M| = 1.37, against 4.5e6 uncut).  Linear power = Mel power @ M.
    Bins 0 and 200, which no filter covers, are exactly zero.  Cached: do not write to it."""
    fb = _mel_matrix(N_MELS, N_FFT, 16000)[:NBIN, :N_MELS].double().numpy()
    M = np.linalg.pinv(fb, rcond=PINV_RCOND)
    M[:, ~fb.any(axis=1)] = 0.0                      # (already below 1e-17 there)
    M.setflags(write=False)
    return M


def envelope(T):
    """E [N + 400] fp64 in padded coordinates: E[p] = sum_t w^2[p - 160 t] over the T frames (what sa_gl_istft
    divides by; the output sample n sits at p = n + 200)"""
    N = n_samples(T)
    w2 = _hamming(N_FFT).astype(np.float64) ** 2
    E = np.zeros(N + N_FFT)
    for t in range(int(T)):
        E[HOP * t:HOP * t + N_FFT] += w2
    return E


@functools.lru_cache(maxsize=None)
def host_tables():
    """(window [400], twiddle [800] = cos then sin(2 pi i / 400)) as fp32 CPU tensors, from fp64"""
    ang = 2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT
    tw = np.concatenate([np.cos(ang), np.sin(ang)]).astype(np.float32)
    return torch.from_numpy(_hamming(N_FFT).copy()), torch.from_numpy(tw)


_dev = {}


def tables(device):
    """(window, twiddle, M fp32 [80, 201]) on ``device``, made once per device"""
    device = torch.device(device)
    if device.type != "cuda":
        raise L.SaHipError("the vocoder runs on the GPU only (no CPU fallback)")
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _dev:
        w, tw = host_tables()
        M = torch.from_numpy(mel_pinv().astype(np.float32))
        _dev[key] = tuple(t.to(device) for t in (w, tw, M))
    return _dev[key]


class GriffinLim(torch.nn.Module):
    """magnitude S [B, T, 201] (device, fp32) -> wav [B, (T - 1) 160]: C = S e^{i phi}, Tprev = 0, then n_iter
    times {y = istft(C); R = stft(y); C = S A / (|A| + 1e-16), A = R - m Tprev; Tprev = R}, m = momentum /
    (1 + momentum), and y = istft(C)."""

    def __init__(self, n_iter=32, momentum=0.99, seed=1986):
        super().__init__()
        if int(n_iter) < 0 or not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"GriffinLim: n_iter {n_iter} >= 0 and momentum {momentum} in [0, 1) expected")
        self.n_iter, self.momentum, self.seed = int(n_iter), float(momentum), int(seed)
        self.gen = torch.Generator()
        self.gen.manual_seed(self.seed)

    @property
    def m(self):
        return self.momentum / (1.0 + self.momentum)

    def draw_phase(self, shape):
        """phi uniform on [0, 2 pi), fp32 on the host, from the module's generator"""
        return torch.rand(tuple(shape), generator=self.gen, dtype=torch.float32) * (2.0 * np.pi)

    @torch.no_grad()
    def forward(self, S, phase=None):
        from . import ops
        if not torch.is_tensor(S) or not S.is_cuda:
            raise L.SaHipError("GriffinLim runs on the GPU only (no CPU fallback)")
        w, tw, _ = tables(S.device)
        phi = self.draw_phase(S.shape) if phase is None else phase
        Cx = torch.polar(S, phi.to(S.device, non_blocking=True))
        Tprev = torch.zeros_like(Cx)
        for _ in range(self.n_iter):
            y = ops.gl_istft(Cx, w, tw)
            Cx, Tprev = ops.gl_project(y, S, Tprev, self.m, w, tw)
        return ops.gl_istft(Cx, w, tw)


def stft(wav):
    """R complex64 [B, T, 201] of wav [B, (T - 1) 160]: sa_gl_project's linear part"""
    from . import ops
    B, N = wav.shape
    if N < HOP or N % HOP:
        raise L.SaHipError(f"wav: expected [B, N] with N a positive multiple of {HOP}, got {tuple(wav.shape)}")
    w, tw, _ = tables(wav.device)
    T = 1 + N // HOP
    one = torch.ones(B, T, NBIN, dtype=torch.float32, device=wav.device)
    return ops.gl_project(wav, one, torch.zeros(B, T, NBIN, dtype=torch.complex64, device=wav.device), 0.0, w, tw)[1]


@torch.no_grad()
def spectral_convergence(wav, S):
    """|| |STFT(wav)| - S ||_F / || S ||_F per utterance -> [B] on the device"""
    mag = stft(wav).abs().double()
    return (((mag - S.double()) ** 2).sum(dim=(1, 2)).sqrt() / (S.double() ** 2).sum(dim=(1, 2)).sqrt()).float()


@torch.no_grad()
def invert_features(feats, normalizer, lens=None, frames=None, return_magnitude=False, **gl):
    """normalised features [B, Tf, 80] (device) -> (wav [B, N], lens): de-normalised with ``normalizer``'s state
    (features.InputNormalization: x std + mean), the first ``frames`` frames kept (the ConvAE pads Tf to a multiple
    of 36), N = (frames - 1) 160.  lens: relative lengths [B] (default ones), returned so that int(lens N) trims
    each row.  gl: GriffinLim's arguments, or gl=<a GriffinLim> to keep one generator across calls."""
    from . import ops
    if not torch.is_tensor(feats) or not feats.is_cuda:
        raise L.SaHipError("invert_features runs on the GPU only (no CPU fallback)")
    if not getattr(normalizer, "_count_positive", False) and normalizer.count <= 0:
        raise L.SaHipError("invert_features: the normaliser has seen no data (count == 0): its mean and std say "
                           "nothing about the features")
    if normalizer.state.device != feats.device:
        normalizer.to(feats.device)
    T = feats.shape[1] if frames is None else int(frames)
    n_samples(T)
    _, _, M = tables(feats.device)
    S = ops.mel_to_mag(feats.float().contiguous(), normalizer.glob_mean.contiguous(),
                       normalizer.glob_std.contiguous(), M, T)
    vocoder = gl.pop("gl", None) or GriffinLim(**gl)
    wav = vocoder(S)
    lens = torch.ones(feats.shape[0]) if lens is None else lens
    return (wav, lens, S) if return_magnitude else (wav, lens)


ANON_MODEL_TYPES = ("convae", "fcae", "endtoend")
# the reports' bounds and defaults, literals because the options are checked before anything loads the library: what
# REPORT_OPTIONS refuses by and reports.REPORTS defaults to (the GPU tests hold them to sa_f0cmp_dim and sa_mcd_dim)
PROSODY_MAX_LAG, PROSODY_LAG_DEFAULT = 32, 8                # ops.F0CMP_MAX_LAG; --prosody_max_lag
MCD_MAX_BAND, MCD_BAND_DEFAULT = 63, 16                     # ops.MCD_MAX_BAND; --mcd_band
MCD_MAX_ORDER, MCD_ORDER_DEFAULT = 32, 13                   # ops.MCD_MAX_ORDER; --mcd_order
# the reports' options (reports.REPORTS) in the order they are checked, rows in the style of pitchnorm.OPTIONS.  A
# flag's ``does`` is what the report does with 16 kHz waveforms only; a dependent option names the flag it needs
# (``owner``) and what nothing else ``does``
ReportOption = collections.namedtuple("ReportOption", "flag kind low high text fmt owner does")


def _report_flag(key, does):
    return ReportOption(f"--{key}", "bool", None, None, "true or false", "{!r}", None, does)


def _report_count(key, low, high, what, owner, does):
    return ReportOption(f"--{key}", "count", low, high, f"{what} in {low}..{high}", "{!r}", owner, does)


REPORT_OPTIONS = {
    "report_stoi": _report_flag("report_stoi", "scores"),
    "report_prosody": _report_flag("report_prosody", "tracks the pitch of"),
    "prosody_max_lag": _report_count("prosody_max_lag", 0, PROSODY_MAX_LAG, "a count of frames", "report_prosody",
                                     "compares two pitch tracks"),
    "report_mcd": _report_flag("report_mcd", "scores"),
    "mcd_band": _report_count("mcd_band", 0, MCD_MAX_BAND, "a count of frames", "report_mcd",
                              "compares two spectral envelopes"),
    "mcd_order": _report_count("mcd_order", 1, MCD_MAX_ORDER, "a count of cepstral coefficients", "report_mcd",
                               "compares two spectral envelopes"),
    "report_formants": _report_flag("report_formants", "tracks the formants of"),
}
# the two modes that re-synthesise the waveform they are given: their flag and what they write
RESYNTH_MODES = {"pitch_norm": ("--pitch_norm true", "pitch-normalised"),
                 "formant_shift": ("--formant_ratio", "formant-shifted")}


TEMPO_FLAGS = ("tempo", "tempo_min", "tempo_max")
# what the time-scale mode refuses: the reports that compare input and output frame against frame
TEMPO_REPORTS = ("report_stoi", "report_prosody", "report_mcd", "report_formants")


def anonymize_mode(settings):
    """what anonymize.py runs: formant_norm (--formant_norm true or --formant_norm_ratio X), mcadams,
    pitch_norm, formant_shift (--formant_ratio without --pitch_norm), passthrough or model; before all of them resynth
    (--resynth true), before that modspec (--modspec_cutoff_hz X), and before
    that tempo (--tempo X or --tempo_min LO --tempo_max HI)"""
    if any(settings.get(k) is not None for k in TEMPO_FLAGS):
        return "tempo"
    if settings.get("modspec_cutoff_hz") is not None:
        return "modspec"
    if settings.get("resynth"):
        return "resynth"
    if settings.get("formant_norm") or settings.get("formant_norm_ratio") is not None:
        return "formant_norm"
    if any(settings.get(k) is not None for k in ("mcadams", "mcadams_min", "mcadams_max")):
        return "mcadams"
    if settings.get("pitch_norm"):
        return "pitch_norm"
    if settings.get("formant_ratio") is not None:
        return "formant_shift"
    return "passthrough" if settings.get("passthrough") else "model"


def check_anonymize_options(settings, run_opts, environ=None):
    """what anonymize.py refuses before anything touches a GPU, one line each"""
    import os
    from . import formantnorm, mcadams, modspec, pitchnorm, sourcefilter, timescale    # (all import this module)
    environ = os.environ if environ is None else environ
    formant = pitchnorm.check_formant_options(settings)
    phase = pitchnorm.check_phase_option(settings)
    mode = anonymize_mode(settings)
    # the modes that move the pitch: --pitch_norm true, and the formant normalisation with a PSOLA stage behind it
    pitch = mode == "pitch_norm" or (mode == "formant_norm" and bool(settings.get("pitch_norm")))
    given = {"--mcadams": any(settings.get(k) is not None for k in ("mcadams", "mcadams_min", "mcadams_max")),
             "--pitch_norm true": settings.get("pitch_norm"),
             "--formant_ratio": "formant_ratio" in formant,
             "--preserve_formants true": formant.get("preserve_formants"),
             "--recon_ckpt": settings.get("recon_ckpt"), "--passthrough true": settings.get("passthrough")}

    def exclude(text, *flags):
        for flag in flags:
            if given[flag]:
                raise SystemExit(text.format(flag))

    if mode == "tempo":                                     # (no model, no checkpoint, no STFT)
        timescale.check_tempo_options(settings)
        for key in ("modspec_cutoff_hz", "modspec_depth") + sourcefilter.FLAGS + formantnorm.FLAGS + (
                "mcadams", "mcadams_min", "mcadams_max", "pitch_norm", "pitch_target_hz", "formant_ratio",
                "preserve_formants", "phase", "psola", "contour_scale", "contour_smooth", "lifter", "recon_ckpt",
                "passthrough"):
            if settings.get(key) is not None:
                raise SystemExit(f"--tempo takes no --{key}: the time-scale modification runs no model and no other "
                                 "transform; it copies windows of the waveform to a new time axis")
        for key in TEMPO_REPORTS:
            if settings.get(key):
                raise SystemExit(f"--tempo takes no --{key} true: that report compares input and output frame against "
                                 "frame, and a changed tempo leaves no such alignment")
    if mode == "modspec":                                   # (no model, no checkpoint, one ISTFT)
        modspec.check_modspec_options(settings)
        for key in sourcefilter.FLAGS + formantnorm.FLAGS + (
                "mcadams", "mcadams_min", "mcadams_max", "pitch_norm", "pitch_target_hz", "formant_ratio",
                "preserve_formants", "phase", "psola", "contour_scale", "contour_smooth", "lifter", "recon_ckpt",
                "passthrough"):
            if settings.get(key) is not None:
                raise SystemExit(f"--modspec_cutoff_hz takes no --{key}: the modulation smoothing runs no model and no "
                                 "other transform; it filters every STFT bin's log magnitude along time, keeps the "
                                 "input's phases and inverts once")
    elif settings.get("modspec_depth") is not None:
        raise SystemExit("--modspec_depth goes with --modspec_cutoff_hz X: the depth is the share of that smoothing "
                         "that is applied")
    if mode == "resynth":                                   # (no model, no checkpoint, no STFT)
        sourcefilter.check_resynth_options(settings)
        given["--formant_norm"] = settings.get("formant_norm") or settings.get("formant_norm_ratio") is not None
        exclude("--resynth true and {} exclude each other: the source-filter resynthesis runs no model and no other "
                "transform; it keeps every frame's LPC envelope and replaces its excitation", "--formant_norm",
                "--mcadams", "--recon_ckpt", "--passthrough true", "--formant_ratio", "--preserve_formants true")
        if settings.get("pitch_norm"):
            raise SystemExit("--resynth true and --pitch_norm true exclude each other: the pulses are laid down at the "
                             "period asked for, so --resynth_pitch_hz X moves the pitch in the same pass")
        if settings.get("pitch_target_hz") is not None:
            raise SystemExit("--resynth true takes no --pitch_target_hz: its target is --resynth_pitch_hz X, and "
                             "without one every utterance keeps its own pitch")
        if phase:
            raise SystemExit("--resynth true and --phase exclude each other: there is no STFT whose phases could be "
                             "chosen")
        for key in ("psola", "contour_scale", "contour_smooth", "lifter") + formantnorm.FLAGS[1:]:
            if settings.get(key) is not None:
                raise SystemExit(f"--resynth true takes no --{key}: that option steers another path, and the "
                                 "resynthesis has no grains, no contour, no cepstral envelope and no formant target")
    else:
        if settings.get("resynth") is not None and not isinstance(settings.get("resynth"), bool):
            raise SystemExit(f"--resynth {settings.get('resynth')}: true or false")
        for key in sourcefilter.FLAGS[1:]:
            if settings.get(key) is not None:
                raise SystemExit(f"--{key} goes with --resynth true: nothing else synthesises an excitation")
    if mode == "formant_norm":                              # (no model, no checkpoint, no STFT)
        formantnorm.check_formant_norm_options(settings)
        exclude("--formant_norm and {} exclude each other: the formant normalisation runs no model and no envelope "
                "warp, and re-synthesises every frame from its own residual", "--mcadams", "--recon_ckpt",
                "--passthrough true", "--formant_ratio", "--preserve_formants true")
        if phase:
            raise SystemExit("--formant_norm and --phase exclude each other: there is no STFT whose phases could be "
                             "chosen")
        if settings.get("pitch_norm") and not pitchnorm.check_psola_option(settings).get("psola"):
            raise SystemExit("--formant_norm true with --pitch_norm true needs --psola true: the one pitch path that "
                             "keeps the envelope the formants were moved to")
    else:
        for key in formantnorm.FLAGS[1:]:
            if settings.get(key) is not None:
                raise SystemExit(f"--{key} goes with --formant_norm true: nothing else normalises the formants")
    if mode == "mcadams":                                   # (no model, no checkpoint)
        mcadams.check_mcadams_options(settings)
        exclude("--mcadams and {} exclude each other: the McAdams transform runs no model, no pitch change and no "
                "envelope warp", "--pitch_norm true", "--formant_ratio", "--preserve_formants true", "--recon_ckpt",
                "--passthrough true")
    if phase.get("phase") == "vocoder":                     # (a real waveform's phases only)
        exclude("--phase vocoder and {} exclude each other: there is no input phase to carry", "--mcadams",
                "--passthrough true", "--recon_ckpt")
        if mode not in RESYNTH_MODES:
            raise SystemExit("--phase vocoder goes with --pitch_norm true or --formant_ratio: the paths that "
                             "re-synthesise a waveform they were given")
    if pitchnorm.check_contour_options(settings) and not pitch:               # 
        raise SystemExit("--contour_scale goes with --pitch_norm true --phase vocoder: the one mode that moves the "
                         "pitch")
    if pitchnorm.check_psola_option(settings).get("psola") and not pitch:                  # 
        raise SystemExit("--psola true goes with --pitch_norm true: it is the pitch normalisation done in the time "
                         "domain, grains between pitch marks laid down again at the new spacing")
    if pitchnorm.check_f0_option(settings) and not pitch and mode not in ("formant_norm", "resynth") and \
            not settings.get("report_f0") \
            and settings.get("report_prosody") is not True and settings.get("report_formants") is not True:
        raise SystemExit("--f0_method goes with --pitch_norm true or --report_f0 true: nothing else tracks F0")  # (21)
    if mode in ("passthrough", "model") and settings.get("model_type") not in ANON_MODEL_TYPES:
        raise SystemExit(f"unknown model_type {settings.get('model_type')!r}: the anonymiser is one of convae, fcae "
                         "and endtoend")
    if formant.get("preserve_formants") and mode != "pitch_norm":
        raise SystemExit("--preserve_formants true goes with --pitch_norm true: it keeps the formants where the "
                         "pitch normalisation would move them")
    if "lifter" in formant and mode not in RESYNTH_MODES:
        raise SystemExit("--lifter goes with --formant_ratio or --pitch_norm true --preserve_formants true")
    if mode in RESYNTH_MODES:
        flag, written = RESYNTH_MODES[mode]
        if settings.get("passthrough"):
            raise SystemExit(f"{flag} and --passthrough true exclude each other: one writes the {written} waveforms, "
                             "the other the vocoded originals")
        if settings.get("recon_ckpt"):
            raise SystemExit(f"{flag} takes no --recon_ckpt: no anonymiser runs, the waveforms are {written}")
    if pitch:
        pitchnorm.check_pitch_target(settings.get("pitch_target_hz", 170.0))
    if mode == "model" and not settings.get("recon_ckpt"):
        raise SystemExit("--recon_ckpt DIR is required without --passthrough true: a CKPT+* directory of "
                         "speechbrain_convae_train.py (model.ckpt, normalizer.ckpt)")
    if not settings.get("out_dir"):
        raise SystemExit("--out_dir OUT is required: the folder the WAV files go to")
    if settings.get("csv") and settings.get("synthetic"):
        raise SystemExit("--csv FILE and --synthetic N exclude each other")
    if not settings.get("csv") and not settings.get("synthetic"):
        raise SystemExit("one of --csv FILE and --synthetic N is required")
    for key, o in REPORT_OPTIONS.items():                   # (DESIGN sections 18, 22, 23, 25: any mode, 16 kHz only)
        val = settings.get(key)
        if val is None:
            continue
        if o.owner and not settings.get(o.owner):
            raise SystemExit(f"{o.flag} needs --{o.owner} true: nothing else {o.does}")
        pitchnorm.check_option(key, val, REPORT_OPTIONS)
        if not o.owner and val and int(settings.get("sample_rate", 16000)) != 16000:
            raise SystemExit(f"{o.flag} true {o.does} 16 kHz waveforms only")
    if int(settings.get("n_iter", 32)) < 0:
        raise SystemExit(f"--n_iter {settings.get('n_iter')}: a count of iterations, 0 or more")
    if run_opts.get("distributed_launch") or int(environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("anonymize runs on one GPU: data parallelism is not implemented for it")
    if run_opts.get("hip_graph") or settings.get("hip_graph"):   # (from the command line it arrives as a setting)
        raise SystemExit("anonymize does not support --hip_graph")
