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
spectrogram.

Formants apart from pitch: with ``formant_ratio`` beta (``preserve_formants``: beta = 1) the
stretched magnitudes pass through sa_env_warp with q_b = r_b / beta before Griffin-Lim -- their cepstral envelope
is read q_b times as far up, so that after the resampling the harmonics sit at r_b f and the envelope at beta f.
``FormantShifter`` is the same warp with no pitch change at all: |STFT| -> warp by 1 / beta -> Griffin-Lim.

The input's own phase: with ``phase="vocoder"`` both classes carry the phases of STFT(wav) through
the stretch (sa_pv_synth, a phase vocoder) and invert once, in place of Griffin-Lim's 32 iterations from random
phases: stretch [-> warp] -> sa_pv_synth -> one sa_gl_istft.  ``"griffin_lim"`` stays the default.

The contour: with ``contour_scale`` gamma (and ``phase="vocoder"``) the ratio varies from frame to
frame so that the output's F0 contour is target + gamma (f0 - mean) -- 1 the additive shift of the reference's
baseline, 0 a monotone voice: sa_pitch_contour -> [sa_env_warp_frames] -> sa_pv_synth_map -> sa_pitch_resample_map.

The track: with ``f0_method="viterbi"`` the F0 of every path above is a Viterbi decode through each
frame's d' dips (sa_f0_candidates -> sa_f0_viterbi on sa_yin_f0's d') instead of the first dip under the threshold.

In the time domain: with ``psola=True`` nothing above but the track and the ratios runs.  The
waveform is cut into two-period grains centred on pitch marks and the same grains are laid down again at the new spacing
(TD-PSOLA): sa_psola_marks -> sa_psola_plan -> sa_psola_ola.  The grains are moved, not altered, so the envelope stays
where it was and there is no phase to choose; the duration is kept, a ratio per frame costs nothing extra, and nothing
is copied to the host."""
import collections
import math

import torch

from . import _lib as L
from . import ops, vocoder
from .features import HOP

SAMPLE_RATE, W, TAU_MIN, TAU_MAX = 16000, 400, 40, 266
R_LOW, R_HIGH = 0.5, 2.0                     # what the kernels take
TARGET_LOW, TARGET_HIGH = 60.0, 400.0        # the tracker's range: 16000 / tau_max .. 16000 / tau_min
BETA_LOW, BETA_HIGH = 0.5, 2.0               # formant ratios: q = r / beta stays in the [0.25, 4] the kernel takes
LIFTER_MAX = 64                              # sa_env_dim(3)
PHASES = ("griffin_lim", "vocoder")          # where the re-synthesis takes its phases from
CONTOUR_LOW, CONTOUR_HIGH = 0.0, 2.0         # contour_scale gamma: 0 a monotone voice, 1 the additive shift
SMOOTH_MAX = 8                               # sa_contour_dim(1)
F0_METHODS = ("yin", "viterbi")              # first dip under the threshold; a path through every frame's dips
F0_COSTS = ("voicing_cost", "switch_cost", "jump_cost", "lag_bias")
F0_COST_LOW, F0_COST_HIGH = 0.0, 4.0         # what sa_f0_viterbi takes

# one definition per option: its flag, its kind ("real", "count", "choice" or "bool"), its bounds (the constants above,
# which the classes' *_settings check against too) or choices, and what the command line says of a value outside
# them; fmt: how the refused value is shown
Option = collections.namedtuple("Option", "flag kind low high text fmt", defaults=("{}",))
OPTIONS = {
    "formant_ratio": Option("--formant_ratio", "real", BETA_LOW, BETA_HIGH, f"a factor between {BETA_LOW:g} and "
                            f"{BETA_HIGH:g} by which the formants are scaled"),
    "preserve_formants": Option("--preserve_formants", "bool", None, None, "true or false"),
    "lifter": Option("--lifter", "count", 1, LIFTER_MAX, f"a count of cepstral coefficients, 1 to {LIFTER_MAX}"),
    "phase": Option("--phase", "choice", PHASES, None, "griffin_lim (phases reconstructed by Griffin-Lim, the default) "
                    "or vocoder (the input's own phases carried through the stretch)"),
    "contour_scale": Option("--contour_scale", "real", CONTOUR_LOW, CONTOUR_HIGH, f"a factor between {CONTOUR_LOW:g} "
                            f"(a monotone voice) and {CONTOUR_HIGH:g} by which the F0 contour's excursions are scaled"),
    "contour_smooth": Option("--contour_smooth", "count", 0, SMOOTH_MAX, f"a half-width in frames, 0 to {SMOOTH_MAX}"),
    "f0_method": Option("--f0_method", "choice", F0_METHODS, None, "yin (the first dip of d' under the threshold, the "
                        "default) or viterbi (a path decoded through every frame's dips)"),
    "psola": Option("--psola", "bool", None, None, "true or false"),
    "target_hz": Option("--pitch_target_hz", "real", TARGET_LOW, TARGET_HIGH, f"a target between {TARGET_LOW:g} and "
                        f"{TARGET_HIGH:g} Hz, the range the F0 tracker covers", "{:g}"),
}


def gpu_only(who, t):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.SaHipError(f"{who} runs on the GPU only (no CPU fallback)")


def n_valid(lens, N, device):
    """round(lens N) in 0..N per row, fp64 on the device: the samples that count (the kernels take them as int32)"""
    return torch.round(lens.to(device).double() * N).clamp(0, N)


def padded_stft(wavs):
    """wavs [B, N] -> (wp, R): wavs zero-padded to the next multiple of the hop, contiguous, and vocoder.stft of it"""
    N = wavs.shape[1]
    Np = HOP * -(-N // HOP)
    wp = (torch.nn.functional.pad(wavs, (0, Np - N)) if Np != N else wavs).contiguous()
    return wp, vocoder.stft(wp)


def resynthesis(gl, R, ratio, Tout, S):
    """the waveform of magnitudes S [B, Tout, 201]: Griffin-Lim (``gl``) from random phases, or without one R's own
    phases carried through the stretch at ``ratio`` (pv_synth; S None: the plain stretch of |R|) and one inversion"""
    if gl is not None:
        return gl(S)
    w, tw, _ = vocoder.tables(R.device)
    return ops.gl_istft(ops.pv_synth(R, ratio, Tout, S), w, tw)


def f0_track(wav, threshold=0.15, method="yin", lens=None, N=None, **costs):
    """wav [B, N] (device, fp32) -> f0 [B, N // 160 + 1] in Hz, one value per Fbank frame, 0 where unvoiced.
    ``method="viterbi"`` decodes a path through every frame's d' dips instead of taking the first
    one under the threshold: sa_yin_f0's d' -> sa_f0_candidates -> sa_f0_viterbi.  ``lens`` [B] (relative lengths;
    None: every frame counts) cuts the decode at the frames of round(lens N) samples, 0 beyond them (N: the unpadded
    width when wav is padded); ``costs``: voicing_cost, switch_cost, jump_cost, lag_bias of ops.f0_viterbi."""
    method, costs = f0_settings("f0_track", method, costs)
    if method == "yin":
        return ops.yin_f0(wav, threshold)
    _, dprime = ops.yin_f0(wav, threshold, return_dprime=True)
    if lens is None:
        lens = torch.ones(wav.shape[0], dtype=torch.float32, device=wav.device)
    tau, q = ops.f0_candidates(dprime)
    return ops.f0_viterbi(dprime, tau, q, lens.to(wav.device, torch.float32).contiguous(),
                          wav.shape[1] if N is None else N, **costs)


def f0_settings(who, method, costs):
    """-> (method, costs as a dict of floats), or ValueError"""
    if method not in F0_METHODS:
        raise ValueError(f"{who}: f0_method {method!r}: one of {', '.join(F0_METHODS)} expected")
    costs = dict(costs or {})
    for key, value in costs.items():
        if key not in F0_COSTS:
            raise ValueError(f"{who}: unknown F0 cost {key!r}: {', '.join(F0_COSTS)} expected")
        if isinstance(value, bool) or not F0_COST_LOW <= float(value) <= F0_COST_HIGH:
            raise ValueError(f"{who}: {key} {value} in {F0_COST_LOW:g}..{F0_COST_HIGH:g} expected")
        costs[key] = float(value)
    if costs and method != "viterbi":
        raise ValueError(f"{who}: {next(iter(costs))} needs f0_method=\"viterbi\" (YIN has no path costs)")
    return method, costs


def stretched_frames(Tp, ratio):
    """T'_b = ceil((T_p - 1) r_b) + 1, from the fp32 ratio in fp64 as the kernel forms it"""
    return int(math.ceil((int(Tp) - 1) * float(ratio))) + 1


def envelope_settings(who, preserve_formants, formant_ratio, lifter, floor_rel, max_gain_db):
    """-> (beta or None, lifter, floor_rel, max_gain_db), or ValueError: what both classes take for the warp"""
    if preserve_formants and formant_ratio is not None:
        raise ValueError(f"{who}: preserve_formants means formant_ratio 1; give one of the two")
    beta = 1.0 if preserve_formants else (None if formant_ratio is None else float(formant_ratio))
    if beta is not None and not BETA_LOW <= beta <= BETA_HIGH:
        raise ValueError(f"{who}: formant_ratio {formant_ratio} in {BETA_LOW}..{BETA_HIGH} expected")
    if int(lifter) != lifter or not 1 <= int(lifter) <= LIFTER_MAX:
        raise ValueError(f"{who}: lifter {lifter} in 1..{LIFTER_MAX} expected")
    if not 0.0 < float(floor_rel) < 1.0:
        raise ValueError(f"{who}: floor_rel {floor_rel} in (0, 1) expected")
    if not float(max_gain_db) > 0.0:
        raise ValueError(f"{who}: max_gain_db {max_gain_db} > 0 expected")
    return beta, int(lifter), float(floor_rel), float(max_gain_db)


def phase_setting(who, phase):
    if phase not in PHASES:
        raise ValueError(f"{who}: phase {phase!r}: one of {', '.join(PHASES)} expected")
    return phase


def contour_settings(who, contour_scale, contour_smooth, phase, psola=False):
    """-> (gamma or None, smooth), or ValueError: the contour needs the vocoder's phases, or PSOLA"""
    if contour_scale is None:
        return None, int(contour_smooth)
    if phase != "vocoder" and not psola:
        raise ValueError(f"{who}: contour_scale needs phase=\"vocoder\" (Griffin-Lim with a contour is not built)")
    gamma = float(contour_scale)
    if not CONTOUR_LOW <= gamma <= CONTOUR_HIGH:
        raise ValueError(f"{who}: contour_scale {contour_scale} in {CONTOUR_LOW:g}..{CONTOUR_HIGH:g} expected")
    if isinstance(contour_smooth, bool) or int(contour_smooth) != contour_smooth or \
            not 0 <= int(contour_smooth) <= SMOOTH_MAX:
        raise ValueError(f"{who}: contour_smooth {contour_smooth} in 0..{SMOOTH_MAX} expected")
    return gamma, int(contour_smooth)


# what PitchNormalizer(psola=True) takes no value of but the default: the STFT path's settings
PSOLA_DEFAULTS = {"preserve_formants": False, "formant_ratio": None, "lifter": 30, "floor_rel": 1e-4,
                  "max_gain_db": 40.0, "phase": "griffin_lim"}


def psola_setting(who, psola, given):
    """-> psola, or ValueError when it is no bool or comes with a setting (``given``: a dict of those in
    PSOLA_DEFAULTS) of the path it replaces"""
    if not isinstance(psola, bool):
        raise ValueError(f"{who}: psola {psola!r}: True or False expected")
    for key, value in given.items():
        if psola and value != PSOLA_DEFAULTS[key]:
            raise ValueError(f"{who}: psola=True takes no {key}: the grains are moved, not altered, so the envelope is "
                             "already preserved and there is no phase to choose")
    return psola


class PitchNormalizer:
    """wavs [B, N] (device), relative lengths [B] -> wavs of the same shape whose voiced F0 has mean ~ target_hz;
    samples from round(lens_b N) on are zero.  ``last``: (ratio, mean f0, voiced frames) of the last batch, on
    the device.  ``formant_ratio`` beta (``preserve_formants=True``: 1) scales the spectral envelope by beta
    instead of by the pitch ratio; without either the envelope moves with the pitch and no warp is launched.
    ``phase="vocoder"`` carries the input's phases through the stretch instead of running Griffin-Lim: no iterations,
    no random numbers (n_iter, momentum and seed are then unused, and ``gl`` is None).  ``contour_scale`` gamma (needs
    ``phase="vocoder"``) moves the contour to target + gamma (f0 - mean) with a ratio per frame, smoothed by a triangle
    of half-width ``contour_smooth`` frames; ``last[0]`` is then the row's mean ratio.  None: one ratio per row.
    ``f0_method="viterbi"`` forms the track with the path decode instead of first-dip YIN, with
    ``f0_costs`` (a dict of voicing_cost, switch_cost, jump_cost, lag_bias) in place of its defaults.
    ``psola=True`` moves the pitch in the time domain instead: the grains between pitch marks are
    laid down again at the new spacing, which keeps the envelope and the duration by construction.  No STFT, no phase
    (``gl`` is None; n_iter, momentum and seed are unused), no device-to-host copy; ``contour_scale`` then needs no
    ``phase="vocoder"``, and ``preserve_formants``, ``formant_ratio``, ``phase`` and the envelope's settings are refused."""

    def __init__(self, target_hz=170.0, n_iter=32, momentum=0.99, seed=1, r_min=0.5, r_max=2.0, min_voiced=5,
                 threshold=0.15, preserve_formants=False, formant_ratio=None, lifter=30, floor_rel=1e-4,
                 max_gain_db=40.0, phase="griffin_lim", contour_scale=None, contour_smooth=2, f0_method="yin",
                 f0_costs=None, psola=False):
        self.psola = psola_setting("PitchNormalizer", psola, dict(
            preserve_formants=preserve_formants, formant_ratio=formant_ratio, lifter=lifter, floor_rel=floor_rel,
            max_gain_db=max_gain_db, phase=phase))
        self.f0_method, self.f0_costs = f0_settings("PitchNormalizer", f0_method, f0_costs)
        self.formant_ratio, self.lifter, self.floor_rel, self.max_gain_db = envelope_settings(
            "PitchNormalizer", preserve_formants, formant_ratio, lifter, floor_rel, max_gain_db)
        self.phase = phase_setting("PitchNormalizer", phase)
        self.contour_scale, self.contour_smooth = contour_settings("PitchNormalizer", contour_scale, contour_smooth,
                                                                   self.phase, self.psola)
        if not TARGET_LOW <= float(target_hz) <= TARGET_HIGH:
            raise ValueError(f"PitchNormalizer: target_hz {target_hz} in {TARGET_LOW:g}..{TARGET_HIGH:g} expected")
        if not R_LOW <= float(r_min) <= float(r_max) <= R_HIGH:
            raise ValueError(f"PitchNormalizer: {R_LOW} <= r_min {r_min} <= r_max {r_max} <= {R_HIGH} expected")
        self.target_hz, self.r_min, self.r_max = float(target_hz), float(r_min), float(r_max)
        self.min_voiced, self.threshold = int(min_voiced), float(threshold)
        self.gl = None
        if phase == "griffin_lim" and not self.psola:
            self.gl = vocoder.GriffinLim(n_iter=n_iter, momentum=momentum, seed=seed)
        self.last = None

    @torch.no_grad()
    def __call__(self, wavs, lens):
        gpu_only("PitchNormalizer", wavs)
        lens = lens.to(wavs.device, torch.float32).contiguous()
        if self.psola:
            return self.shift_psola(wavs, lens)
        if self.contour_scale is not None:
            return self.shift_contour(wavs, lens)
        f0 = self.track(wavs, lens)
        self.last = ops.pitch_ratio(f0, lens, wavs.shape[1], self.target_hz, self.r_min, self.r_max, self.min_voiced)
        return self.shift(wavs, lens, self.last[0])

    def track(self, wavs, lens, N=None):
        """the F0 track the ratios are formed from: f0_track with the object's method, threshold and costs (N: the
        unpadded width when wavs is padded)"""
        return f0_track(wavs, self.threshold, self.f0_method, lens, N, **self.f0_costs)

    @torch.no_grad()
    def shift_psola(self, wavs, lens):
        """the time-domain path: the track -> one ratio per row (pitch_ratio, as rho_q = rint(ratio
        2^16) in every frame) or one per frame (pitch_contour) -> psola_marks -> psola_plan -> psola_ola.  Everything
        stays on the device.  ``last`` as the other paths leave it."""
        B, N = wavs.shape
        wavs = wavs.contiguous()
        f0 = self.track(wavs, lens)
        T = f0.shape[1]
        if self.contour_scale is None:
            self.last = ops.pitch_ratio(f0, lens, N, self.target_hz, self.r_min, self.r_max, self.min_voiced)
            rho_q = torch.round(self.last[0].double() * ops.CT_RHO_ONE).to(torch.int32)[:, None].expand(B, T)
            rho_q = rho_q.contiguous()
        else:
            if T < 2:                                            # (ops.pitch_contour's bound, said before its division below)
                raise L.SaHipError(f"PitchNormalizer: contour_scale needs 2 frames, {HOP} samples or more; got {N}")
            rho_q, Q, _, mean, voiced = ops.pitch_contour(f0, lens, N, self.target_hz, self.contour_scale,
                                                          self.contour_smooth, self.r_min, self.r_max, self.min_voiced)
            self.last = ((Q[:, T - 1].double() / float((T - 1) * ops.CT_Q_ONE)).float(), mean, voiced)
        return ops.psola(wavs, f0, rho_q, n_valid(lens, N, wavs.device).to(torch.int32))

    @torch.no_grad()
    def shift_contour(self, wavs, lens):
        """the contour path: pad -> STFT, yin_f0 of the padded waveform -> pitch_contour [-> |R| ->
        env_warp_frames at q[b, t] = rho[b, t] / beta] -> pv_synth_map -> one gl_istft -> pitch_resample_map.
        ``last`` is (the row's mean ratio Q[T - 1] / ((T - 1) 2^17), mean f0, voiced frames)."""
        B, N = wavs.shape
        wp, R = padded_stft(wavs)
        f0 = self.track(wp, lens, N)
        rho_q, Q, Tq, mean, voiced = ops.pitch_contour(f0, lens, N, self.target_hz, self.contour_scale,
                                                       self.contour_smooth, self.r_min, self.r_max, self.min_voiced)
        T = f0.shape[1]
        self.last = ((Q[:, T - 1].double() / float((T - 1) * ops.CT_Q_ONE)).float(), mean, voiced)
        M = None
        if self.formant_ratio is not None:                   # on the input grid: the frame's own ratio is known there
            one = torch.ones(B, dtype=torch.float32, device=wavs.device)
            q = (rho_q.float() / (ops.CT_RHO_ONE * self.formant_ratio)).contiguous()
            M = ops.env_warp_frames(ops.pitch_stretch_mag(R, one, T), q, self.lifter, self.floor_rel,
                                    self.max_gain_db)
        Tout = int(Tq.max())                                 # the path's one synchronisation: T' is a shape
        w, tw, _ = vocoder.tables(wavs.device)
        y = ops.gl_istft(ops.pv_synth_map(R, rho_q, Q, Tout, M), w, tw)
        return ops.pitch_resample_map(y, rho_q, Q, n_valid(lens, N, wavs.device).to(torch.int32), N)

    @torch.no_grad()
    def shift(self, wavs, lens, ratio):
        """the stretch, the phase reconstruction and the resampling with a given ratio (fp32 [B], device)"""
        gpu_only("PitchNormalizer", wavs)
        N = wavs.shape[1]
        host = ratio.detach().cpu().tolist()                 # the path's one synchronisation: T' is a shape
        if not all(R_LOW <= r <= R_HIGH for r in host):
            raise L.SaHipError(f"PitchNormalizer.shift: ratios in [{R_LOW}, {R_HIGH}] expected, got {host}")
        _, R = padded_stft(wavs)
        Tout = max(stretched_frames(R.shape[1], r) for r in host)
        S = None                                             # (the vocoder path forms the plain stretch itself)
        if self.gl is not None or self.formant_ratio is not None:
            S = ops.pitch_stretch_mag(R, ratio, Tout)
        if self.formant_ratio is not None:                   # q_b = r_b / beta, formed on the device
            q = (ratio.float() / self.formant_ratio).contiguous()
            S = ops.env_warp(S, q, self.lifter, self.floor_rel, self.max_gain_db)
        y = resynthesis(self.gl, R, ratio, Tout, S)
        return ops.pitch_resample(y, ratio, n_valid(lens, N, wavs.device).to(torch.int32), N)


class FormantShifter:
    """wavs [B, N] (device), relative lengths [B] -> wavs of the same shape whose spectral envelope is scaled along
    frequency by ``formant_ratio`` while the pitch stays: |STFT| -> sa_env_warp at q = 1 / beta -> Griffin-Lim.  No
    stretch, no resampling, no tracker, and no device-to-host copy.  Samples from round(lens_b N) on are zero.
    ``phase="vocoder"`` keeps the input's phases under the warped magnitudes (sa_pv_synth at ratio 1) and inverts
    once, instead of running Griffin-Lim (``gl`` is then None)."""

    def __init__(self, formant_ratio, n_iter=32, momentum=0.99, seed=1, lifter=30, floor_rel=1e-4, max_gain_db=40.0,
                 phase="griffin_lim"):
        if formant_ratio is None:
            raise ValueError("FormantShifter: formant_ratio expected")
        self.formant_ratio, self.lifter, self.floor_rel, self.max_gain_db = envelope_settings(
            "FormantShifter", False, formant_ratio, lifter, floor_rel, max_gain_db)
        self.phase = phase_setting("FormantShifter", phase)
        self.gl = vocoder.GriffinLim(n_iter=n_iter, momentum=momentum, seed=seed) if phase == "griffin_lim" else None

    @torch.no_grad()
    def __call__(self, wavs, lens):
        gpu_only("FormantShifter", wavs)
        B, N = wavs.shape
        _, R = padded_stft(wavs)
        one = torch.ones(B, dtype=torch.float32, device=wavs.device)
        S = ops.pitch_stretch_mag(R, one, R.shape[1])        # |R| exactly: the stretch at ratio 1
        S = ops.env_warp(S, one / self.formant_ratio, self.lifter, self.floor_rel, self.max_gain_db)
        y = resynthesis(self.gl, R, one, R.shape[1], S)[:, :N]
        # (the fp64 counts and a torch.where, on purpose: the other paths hand int32 counts to their resampling kernel)
        live = torch.arange(N, device=wavs.device)[None, :] < n_valid(lens, N, wavs.device)[:, None]
        return torch.where(live, y, torch.zeros((), dtype=y.dtype, device=y.device)).contiguous()


def given_options(keys, settings, block=None):
    """the options ``keys`` as the top-level settings give them, else the recipe's block (if any) -> a dict, in the
    order of ``keys``, of those that were given"""
    block = block or {}
    return {k: v for k in keys for v in (settings.get(k, block.get(k)),) if v is not None}


def check_option(key, value, options=OPTIONS):
    """``value`` of the option ``key`` -> as the classes take it (a float where it is real), or the option's one line;
    options: the table its row is in"""
    o = options[key]
    if o.kind == "bool":
        ok = isinstance(value, bool)
    elif o.kind == "choice":
        ok = isinstance(value, str) and value in o.low
    elif o.kind == "count":
        ok = not isinstance(value, bool) and isinstance(value, int) and o.low <= value <= o.high
    else:
        try:
            real = float(value)
        except (TypeError, ValueError):
            real = float("nan")
        # (--formant_ratio true has always read as 1; --contour_scale true is refused)
        ok = o.low <= real <= o.high and not (isinstance(value, bool) and key != "formant_ratio")
    if not ok:
        raise SystemExit(f"{o.flag} {o.fmt.format(value)}: {o.text}")
    return value if o.kind != "real" else real


def refuse_run_modes(script, settings, run_opts, environ=None):
    """the two run modes no waveform or recon recipe of the gender classifier has, one line each"""
    import os
    environ = os.environ if environ is None else environ
    if run_opts.get("distributed_launch") or int(environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{script} runs on one GPU: data parallelism is not implemented for it")
    if run_opts.get("hip_graph") or settings.get("hip_graph"):   # (from the command line it arrives as a setting)
        raise SystemExit(f"{script} does not support --hip_graph")


def check_formant_options(settings, block=None):
    """the envelope settings of a recipe's ``pitch_norm:`` block (if any) under the top-level overrides ->
    a dict of the keys that were given (preserve_formants, formant_ratio, lifter), each refused in one line"""
    given = given_options(("preserve_formants", "formant_ratio", "lifter"), settings, block)
    for key in ("preserve_formants", "formant_ratio"):
        if key in given:
            given[key] = check_option(key, given[key])
    if "formant_ratio" in given and given.get("preserve_formants"):
        raise SystemExit("--preserve_formants true and --formant_ratio exclude each other: preserving the "
                         "formants is formant_ratio 1")
    if "lifter" in given:
        check_option("lifter", given["lifter"])
    return given


def check_phase_option(settings, block=None):
    """the ``phase`` of a recipe's ``pitch_norm:`` block (if any) under the top-level override -> a dict that carries
    the key only when it was given; anything but griffin_lim and vocoder is refused in one line"""
    return {k: check_option(k, v) for k, v in given_options(("phase",), settings, block).items()}


def check_f0_option(settings, block=None):
    """the ``f0_method`` of a recipe's ``pitch_norm:`` block (if any) under the top-level override -> a dict that
    carries the key only when it was given; anything but yin and viterbi is refused in one line"""
    return {k: check_option(k, v) for k, v in given_options(("f0_method",), settings, block).items()}


def check_psola_option(settings, block=None):
    """the ``psola`` of a recipe's ``pitch_norm:`` block (if any) under the top-level override -> a dict that carries
    the key only when it was given; anything but true and false is refused in one line, and so is ``psola: true`` next
    to a setting of the STFT path it replaces (``phase`` with any value, ``preserve_formants: true``, ``formant_ratio``,
    ``lifter``)"""
    given = {k: check_option(k, v) for k, v in given_options(("psola",), settings, block).items()}
    if given.get("psola"):
        other = given_options(("phase", "preserve_formants", "formant_ratio", "lifter"), settings, block)
        if other.get("preserve_formants") is False:
            del other["preserve_formants"]
        for key in other:
            why = "there is no phase to choose" if key == "phase" else "the envelope is already preserved"
            raise SystemExit(f"--psola true and {OPTIONS[key].flag} exclude each other: the grains are moved, not "
                             f"altered, so {why}")
    return given


def check_contour_options(settings, block=None):
    """``contour_scale`` and ``contour_smooth`` of a recipe's ``pitch_norm:`` block (if any) under the top-level
    overrides -> a dict that carries a key only when it was given; each is refused in one line when out of range or
    given without ``phase: vocoder`` or ``psola: true``"""
    given = given_options(("contour_scale", "contour_smooth"), settings, block)
    if given and given_options(("phase",), settings, block).get("phase") != "vocoder" and \
            given_options(("psola",), settings, block).get("psola") is not True:
        raise SystemExit(f"--{next(iter(given))} needs --phase vocoder: the contour is moved on the phase-vocoder path "
                         "only")
    for key in given:
        given[key] = check_option(key, given[key])
    if "contour_smooth" in given and "contour_scale" not in given:
        raise SystemExit("--contour_smooth needs --contour_scale: there is no contour to smooth without it")
    return given


def check_pitch_target(value):
    return check_option("target_hz", float(value))


def check_pitch_options(settings, run_opts, environ=None):
    """what gender_classifier_train_pitch_norm.py refuses before anything touches a GPU, one line each"""
    pn = settings.get("pitch_norm") or {}
    target = check_pitch_target(settings.get("pitch_target_hz", pn.get("target_hz", 170.0)))
    r_min, r_max = float(pn.get("r_min", R_LOW)), float(pn.get("r_max", R_HIGH))
    if r_min < R_LOW or r_max > R_HIGH:
        raise SystemExit(f"pitch_norm: r_min {r_min:g} and r_max {r_max:g} must lie in [{R_LOW}, {R_HIGH}], the "
                         "ratios the kernels take")
    if r_min > r_max:
        raise SystemExit(f"pitch_norm: r_min {r_min:g} is above r_max {r_max:g}")
    refuse_run_modes("gender_classifier_train_pitch_norm", settings, run_opts, environ)
    return dict(pn, target_hz=target, r_min=r_min, r_max=r_max, **check_formant_options(settings, pn),
                **check_phase_option(settings, pn), **check_contour_options(settings, pn),
                **check_f0_option(settings, pn), **check_psola_option(settings, pn))
