"""The phase-vocoder resynthesis on the CPU: the fp64 restatement of tests/phasevoc_ref.py against
the properties that define it -- the identity at ratio 1, the textbook form, a stationary sinusoid, the F0 claim --
and the option plumbing.  No GPU, no library call."""
import math
import os

import pytest
import torch

from tests import phasevoc_ref as V
from tests import pitch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = (0.5, 1.37, 2.0)


@pytest.fixture(scope="module")
def rows():
    """three harmonic rows of 0.3 s (N a multiple of the hop) and their STFT: computed once, left unchanged"""
    g = torch.Generator().manual_seed(19)
    wav = torch.stack([P.harmonic_row(f, 4800, g) for f in (103.0, 170.0, 248.0)])
    return wav, P.stft(wav)


def test_ratio_one_returns_the_input(rows):
    wav, R = rows
    one = [1.0] * 3
    C, phi, S, Tb = V.pv_synth(R, one)
    err = float((C - R).abs().max() / R.abs().max())
    back = float((V.shift(wav, torch.ones(3), one) - wav).abs().max())
    print(f"ratio 1: max |C - R| / max |R| = {err:.2e}; the whole path returns its input within {back:.2e}")
    assert Tb == [R.shape[1]] * 3 and C.shape == R.shape
    assert err <= 1e-12 and back <= 1e-12


@pytest.mark.parametrize("r", RATIOS)
def test_step_three_is_the_textbook_phase_vocoder(rows, r):
    """theta[i + 1] - theta[i] against Omega_k + wrap(theta[i + 1] - theta[i] - Omega_k), Omega_k = 0.4 k turns, and
    against another summation order"""
    _, R = rows
    plain = V.pv_phase(R, [r] * 3)
    d_text = float(V.circular(plain, V.pv_phase(R, [r] * 3, form="textbook")).max())
    d_order = float(V.circular(plain, V.pv_phase(R, [r] * 3, order="cumsum")).max())
    print(f"r = {r}: {plain.shape[1]} frames; textbook form within {d_text:.2e} turns, cumulative sum within "
          f"{d_order:.2e}")
    assert plain.shape[1] == P.stretched_frames(R.shape[1], r)
    assert bool((plain >= 0).all()) and bool((plain <= 1).all())
    assert d_text <= 1e-11 and d_order <= 1e-11


@pytest.mark.parametrize("r", RATIOS)
def test_stationary_sinusoid_keeps_its_frequency_through_the_stretch(r):
    """180 Hz lies half-way between the centres of bins 4 and 5 (40 Hz apart): after the stretch and the inversion
    it is still 180 Hz (over r times the duration), after the resampling r 180 Hz"""
    f, N = 180.0, 8000
    wav = 0.5 * torch.sin(2.0 * math.pi * f * torch.arange(N, dtype=torch.float64) / P.SR)[None, :]
    C = V.pv_synth(P.stft(wav), [r])[0]
    y = P.istft(C)
    assert y.shape[1] == (P.stretched_frames(N // 160 + 1, r) - 1) * 160
    out = P.resample(y, [r], [N], N)[0]
    for sig, want in ((y, f), (out, r * f)):
        f0 = P.yin(sig)[0][0, 3:-3]                                        # (the edge frames see the zero padding)
        got = float(f0[f0 > 0].mean())
        print(f"r = {r}: {int((f0 > 0).sum())} of {f0.numel()} frames voiced, mean {got:.3f} Hz, expected {want:.3f}")
        assert int((f0 > 0).sum()) >= 0.9 * f0.numel()
        assert abs(got - want) <= 0.5


def test_f0_lands_closer_to_the_target_than_griffin_lim():
    """the cases of tools/phasevoc_delta.py against DELTA_WORST_HZ, what tools/pitch_norm_delta.py measured for the
    Griffin-Lim path on the same utterances"""
    from tests.test_pitchnorm_gpu import DELTA_WORST_HZ
    worst, share, spread = V.delta_cases(170.0)
    print(f"worst |mean - 170| = {worst:.4f} Hz (Griffin-Lim: {DELTA_WORST_HZ}); smallest voiced share {share:.3f}; "
          f"spread between two summation orders {spread:.2e} turns")
    assert worst < DELTA_WORST_HZ
    assert share > 0.9 and spread <= 1e-11


# ---------------------------------------------------------------------------------------------------
# options
# ---------------------------------------------------------------------------------------------------
def _one_line(fn, *args):
    with pytest.raises(SystemExit) as e:
        fn(*args)
    msg = str(e.value)
    assert msg and "\n" not in msg
    return msg


def test_check_phase_option():
    from speech_anonymization_amd import pitchnorm
    assert pitchnorm.check_phase_option({}) == {} and pitchnorm.check_phase_option({}, {"r_min": 0.6}) == {}
    for v in ("griffin_lim", "vocoder"):
        assert pitchnorm.check_phase_option({"phase": v}) == {"phase": v}
        assert pitchnorm.check_phase_option({}, {"phase": v}) == {"phase": v}
    assert pitchnorm.check_phase_option({"phase": "vocoder"}, {"phase": "griffin_lim"}) == {"phase": "vocoder"}
    for bad in ("world", True, 3):
        assert "griffin_lim" in _one_line(pitchnorm.check_phase_option, {"phase": bad})
    for cls, args in ((pitchnorm.PitchNormalizer, ()), (pitchnorm.FormantShifter, (1.15,))):
        with pytest.raises(ValueError, match="phase"):
            cls(*args, phase="world")
        assert cls(*args).phase == "griffin_lim" and cls(*args).gl is not None
        assert cls(*args, phase="vocoder").gl is None                       # no GriffinLim, no generator


def test_committed_recipe_yields_the_old_options():
    from speech_anonymization_amd import pitchnorm
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    path = os.path.join(ROOT, "speechbrain_configs", "gender_classifier_pitch_norm.yaml")
    with open(path) as fin:
        settings = load_hyperpyyaml(fin, {})
    pn = pitchnorm.check_pitch_options(settings, {}, environ={})
    assert "phase" not in pn
    with open(path) as fin:
        settings = load_hyperpyyaml(fin, {"phase": "vocoder"})
    assert pitchnorm.check_pitch_options(settings, {}, environ={}) == dict(pn, phase="vocoder")
    settings["phase"] = "world"
    assert "--phase world" in _one_line(pitchnorm.check_pitch_options, settings, {}, {})


def test_anonymize_refuses_the_vocoder_where_there_is_no_input_phase():
    from speech_anonymization_amd.vocoder import check_anonymize_options as check
    base = {"out_dir": "o", "synthetic": 4, "model_type": "convae"}
    for extra in ({"pitch_norm": True}, {"formant_ratio": 1.15}, {"pitch_norm": True, "preserve_formants": True},
                  {"pitch_norm": True, "formant_ratio": 0.9}):
        for v in ("vocoder", "griffin_lim"):
            check(dict(base, phase=v, **extra), {}, {})                     # accepted
    for extra in ({"recon_ckpt": "d"}, {"passthrough": True}, {"mcadams": 0.8},
                  {"pitch_norm": True, "passthrough": True}, {"formant_ratio": 1.15, "recon_ckpt": "d"}):
        assert "no input phase to carry" in _one_line(check, dict(base, phase="vocoder", **extra), {}, {})
    assert "--phase vocoder goes with" in _one_line(check, dict(base, phase="vocoder"), {}, {})
    assert "--phase world" in _one_line(check, dict(base, phase="world", pitch_norm=True), {}, {})
    # earlier refusals keep their wording, with and without the flag
    old = _one_line(check, dict(base, pitch_norm=True, passthrough=True), {}, {})
    assert old.startswith("--pitch_norm true and --passthrough true exclude each other")
    assert _one_line(check, dict(base, pitch_norm=True, passthrough=True, phase="griffin_lim"), {}, {}) == old
    check(dict(base, recon_ckpt="d", phase="griffin_lim"), {}, {})          # the default, named
