"""Host side of the spectral envelope and the formant warp (speech_anonymization_amd.pitchnorm, csrc/sa_envelope.hip;
DESIGN section 16): the fp64 restatement of tests/formant_ref.py against the FFT and against closed forms, its edge
cases, the inputs of the GPU test, the refusals of the recipes, the entry point's -EINVAL answers and the refusal of
CPU tensors.  No GPU."""
import ctypes
import errno
import math
import os

import numpy as np
import pytest
import torch

from tests import formant_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _log_spectrum_of(c):
    """L_k = c_0 + 2 sum_{n >= 1} c_n cos(n w_k): the log spectrum whose cepstrum is c (n <= len(c) - 1 < 200)"""
    return F.envelope_at(torch.as_tensor(c, dtype=torch.float64)[None], F.COS_NK[:len(c)])[0]


def test_cepstrum_is_the_fft_of_the_even_extension():
    g = torch.Generator().manual_seed(5)
    L = torch.randn(4, F.K, generator=g, dtype=torch.float64) * 3.0 - 2.0
    even = torch.cat([L, L[:, 1:F.K - 1].flip(-1)], dim=-1)                # 400 values, L[400 - k] = L[k]
    assert even.shape[-1] == F.N_FFT
    fft = torch.fft.fft(even, dim=-1)
    assert float(fft.imag.abs().max()) < 1e-11
    for n_c in (1, 30, 64):
        c = F.cepstrum(L, n_c)
        assert c.shape == (4, n_c + 1)
        assert float((c - fft.real[:, :n_c + 1] / F.N_FFT).abs().max()) <= 1e-12


def test_known_cepstrum_comes_back_with_the_closed_form_gain():
    """L built from c_n, n <= n_c: the lifter passes all of it, so E == L, and the gain at q is L's own closed form
    read at q w_k minus L"""
    g = torch.Generator().manual_seed(6)
    n_c = 30
    c = torch.randn(n_c + 1, generator=g, dtype=torch.float64) * 0.2
    c[0] = -1.0
    S = torch.exp(_log_spectrum_of(c)).float()[None, None]                  # the kernel's input is fp32
    q = torch.tensor([1.37], dtype=torch.float32)
    w = F.warp(S, q, n_c=n_c, floor_rel=1e-6, max_gain_db=200.0)
    assert float((w.c[0, 0] - c).abs().max()) <= 2e-7                      # S was rounded to fp32: relative 6e-8
    assert float((w.env - w.L).abs().max()) <= 2e-7                        # (the rounded S is not band-limited)
    x = (float(q[0]) * torch.arange(F.K, dtype=torch.float64) / 200.0).clamp(max=1.0)
    closed = c[0] + 2.0 * sum(c[n] * torch.cos(n * math.pi * x) for n in range(1, n_c + 1)) - _log_spectrum_of(c)
    assert float((w.g_raw[0, 0] - closed).abs().max()) <= 1e-5             # 2 sum |c_n| n_c x the 2e-7 above
    assert float((w.out[0, 0] - S[0, 0].double() * torch.exp(closed)).abs().max()) <= 1e-5


def test_all_zero_frames_stay_zero():
    S = F.kernel_case(2, 9, zero_row=1)
    w = F.warp(S, torch.tensor([2.0, 0.5]), n_c=30)
    assert bool((w.out[1] == 0).all()) and float(w.g[1].abs().max()) <= 1e-12
    assert bool((w.L[1] == math.log(F.TINY)).all())
    zero_frames = ~S[0].bool().any(-1)
    assert int(zero_frames.sum()) >= 2 and bool((w.out[0][zero_frames] == 0).all())
    assert bool(torch.isfinite(w.out).all()) and bool(torch.isfinite(w.env).all())


def test_q_one_copies_and_bad_q_is_taken_as_documented():
    S = F.kernel_case(3, 4)
    w = F.warp(S, torch.tensor([1.0, float("nan"), 1.0]))
    assert torch.equal(w.out, S.double()) and float(w.g_raw.abs().max()) <= 1e-12
    assert F.sanitize_q(torch.tensor([0.1, 0.25, 1.37, 4.0, 9.0, float("nan"), float("inf"), -1.0])).tolist() == \
        [0.25, 0.25, float(np.float32(1.37)), 4.0, 4.0, 1.0, 4.0, 0.25]
    a, b = F.warp(S, torch.tensor([9.0, 0.1, 4.0])), F.warp(S, torch.tensor([4.0, 0.25, 4.0]))
    assert torch.equal(a.out, b.out)


def test_warp_beyond_pi_reads_the_envelope_at_nyquist():
    S = F.kernel_case(1, 4)
    w = F.warp(S, torch.tensor([2.0]))
    x = F.theta_over_pi(torch.tensor([2.0]))[0]
    assert bool((x[100:] == 1.0).all()) and float(x[99]) < 1.0
    at_pi = w.env[..., 200:201]
    assert float((w.env_t[..., 100:] - at_pi).abs().max()) <= 1e-12        # E(pi) from bin 100 on
    assert float((w.env_t[..., :101:1] - w.env[..., :201:2]).abs().max()) <= 1e-12   # q = 2 reads every second bin


def test_clamp_and_bars():
    """the clamp holds and is reached (the six-decade and the one-bin frames drive the unclamped gain to 1.5 times the
    default limit), the bars are positive and small against the quantities they bound, and the inputs of the GPU test
    leave no element out: its clamp decision is stable everywhere"""
    hit, far = 0, 0.0
    for (B, T, q, zero_row) in F.GPU_CASES:
        S = F.kernel_case(B, T, zero_row)
        for n_c in (1, 30, 64):
            w = F.warp(S, torch.tensor(q), n_c=n_c)
            assert float(w.g.abs().max()) <= w.limit and not bool(w.unstable.any()), (B, T, n_c)
            assert 0 < float(w.env_bar.min()) and float(w.env_bar.max()) < 0.05
            assert 0 < float(w.out_bar.min()) and float(w.out_bar.max()) < 0.1
            hit += int((w.g_raw.abs() > w.limit).sum())
            far = max(far, float(w.g_raw.abs().max()) / w.limit)
    print(f"{hit} elements clamped over the twelve cases; largest |g| / limit {far:.2f}")
    assert hit >= 100 and far >= 1.4


def test_resonance_rows_and_envelope_peak():
    """the end-to-end rows: full scale under 0.9, and the envelope peak finds each resonance within a harmonic
    spacing; the restatement's tracker finds each fundamental"""
    wav = F.resonance_rows()
    assert wav.shape == (3, 8000) and float(wav.abs().max()) < 0.9
    peak = F.envelope_peak(wav)
    f0, share = F.voiced_f0(wav)
    for (f, res), p, m in zip(F.ROWS, peak.tolist(), f0.tolist()):
        assert abs(p - res) <= f / 2 and abs(m - f) <= 0.5, (f, res, p, m)
    assert float(share.min()) >= 0.9


GOOD = {"pitch_norm": {"target_hz": 170.0, "r_min": 0.5, "r_max": 2.0}}


@pytest.mark.parametrize("change,word", [
    ({"preserve_formants": "yes"}, "--preserve_formants"),
    ({"preserve_formants": 1}, "--preserve_formants"),
    ({"formant_ratio": 0.4}, "--formant_ratio"),
    ({"formant_ratio": 2.5}, "--formant_ratio"),
    ({"formant_ratio": "wide"}, "--formant_ratio"),
    ({"formant_ratio": float("nan")}, "--formant_ratio"),
    ({"preserve_formants": True, "formant_ratio": 1.2}, "exclude"),
    ({"pitch_norm": {"preserve_formants": True, "formant_ratio": 1.2}}, "exclude"),
    ({"lifter": 0}, "--lifter"),
    ({"lifter": 65}, "--lifter"),
    ({"lifter": 30.5}, "--lifter"),
    ({"pitch_norm": {"lifter": 100}}, "--lifter"),
])
def test_check_pitch_options_refuses_formant_settings_in_one_line(change, word):
    from speech_anonymization_amd import pitchnorm
    with pytest.raises(SystemExit) as e:
        pitchnorm.check_pitch_options(dict(GOOD, **change), {}, {})
    msg = str(e.value)
    assert word in msg and "\n" not in msg


def test_check_pitch_options_carries_the_new_keys_only_when_given():
    from speech_anonymization_amd import pitchnorm
    base = {"target_hz": 170.0, "r_min": 0.5, "r_max": 2.0}
    assert pitchnorm.check_pitch_options(dict(GOOD), {}, {}) == base
    assert pitchnorm.check_pitch_options(dict(GOOD, preserve_formants=True), {}, {}) == dict(base, preserve_formants=True)
    assert pitchnorm.check_pitch_options(dict(GOOD, formant_ratio=1.2, lifter=24), {}, {}) == \
        dict(base, formant_ratio=1.2, lifter=24)
    block = {"pitch_norm": {"target_hz": 170.0, "preserve_formants": True, "lifter": 20}}
    assert pitchnorm.check_pitch_options(block, {}, {}) == dict(base, preserve_formants=True, lifter=20)
    # the command line wins over the block
    assert pitchnorm.check_pitch_options(dict(block, preserve_formants=False, formant_ratio=0.9), {}, {}) == \
        dict(base, preserve_formants=False, formant_ratio=0.9, lifter=20)
    for pn in (dict(base, preserve_formants=True), dict(base, formant_ratio=1.2, lifter=24)):
        norm = pitchnorm.PitchNormalizer(**pn)
        assert norm.formant_ratio == pn.get("formant_ratio", 1.0) and norm.lifter == pn.get("lifter", 30)
    assert pitchnorm.PitchNormalizer().formant_ratio is None


def test_recipe_arguments_reach_the_options(tmp_path):
    from speech_anonymization_amd import pitchnorm
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml, parse_arguments
    fn = os.path.join(ROOT, "speechbrain_configs", "gender_classifier_pitch_norm.yaml")
    _, run_opts, overrides = parse_arguments([fn, "--preserve_formants", "true", "--output_folder", str(tmp_path)])
    with open(fn) as f:
        pn = pitchnorm.check_pitch_options(load_hyperpyyaml(f, overrides), run_opts, {})
    assert pn["preserve_formants"] is True and "formant_ratio" not in pn and "lifter" not in pn
    _, run_opts, overrides = parse_arguments([fn, "--formant_ratio", "1.15", "--output_folder", str(tmp_path)])
    with open(fn) as f:
        pn = pitchnorm.check_pitch_options(load_hyperpyyaml(f, overrides), run_opts, {})
    assert pn["formant_ratio"] == 1.15 and "preserve_formants" not in pn


@pytest.mark.parametrize("kw", [
    dict(preserve_formants=True, formant_ratio=1.0), dict(formant_ratio=0.49), dict(formant_ratio=2.01),
    dict(formant_ratio=float("nan")), dict(lifter=0), dict(lifter=65), dict(lifter=2.5), dict(floor_rel=0.0),
    dict(floor_rel=1.0), dict(max_gain_db=0.0),
])
def test_constructors_refuse_bad_envelope_settings(kw):
    from speech_anonymization_amd import pitchnorm
    with pytest.raises(ValueError):
        pitchnorm.PitchNormalizer(**kw)
    if "preserve_formants" not in kw:
        with pytest.raises(ValueError):
            pitchnorm.FormantShifter(**dict({"formant_ratio": 1.2}, **kw))
    with pytest.raises(ValueError):
        pitchnorm.FormantShifter(None)


SHIFT = {"model_type": None, "out_dir": "/tmp/out", "synthetic": 4, "formant_ratio": 1.15}
NORM = {"model_type": "fcae", "out_dir": "/tmp/out", "synthetic": 4, "pitch_norm": True}


@pytest.mark.parametrize("settings,word", [
    (dict(SHIFT, passthrough=True), "--passthrough"),
    (dict(SHIFT, recon_ckpt="/some/CKPT+x"), "--recon_ckpt"),
    (dict(SHIFT, formant_ratio=3.0), "--formant_ratio"),
    (dict(SHIFT, out_dir=None), "--out_dir"),
    (dict(SHIFT, hip_graph=True), "hip_graph"),
    (dict(SHIFT, lifter=0), "--lifter"),
    (dict(SHIFT, formant_ratio=None, model_type="fcae", preserve_formants=True), "--pitch_norm"),
    (dict(SHIFT, formant_ratio=None, model_type="fcae", recon_ckpt="/x", lifter=20), "--lifter"),
    (dict(NORM, preserve_formants=True, formant_ratio=1.1), "exclude"),
    (dict(NORM, preserve_formants=True, passthrough=True), "--passthrough"),
    (dict(NORM, preserve_formants=True, recon_ckpt="/x"), "--recon_ckpt"),
])
def test_check_anonymize_options_formant_branches(settings, word):
    from speech_anonymization_amd import vocoder
    with pytest.raises(SystemExit) as e:
        vocoder.check_anonymize_options(settings, {}, {})
    msg = str(e.value)
    assert word in msg and "\n" not in msg


def test_check_anonymize_options_lets_the_formant_modes_through_and_keeps_its_wording():
    from speech_anonymization_amd import vocoder
    vocoder.check_anonymize_options(dict(SHIFT), {"device": "cuda:0"}, {})
    vocoder.check_anonymize_options(dict(SHIFT, report_f0=True, lifter=24), {}, {})
    vocoder.check_anonymize_options(dict(NORM, preserve_formants=True, report_f0=True), {}, {})
    vocoder.check_anonymize_options(dict(NORM, formant_ratio=0.9, model_type=None), {}, {})
    with pytest.raises(SystemExit, match="unknown model_type None: the anonymiser is one of convae, fcae and endtoend"):
        vocoder.check_anonymize_options(dict(SHIFT, formant_ratio=None), {}, {})
    with pytest.raises(SystemExit, match="--pitch_norm true and --passthrough true exclude each other"):
        vocoder.check_anonymize_options(dict(NORM, passthrough=True), {}, {})
    with pytest.raises(SystemExit, match="--recon_ckpt DIR is required without --passthrough true"):
        vocoder.check_anonymize_options(dict(NORM, pitch_norm=False), {}, {})


def test_env_dim_exports_the_constants():
    from speech_anonymization_amd import _lib, ops, pitchnorm
    lib = _lib.load()
    assert [lib.sa_env_dim(i) for i in range(5)] == [400, 201, 8, 64, 256]
    assert lib.sa_env_dim(5) == -errno.EINVAL and lib.sa_env_dim(-1) == -errno.EINVAL
    assert (F.N_FFT, F.K, F.NC_MAX) == (400, 201, 64) and ops.ENV_NC_MAX == pitchnorm.LIFTER_MAX == 64
    assert ops.LN10_OVER_20 == F.LN10_OVER_20 == math.log(10.0) / 20.0


def test_entry_point_refuses_bad_arguments():
    """-EINVAL before any launch.  The pointers are host buffers nothing dereferences."""
    from speech_anonymization_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p, f, E = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_float, -errno.EINVAL

    def warp(S=p, q=p, B=2, T=9, n_c=30, floor_rel=1e-4, lim=4.6, out=p, env=None):
        return lib.sa_env_warp(S, q, B, T, n_c, f(floor_rel), f(lim), out, env, None)

    for bad in (dict(S=None), dict(q=None), dict(out=None), dict(B=0), dict(B=-1), dict(B=65536), dict(T=0),
                dict(T=-3), dict(T=(1 << 23) + 1), dict(n_c=0), dict(n_c=65), dict(n_c=-1), dict(floor_rel=0.0),
                dict(floor_rel=1.0), dict(floor_rel=-0.1), dict(floor_rel=float("nan")), dict(lim=0.0),
                dict(lim=-1.0), dict(lim=float("nan"))):
        assert warp(**bad) == E, bad


def test_ops_and_classes_refuse_cpu_tensors_before_loading_anything(monkeypatch):
    from speech_anonymization_amd import _lib, ops, pitchnorm
    from speech_anonymization_amd._lib import SaHipError

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(SaHipError, match="GPU"):
        ops.env_warp(torch.zeros(1, 4, 201), torch.ones(1))
    with pytest.raises(SaHipError, match="GPU"):
        pitchnorm.PitchNormalizer(preserve_formants=True)(torch.zeros(1, 500), torch.ones(1))
    with pytest.raises(SaHipError, match="GPU"):
        pitchnorm.PitchNormalizer(formant_ratio=1.2).shift(torch.zeros(1, 500), torch.ones(1), torch.ones(1))
    with pytest.raises(SaHipError, match="GPU"):
        pitchnorm.FormantShifter(1.2)(torch.zeros(1, 500), torch.ones(1))
