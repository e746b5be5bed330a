"""CPU checks of the F0-contour pitch modification: the restatement tests/contour_ref.py against
the constant-ratio restatements it generalises and against hand-made rows, the decision margins of the rows the GPU
test feeds the contour kernel, the claim (gamma 0 flattens the contour, the mean lands on the target) on the cases of
tools/contour_delta.py, and the options."""
import os

import pytest
import torch

from tests import contour_ref as Cr
from tests import phasevoc_ref as V
from tests import pitch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = (0.5, 1.0, 1.25, 2.0)


# ---------------------------------------------------------------------------------------------------
# the time map
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 5, 23])
def test_time_map_at_a_constant_ratio_is_the_old_stretch(T):
    for r in RATIOS:
        rho_q, Q, Tq = Cr.constant_tables(r, T)
        assert Q[0].tolist() == [int(t * r * Cr.Q_ONE) for t in range(T)]
        Tb, i, a = Cr.positions(rho_q[0], Q[0])
        Tb_old, i_old, a_old = V.positions(T, r)
        assert Tb == Tb_old == int(Tq[0]) == P.stretched_frames(T, r)
        assert torch.equal(i, i_old) and torch.equal(a, a_old.float().double())
        n = torch.arange((T - 1) * 160 + 7, dtype=torch.int64)
        ip, fr, r_loc = Cr.sample_positions(rho_q[0], Q[0], n)
        assert torch.equal(ip.double() + fr, n.double() * r) and bool((r_loc == r).all())


def test_time_map_of_a_moving_ratio():
    rho_q = torch.tensor([[1 << 16, 3 << 15, 1 << 17, 1 << 15]])           # 1, 1.5, 2, 0.5
    Q, Tq = Cr.time_map(rho_q)
    assert Q.tolist() == [[0, 5 << 15, 12 << 15, 17 << 15]] and int(Tq[0]) == 6      # 4.25 frames -> ceil + 1
    Tb, i, a = Cr.positions(rho_q[0], Q[0])
    assert Tb == 6 and i.tolist() == [0, 0, 1, 2, 2, 2]                     # X = 0, 4, 8, 12, 16, 20 (<< 15)
    want = [0.0, 4 / 5, (8 - 5) / 7, 0.0, (16 - 12) / 5, 1.0]
    assert a.tolist() == [float(torch.tensor(v, dtype=torch.float64).float()) for v in want]
    ip, fr, r_loc = Cr.sample_positions(rho_q[0], Q[0], torch.tensor([0, 159, 160, 320, 479, 500]))
    pos = (ip.double() + fr).tolist()
    assert pos[:4] == [0.0, 159 * 1.25, 200.0, 480.0] and r_loc.tolist()[:4] == [1.25, 1.25, 1.75, 1.25]
    assert pos[4] == 480.0 + 159 * 1.25 and pos[5] == 480.0 + 180 * 1.25   # beyond the last interval: its ratio holds


# ---------------------------------------------------------------------------------------------------
# the contour
# ---------------------------------------------------------------------------------------------------
def _voiced_row(T=40, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (120.0 + 60.0 * torch.rand(1, T, generator=g)).float()


def test_gamma_one_is_the_additive_shift_and_gamma_zero_the_flat_contour():
    f0 = _voiced_row()
    T = f0.shape[1]
    N = (T - 1) * 160
    mean = float(f0.double().mean())
    c = Cr.contour(f0, torch.ones(1), N, 170.0, 1.0, 0)
    assert int(c.voiced[0]) == T and abs(float(c.mean[0]) - mean) <= 1e-12 * mean
    g = c.raw[0] * f0[0].double()                                           # g = rho f~, f~ = f0 at s = 0
    assert bool((g - (f0[0].double() - mean + 170.0)).abs().max() <= 1e-10)
    c0 = Cr.contour(f0, torch.ones(1), N, 170.0, 0.0, 0)
    assert bool((c0.raw[0] - 170.0 / f0[0].double()).abs().max() <= 1e-14)
    assert torch.equal(c0.rho_q[0], torch.round(c0.raw[0] * 65536.0).long())
    c2 = Cr.contour(f0, torch.ones(1), N, 170.0, 0.0, 2)                    # smoothed: rho = target / f~
    ft = torch.from_numpy(Cr.smooth(f0[0].double().numpy(), 2))
    assert bool((c2.raw[0] - 170.0 / ft).abs().max() <= 1e-14)
    d = f0[0].double()
    assert abs(float(ft[0]) - float(3 * d[0] + 2 * d[0] + d[0] + 2 * d[1] + d[2]) / 9) <= 1e-12    # clamped at the ends


def test_fill_hold_cut_clamps_floor_and_min_voiced():
    f0 = torch.zeros(6, 12)
    f0[0, 3], f0[0, 7] = 100.0, 140.0                                       # hold, interpolate, hold
    fh = Cr.fill(f0[0].numpy(), 12)
    assert fh.tolist() == [100.0] * 4 + [110.0, 120.0, 130.0] + [140.0] * 5
    assert Cr.fill(f0[0].numpy(), 7).tolist() == [100.0] * 12               # frame 7 is beyond F_b: not voiced
    f0[1, :] = 150.0
    f0[1, 8:] = 300.0                                                       # beyond the cut of lens 0.6
    f0[2, 2:6] = 150.0                                                      # 4 voiced < 5
    f0[3, :] = torch.tensor([61.0, 62.0, 64.0, 70.0, 80.0, 100.0, 200.0, 300.0, 350.0, 380.0, 390.0, 399.0])
    f0[4, :] = f0[3]
    N = 11 * 160
    lens = torch.tensor([1.0, 0.6, 1.0, 1.0, 1.0, 1.0])
    c = Cr.contour(f0, lens, N, 170.0, 0.0, 0)
    assert c.voiced.tolist() == [2, 7, 4, 12, 12, 0] and c.moved.tolist() == [False, True, False, True, True, False]
    assert abs(float(c.mean[1]) - 150.0) <= 1e-12                           # round(0.6 N) = 1056 -> F_b = 7 frames
    assert c.rho_q[1].tolist() == [round(170.0 / 150.0 * 65536)] * 12       # ... and frame 6's value is held beyond
    for b in (0, 2, 5):                                                     # under min_voiced: ratio one
        assert c.rho_q[b].tolist() == [1 << 16] * 12 and int(c.Tq[b]) == 12
        assert c.Q[b].tolist() == [t << 17 for t in range(12)]
    assert c.rho_q[3, 0] == 1 << 17 and c.rho_q[3, -1] == 1 << 15           # both clamps
    assert float(c.raw[3, 0]) > 2.0 and float(c.raw[3, -1]) < 0.5
    assert bool((c.rho_q >= 1 << 15).all()) and bool((c.rho_q <= 1 << 17).all())
    c = Cr.contour(f0, lens, N, 170.0, 2.0, 0)                              # the floor: 170 + 2 (61 - mean) < 60
    assert float(c.raw[4, 0]) == 60.0 / 61.0 and c.rho_q[4, 0] == round(60.0 / 61.0 * 65536)
    c = Cr.contour(f0, lens, N, 170.0, 0.0, 0, min_voiced=2)
    assert c.moved.tolist() == [True, True, True, True, True, False]
    assert c.rho_q[0].tolist() == [round(170.0 * 65536 / v) for v in fh]
    c = Cr.contour(f0, lens, N, 170.0, 0.0, 0, r_min=0.8, r_max=1.25)
    assert c.rho_q[3, 0] == round(1.25 * 65536) and c.rho_q[3, -1] == round(0.8 * 65536)


def _pass_width():
    import __graft_entry__ as g
    g.build()
    from speech_anonymization_amd import _lib
    return _lib.load().sa_contour_dim(0)


def test_decision_margins_of_the_gpu_rows():
    """every row the GPU test feeds sa_pitch_contour: no 2^16 rho within 1e-6 of a half-integer before rint, no g / f~
    within 1e-9 of a clamp -- the kernel's fp64 may differ from this restatement's by a few ulp (an FMA, a division),
    1e-11 at 2^16, and must still decide alike.  None is left out."""
    W = _pass_width()
    assert W >= 64 and W % 64 == 0
    f0, lens, N = Cr.contour_rows(W)
    assert f0.shape == (8, 2 * W + 17)
    for gamma, s, r_min, r_max in Cr.CONTOUR_CALLS:
        c = Cr.contour(f0, lens, N, 170.0, gamma, s, r_min, r_max)
        assert c.moved.tolist() == [True, True, False, False, True, True, True, True]
        rint, clamp = Cr.margins(c, r_min, r_max)
        print(f"gamma {gamma:g}, smooth {s}, [{r_min}, {r_max}]: rint margin {rint:.3e}, clamp margin {clamp:.3e}")
        assert rint > 1e-6 and clamp > 1e-9
    c = Cr.contour(f0, lens, N, 170.0, 0.0, 2)
    assert bool((c.rho_q[5] == 1 << 17).any()) and bool((c.rho_q[5] == 1 << 15).any())       # both clamps active
    c = Cr.contour(f0, lens, N, 170.0, 2.0, 8)
    g = c.raw[6] * torch.from_numpy(Cr.smooth(Cr.fill(f0[6].double().numpy(), f0.shape[1]), 8))
    assert bool(((g - 60.0).abs() <= 1e-9).any()) and bool((g > 61.0).any())                  # the floor active
    assert int(c.voiced[4]) < int((f0[4] > 0).sum())                                         # the cut left frames out
    f2, l2, N2 = Cr.contour_rows_T2()
    for gamma, s, r_min, r_max in Cr.CONTOUR_CALLS:
        c = Cr.contour(f2, l2, N2, 170.0, gamma, s, r_min, r_max, min_voiced=1)
        assert c.moved.tolist() == [True, True, True, False, True, True, True, True]
        rint, clamp = Cr.margins(c, r_min, r_max)
        assert rint > 1e-6 and clamp > 1e-9


# ---------------------------------------------------------------------------------------------------
# the claim
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delta():
    import importlib.util
    spec = importlib.util.spec_from_file_location("contour_delta", os.path.join(ROOT, "tools", "contour_delta.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.main([])


def test_gamma_zero_flattens_the_contour_and_lands_on_the_target(delta):
    from tests.test_contour_gpu import REF_FIGURES
    mod, res = delta
    flat = res[0.0]
    for b, name in enumerate(("glide", "vibrato")):
        print(f"{name}: std {flat['std_in'][b]:.2f} -> {flat['std_out'][b]:.3f} Hz, |mean - 170| "
              f"{flat['mean_err'][b]:.3f} Hz; worst per-frame error at gamma 0.5 {res[0.5]['worst'][b]:.3f}, at 1 "
              f"{res[1.0]['worst'][b]:.3f} Hz")
        assert flat["std_out"][b] <= 0.25 * flat["std_in"][b]
        assert flat["mean_err"][b] <= 0.5
        assert min(res[g]["frames"][b] for g in res) >= 0.9 * (Cr.N_CASE // 160 + 1 - 2 * Cr.EDGE)
    # the figures the GPU test's bars are 4 x of are these, to the digits recorded there
    for key, g in (("std_out", 0.0), ("mean_err", 0.0), ("worst", 0.0), ("worst", 0.5), ("worst", 1.0)):
        for b in range(2):
            assert abs(res[g][key][b] - REF_FIGURES[(key, g)][b]) <= 5e-4 + 1e-3 * REF_FIGURES[(key, g)][b], (key, g, b)


def test_preserve_formants_figures_are_the_restatement_s(delta):
    """what decides that tests/test_contour_gpu.py asserts the envelope-peak condition: the restatement's own figures,
    recomputed here, against section 16's bar"""
    from tests.test_contour_gpu import REF_PRESERVE_MOVE, REF_PRESERVE_STD
    from tests.test_formant_gpu import PRESERVE_PEAK_BAR
    std_in, std, mean_err, move = delta[0].preserved(report=print)
    assert abs(std - REF_PRESERVE_STD) <= 5e-4 and abs(move - REF_PRESERVE_MOVE) <= 5e-3
    assert std <= 0.25 * std_in and mean_err <= 0.5
    assert move <= PRESERVE_PEAK_BAR


def test_steady_row_reproduces_the_constant_ratio_result():
    wav, lens = Cr.steady_row(), torch.ones(1)
    N = wav.shape[1]
    out, c, _ = Cr.normalize(wav, lens, 170.0, 1.0)
    got = float(P.voiced_mean(P.yin(out)[0], lens, N)[0])
    const = float(P.voiced_mean(P.yin(V.normalize(wav, lens)[0])[0], lens, N)[0])
    print(f"steady 140 Hz row: contour path {got:.4f} Hz, constant-ratio path {const:.4f} Hz")
    assert abs(got - 170.0) <= 0.05 and abs(got - const) <= 0.05


# ---------------------------------------------------------------------------------------------------
# options
# ---------------------------------------------------------------------------------------------------
def _one_line(fn, *args):
    with pytest.raises(SystemExit) as e:
        fn(*args)
    msg = str(e.value)
    assert msg and "\n" not in msg
    return msg


def test_check_contour_options():
    from speech_anonymization_amd.pitchnorm import check_contour_options as check
    assert check({}) == {} and check({}, {"r_min": 0.6}) == {} and check({"phase": "vocoder"}) == {}
    assert check({"phase": "vocoder", "contour_scale": 0}) == {"contour_scale": 0.0}
    assert check({"contour_scale": 0.5, "contour_smooth": 4}, {"phase": "vocoder"}) == {"contour_scale": 0.5,
                                                                                       "contour_smooth": 4}
    assert check({"phase": "vocoder"}, {"contour_scale": 1, "contour_smooth": 0}) == {"contour_scale": 1.0,
                                                                                      "contour_smooth": 0}
    assert check({"contour_scale": 2.0, "phase": "vocoder"}, {"contour_scale": 1.0}) == {"contour_scale": 2.0}
    for bad in (-0.1, 2.5, "flat", True, float("nan")):
        assert "--contour_scale" in _one_line(check, {"phase": "vocoder", "contour_scale": bad})
    for bad in (-1, 9, 1.5, True, "2"):
        assert "--contour_smooth" in _one_line(check, {"phase": "vocoder", "contour_scale": 1.0, "contour_smooth": bad})
    assert "needs --contour_scale" in _one_line(check, {"phase": "vocoder", "contour_smooth": 2})
    for settings in ({"contour_scale": 1.0}, {"contour_scale": 1.0, "phase": "griffin_lim"}, {"contour_smooth": 2}):
        assert "needs --phase vocoder" in _one_line(check, settings)


def test_normalizer_takes_the_contour_with_the_vocoder_only():
    from speech_anonymization_amd import pitchnorm
    pn = pitchnorm.PitchNormalizer()
    assert pn.contour_scale is None and pn.contour_smooth == 2
    pn = pitchnorm.PitchNormalizer(phase="vocoder", contour_scale=0, contour_smooth=4)
    assert pn.contour_scale == 0.0 and pn.contour_smooth == 4 and pn.gl is None
    with pytest.raises(ValueError, match="contour_scale needs phase") as e:
        pitchnorm.PitchNormalizer(contour_scale=1.0)
    assert "\n" not in str(e.value)
    for kw in (dict(contour_scale=2.1), dict(contour_scale=-1), dict(contour_scale=1, contour_smooth=9),
               dict(contour_scale=1, contour_smooth=1.5), dict(contour_scale=1, contour_smooth=-1)):
        with pytest.raises(ValueError, match="contour_"):
            pitchnorm.PitchNormalizer(phase="vocoder", **kw)
    with pytest.raises(pitchnorm.L.SaHipError, match="GPU only"):
        pitchnorm.PitchNormalizer(phase="vocoder", contour_scale=1.0)(torch.zeros(1, 800), torch.ones(1))


def test_committed_recipe_yields_the_old_options_and_carries_the_keys_only_when_given():
    from speech_anonymization_amd import pitchnorm
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    path = os.path.join(ROOT, "speechbrain_configs", "gender_classifier_pitch_norm.yaml")

    def options(over):
        with open(path) as fin:
            return pitchnorm.check_pitch_options(load_hyperpyyaml(fin, over), {}, environ={})

    pn = options({})
    assert "contour_scale" not in pn and "contour_smooth" not in pn and "phase" not in pn
    assert options({"phase": "vocoder"}) == dict(pn, phase="vocoder")
    assert options({"phase": "vocoder", "contour_scale": 0.0}) == dict(pn, phase="vocoder", contour_scale=0.0)
    assert options({"phase": "vocoder", "contour_scale": 1, "contour_smooth": 3}) == dict(
        pn, phase="vocoder", contour_scale=1.0, contour_smooth=3)
    pitchnorm.PitchNormalizer(**options({"phase": "vocoder", "contour_scale": 1, "contour_smooth": 3}))
    with open(path) as fin:
        settings = load_hyperpyyaml(fin, {"contour_scale": 1.0})
    assert "needs --phase vocoder" in _one_line(pitchnorm.check_pitch_options, settings, {}, {})


def test_anonymize_takes_the_contour_with_pitch_norm_and_the_vocoder_only():
    from speech_anonymization_amd.vocoder import check_anonymize_options as check
    base = {"out_dir": "o", "synthetic": 4, "model_type": "convae"}
    check(dict(base, pitch_norm=True, phase="vocoder", contour_scale=0.0), {}, {})
    check(dict(base, pitch_norm=True, phase="vocoder", contour_scale=1.0, contour_smooth=0, preserve_formants=True), {},
          {})
    for extra in ({"pitch_norm": True}, {"pitch_norm": True, "phase": "griffin_lim"}, {"recon_ckpt": "d"},
                  {"passthrough": True}, {"mcadams": 0.8}, {"formant_ratio": 1.15}):
        assert "needs --phase vocoder" in _one_line(check, dict(base, contour_scale=1.0, **extra), {}, {})
    assert "goes with --pitch_norm true" in _one_line(check, dict(base, contour_scale=1.0, phase="vocoder",
                                                                  formant_ratio=1.15), {}, {})
    assert "--contour_scale 3" in _one_line(check, dict(base, pitch_norm=True, phase="vocoder", contour_scale=3), {}, {})
    # earlier refusals keep their wording
    old = _one_line(check, dict(base, pitch_norm=True, passthrough=True), {}, {})
    assert old.startswith("--pitch_norm true and --passthrough true exclude each other")
