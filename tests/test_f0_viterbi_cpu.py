"""CPU checks of the Viterbi F0 tracker: the scenario claims on the restatement
tests/f0v_ref.py, the decode's properties on random integer candidates, the options, and the C entry points' refusals
(no launch is reached)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from speech_anonymization_amd.pitchnorm import F0_COSTS, F0_METHODS
from tests import f0v_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------
# the scenario claims
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenario():
    dp = R.dprime32(R.scenario_rows())
    assert dp.shape == (6, R.T_CASE, R.TAU_MAX + 1) and R.N_CASE == 160 * 39 + 37
    f0_v, path, tau, q = R.track(dp, np.ones(6), R.N_CASE)
    f0_y, lag = R.yin_f0(dp)
    return dp, f0_v, path, tau, q, f0_y, lag


def test_scenario_claims_on_the_restatement(scenario):
    _, f0_v, _, _, _, f0_y, _ = scenario
    R.check_scenarios(f0_v, f0_y, report=print)


def test_candidates_of_the_scenarios(scenario):
    dp, _, path, tau, q, _, lag = scenario
    live = tau >= 0
    assert bool((live[..., :-1] | ~live[..., 1:]).all())                   # the unused slots come last
    assert bool(((tau[..., 1:] > tau[..., :-1]) | ~live[..., 1:]).all())   # ascending lag
    assert bool((tau[~live] == -1).all()) and bool((q[~live] == 0).all())
    assert bool((tau[live] >= R.TAU_MIN).all()) and bool((tau[live] < R.TAU_MAX).all())
    assert bool((q >= 0).all()) and bool((q <= R.ONE).all())
    assert not live[5].any()                                               # silence: d' = 1 throughout, no dip
    assert bool(live[4].sum(-1).max() == R.K)                              # noise: more dips than slots
    # the deeper dip at the period (160 +- 1) that first-dip YIN never looks at, on the frames where it reports the
    # octave
    for t in range(17, 25):
        lags = tau[0, t].tolist()
        period = [s for s, v in enumerate(lags) if abs(v - 160) <= 1]
        assert lag[0, t] in (79, 80) and len(period) == 1
        assert q[0, t][period[0]] < q[0, t][lags.index(int(lag[0, t]))]
    # where both trackers choose the same lag the refinement gives the same bits
    same = R.lags_of(tau, path) == lag
    assert int(same.sum()) > 150
    assert np.array_equal(R.refine(dp, R.lags_of(tau, path))[same], R.refine(dp, lag)[same])


def test_log_table_and_weights():
    import inspect
    from speech_anonymization_amd import ops
    sig = inspect.signature(ops.f0_viterbi).parameters
    assert tuple(R.DEFAULTS) == F0_COSTS and F0_METHODS == ("yin", "viterbi")
    assert {k: sig[k].default for k in F0_COSTS} == R.DEFAULTS              # the restatement decodes with the defaults
    assert ops.f0v_log_table("cpu").tolist() == R.log_table().tolist()
    LOG = R.log_table()
    assert LOG.dtype == np.int32 and LOG.shape == (267,) and LOG[0] == LOG[1] == 0
    assert LOG[2] == 65536 and LOG[64] == 6 * 65536 and LOG[256] == 8 * 65536
    assert LOG[160] - LOG[80] == 65536 and bool((np.diff(LOG[1:]) > 0).all())
    assert R.weights_q() == (9830, 9175, 22938, 655)
    assert R.weights_q(4.0, 0.0, 1.0, 0.5) == (262144, 0, 65536, 32768)


# ---------------------------------------------------------------------------------------------------
# decode properties on random integer candidates
# ---------------------------------------------------------------------------------------------------
def test_zero_transition_weights_give_the_per_frame_rule():
    tau, q = R.random_candidates(3, 61, seed=5)
    LOG, wq = R.log_table(), R.weights_q(**R.ZERO_TRANSITIONS)
    assert wq == (9830, 0, 0, 0)
    for b in range(3):
        got = R.decode_row(tau[b].tolist(), q[b].tolist(), 61, wq, LOG)
        assert got == R.per_frame_rule(tau[b].tolist(), q[b].tolist(), 61, wq[0])
        assert got[61 // 2] == -1 and max(got) >= 0 and min(got) == -1


def test_every_tie_goes_to_the_smaller_index():
    LOG = R.log_table()
    T = 6
    tau = [[80, 160, 200, -1, -1, -1, -1, -1]] * T
    q = [[1000, 1000, 1000, 0, 0, 0, 0, 0]] * T
    # no transition cost, no bias: the three candidates tie at every step and at the end -> state 0
    assert R.decode_row(tau, q, T, (5000, 0, 0, 0), LOG) == [0] * T
    # the voicing cost equal to the candidates': unvoiced is state 8 and loses the tie
    assert R.decode_row(tau, q, T, (1000, 0, 0, 0), LOG) == [0] * T
    assert R.decode_row(tau, q, T, (999, 0, 0, 0), LOG) == [-1] * T
    # slot 0 absent: the tie falls to state 1
    tau1 = [[-1, 160, 200, -1, -1, -1, -1, -1]] * T
    assert R.decode_row(tau1, q, T, (5000, 0, 0, 0), LOG) == [1] * T
    # a tie between predecessors: two lags an octave either side of the target cost the same jump
    tau2 = [[40, 160, -1, -1, -1, -1, -1, -1], [80, -1, -1, -1, -1, -1, -1, -1]]
    q2 = [[700, 700, 0, 0, 0, 0, 0, 0], [0] * 8]
    path, costs = R.decode_row(tau2, q2, 2, (60000, 60000, 65536, 0), LOG, return_costs=True)
    assert path == [0, 0] and costs[0] == 700 + 65536
    # a frame without candidates is unvoiced whatever it costs
    tau3 = [tau[0], [-1] * 8, tau[0]]
    assert R.decode_row(tau3, q[:3], 3, (60000, 1, 1, 0), LOG) == [0, -1, 0]


def test_a_row_cut_by_lens_is_the_decode_of_its_first_frames():
    T, N = 50, 160 * 49 + 80
    tau, q = R.random_candidates(2, T, seed=9, tie_runs=False)
    lens = [0.6, 0.31]
    F = R.frames_counted(lens, N, T)
    assert F == [int(round(0.6 * N)) // 160 + 1, int(round(0.31 * N)) // 160 + 1] and max(F) < T
    cut = R.decode(tau, q, lens, N)
    for b in range(2):
        head = R.decode(tau[b:b + 1, :F[b]], q[b:b + 1, :F[b]], [1.0], N)[0]
        assert cut[b, :F[b]].tolist() == head.tolist() and bool((cut[b, F[b]:] == -1).all())
    assert R.frames_counted([2.0, -1.0, float("nan"), 0.0], N, T) == [T, 1, 1, 1]


# ---------------------------------------------------------------------------------------------------
# options
# ---------------------------------------------------------------------------------------------------
def _one_line(fn, *args):
    with pytest.raises(SystemExit) as e:
        fn(*args)
    msg = str(e.value)
    assert msg and "\n" not in msg
    return msg


def test_check_f0_option():
    from speech_anonymization_amd.pitchnorm import check_f0_option as check
    assert check({}) == {} and check({}, {"r_min": 0.6}) == {}
    assert check({"f0_method": "viterbi"}) == {"f0_method": "viterbi"}
    assert check({}, {"f0_method": "viterbi"}) == {"f0_method": "viterbi"}
    assert check({"f0_method": "yin"}, {"f0_method": "viterbi"}) == {"f0_method": "yin"}
    for bad in ("pyin", "Viterbi", True, 1, ""):
        assert "--f0_method" in _one_line(check, {"f0_method": bad})


def test_normalizer_and_f0_track_settings():
    from speech_anonymization_amd import pitchnorm
    pn = pitchnorm.PitchNormalizer()
    assert pn.f0_method == "yin" and pn.f0_costs == {}
    pn = pitchnorm.PitchNormalizer(f0_method="viterbi", f0_costs={"jump_cost": 1, "lag_bias": 0})
    assert pn.f0_method == "viterbi" and pn.f0_costs == {"jump_cost": 1.0, "lag_bias": 0.0}
    for kw in (dict(f0_method="pyin"), dict(f0_method="viterbi", f0_costs={"jump": 1.0}),
               dict(f0_method="viterbi", f0_costs={"jump_cost": 4.5}),
               dict(f0_method="viterbi", f0_costs={"switch_cost": -0.1}),
               dict(f0_method="viterbi", f0_costs={"voicing_cost": float("nan")}),
               dict(f0_costs={"jump_cost": 1.0})):
        with pytest.raises(ValueError) as e:
            pitchnorm.PitchNormalizer(**kw)
        assert "\n" not in str(e.value)
    with pytest.raises(ValueError, match="f0_method"):
        pitchnorm.f0_track(torch.zeros(1, 800), method="praat")
    with pytest.raises(pitchnorm.L.SaHipError, match="GPU"):
        pitchnorm.f0_track(torch.zeros(1, 800), method="viterbi")
    with pytest.raises(pitchnorm.L.SaHipError, match="GPU only"):
        pitchnorm.PitchNormalizer(f0_method="viterbi")(torch.zeros(1, 800), torch.ones(1))


def test_ops_refuse_before_anything_is_loaded(monkeypatch):
    from speech_anonymization_amd import _lib, ops

    def no_load():
        raise AssertionError("the library must not be loaded for a refused tensor")

    monkeypatch.setattr(_lib, "load", no_load)
    dp = torch.zeros(2, 3, 267)
    tau = torch.zeros(2, 3, 8, dtype=torch.int32)
    with pytest.raises(_lib.SaHipError, match="GPU tensors"):
        ops.f0_candidates(dp)
    with pytest.raises(_lib.SaHipError, match="GPU tensors"):
        ops.f0_viterbi(dp, tau, tau, torch.ones(2), 480)


def test_committed_recipe_carries_the_key_only_when_given():
    from speech_anonymization_amd import pitchnorm
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    path = os.path.join(ROOT, "speechbrain_configs", "gender_classifier_pitch_norm.yaml")

    def options(over):
        with open(path) as fin:
            return pitchnorm.check_pitch_options(load_hyperpyyaml(fin, over), {}, environ={})

    pn = options({})
    assert "f0_method" not in pn
    assert options({"f0_method": "viterbi"}) == dict(pn, f0_method="viterbi")
    assert options({"f0_method": "yin"}) == dict(pn, f0_method="yin")
    assert pitchnorm.PitchNormalizer(**options({"f0_method": "viterbi"})).f0_method == "viterbi"
    assert pitchnorm.PitchNormalizer(**options({"f0_method": "viterbi", "phase": "vocoder",
                                                "contour_scale": 1.0})).f0_method == "viterbi"
    with open(path) as fin:
        settings = load_hyperpyyaml(fin, {"f0_method": "pyin"})
    assert "--f0_method pyin" in _one_line(pitchnorm.check_pitch_options, settings, {}, {})


def test_anonymize_takes_the_method_where_something_tracks_f0():
    from speech_anonymization_amd.vocoder import check_anonymize_options as check
    base = {"out_dir": "o", "synthetic": 4, "model_type": "convae"}
    check(dict(base, pitch_norm=True, f0_method="viterbi"), {}, {})
    check(dict(base, pitch_norm=True, f0_method="yin"), {}, {})
    check(dict(base, pitch_norm=True, phase="vocoder", contour_scale=0.5, f0_method="viterbi"), {}, {})
    for mode in ({"recon_ckpt": "d"}, {"passthrough": True}, {"mcadams": 0.8}, {"formant_ratio": 1.15},
                 {"pitch_norm": True}):
        check(dict(base, report_f0=True, f0_method="viterbi", **mode), {}, {})
    for mode in ({"recon_ckpt": "d"}, {"passthrough": True}, {"mcadams": 0.8}, {"formant_ratio": 1.15},
                 {"recon_ckpt": "d", "report_f0": False}):
        assert "--f0_method goes with" in _one_line(check, dict(base, f0_method="viterbi", **mode), {}, {})
    assert "--f0_method pyin" in _one_line(check, dict(base, pitch_norm=True, f0_method="pyin"), {}, {})
    # earlier refusals keep their wording
    old = _one_line(check, dict(base, pitch_norm=True, passthrough=True), {}, {})
    assert old.startswith("--pitch_norm true and --passthrough true exclude each other")
    assert "needs --phase vocoder" in _one_line(check, dict(base, pitch_norm=True, contour_scale=1.0), {}, {})


# ---------------------------------------------------------------------------------------------------
# the C entry points
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from speech_anonymization_amd import _lib
    return _lib.load()


def test_f0v_dim(lib):
    assert [lib.sa_f0v_dim(i) for i in range(5)] == [8, 9, 8, lib.sa_f0v_dim(3), 16]
    assert lib.sa_f0v_dim(3) >= 64 and lib.sa_f0v_dim(3) % 64 == 0
    assert lib.sa_f0v_dim(5) == -22 and lib.sa_f0v_dim(-1) == -22
    assert lib.sa_f0v_dim(2) == lib.sa_yin_dim(6)


def test_entry_points_refuse_before_any_launch(lib):
    """NULL pointers, bounds and NaN weights are -EINVAL; the pointers are never dereferenced on the host and no
    kernel is launched (there is no GPU here)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = ctypes.c_float

    def cand(dp=p, B=1, T=1, tau=p, q=p):
        return lib.sa_f0_candidates(dp, B, T, tau, q, None)

    for kw in (dict(dp=None), dict(tau=None), dict(q=None), dict(B=0), dict(B=65536), dict(T=0), dict(T=(1 << 23) + 1)):
        assert cand(**kw) == -22, kw

    def vit(dp=p, tau=p, q=p, lens=p, log_q=p, B=1, T=1, N=160, w=(0.15, 0.14, 0.35, 0.01), psi=p, path=p, f0=p):
        return lib.sa_f0_viterbi(dp, tau, q, lens, log_q, B, T, N, f(w[0]), f(w[1]), f(w[2]), f(w[3]), psi, path, f0,
                                 None)

    for name in ("dp", "tau", "q", "lens", "log_q", "psi", "path", "f0"):
        assert vit(**{name: None}) == -22, name
    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(T=(1 << 23) + 1), dict(N=0), dict(N=(1 << 30) + 1)):
        assert vit(**kw) == -22, kw
    for i in range(4):
        for bad in (float("nan"), -0.01, 4.01, float("inf")):
            w = [0.15, 0.14, 0.35, 0.01]
            w[i] = bad
            assert vit(w=tuple(w)) == -22, (i, bad)
