"""The modulation-spectrum smoothing without a GPU: the taps, the invariants of the fp64 restatement
tests/modspec_ref.py (which the GPU tests hold the kernel to), the option checks, and that profiles/modspec_delta.json
holds what tools/modspec_delta.py computes."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from speech_anonymization_amd import _lib, modspec, ops, vocoder
from tests import modspec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- taps -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", [3.2, 4.0, 7.5, 10.0, 16.0, 25.0])
def test_taps_are_a_unit_gain_low_pass_with_half_response_at_the_cutoff(cutoff):
    t, J = ops.modspec_taps(cutoff, "cpu")
    h = t.numpy()
    assert t.dtype == torch.float64 and J == len(h) - 1 == int(np.ceil(200.0 / cutoff)) <= ops.MODSPEC_JMAX
    full = np.concatenate([h[:0:-1], h])                     # the filter along time: symmetric by construction
    assert (full == full[::-1]).all() and abs(full.sum() - 1.0) <= 4e-16
    assert abs(R.response(h, 0.0) - 1.0) <= 4e-16
    assert abs(R.response(h, cutoff) - 0.5) <= 0.01
    assert R.response(h, min(50.0, 2.5 * cutoff)) < 0.02 and R.response(h, 0.25 * cutoff) > 0.95
    assert np.abs(h - R.taps(cutoff)).max() <= 1e-15          # the restatement's, formed with numpy
    assert ops.modspec_taps(cutoff, "cpu")[0] is t            # cached per (cutoff, device)


def test_taps_lengths_and_the_identity_at_50_hz():
    assert ops.modspec_taps(10.0, "cpu")[1] == 20 and ops.modspec_taps(3.2, "cpu")[1] == 63
    t, J = ops.modspec_taps(50.0, "cpu")
    assert J == 4 and t.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert R.taps(50.0).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("cutoff", [3.19, 0.0, -10.0, 50.01, float("nan"), float("inf"), True])
def test_taps_refuse_outside_their_range(cutoff):
    with pytest.raises(_lib.SaHipError) as e:
        ops.modspec_taps(cutoff, "cpu")
    assert "\n" not in str(e.value)


# ---- the restatement's invariants ----------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.complex64).view(np.uint32)


def test_identity_taps_depth_0_and_no_frames_give_r_bit_for_bit():
    Rin = R.spectrum(3, 40, 7)
    for h in (np.ones(1), R.taps(50.0)):
        C, peak, Lout, _ = R.smooth(Rin, h, (1.0, 0.5, 1.0), (40, 40, 17))
        assert (_bits(C) == _bits(Rin)).all()
    C, peak, Lout, _ = R.smooth(Rin, R.taps(10.0), (0.0, float("nan"), -1.0), (40, 40, 40))
    assert (_bits(C) == _bits(Rin)).all() and (peak > 0).all()
    assert (Lout == R.log_mag(Rin, (40, 40, 40))[0]).all()    # depth 0: g = 0, Lout = L
    C, peak, Lout, _ = R.smooth(Rin, R.taps(10.0), (1.0, 1.0, 1.0), (0, -3, 0))
    assert (_bits(C) == _bits(Rin)).all() and (peak == 0).all() and (Lout == 0).all()


def test_a_column_constant_in_time_comes_back_within_an_ulp():
    Rin = R.spectrum(2, 90, 3)
    assert (Rin[:, :, 5] == Rin[0, 0, 5]).all()
    for J in (1, 20, 64):
        C, _, _, _ = R.smooth(Rin, R.case_taps(J), (1.0, 1.0), (90, 61))
        for part in (np.real, np.imag):
            got, want = part(C[:, :, 5]).astype(np.float64), part(Rin[:, :, 5]).astype(np.float64)
            assert (np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


def test_frames_past_the_count_are_untouched_and_unread():
    Rin = R.spectrum(2, 50, 11)
    C, peak, Lout, _ = R.smooth(Rin, R.taps(10.0), (1.0, 1.0), (50, 23))
    assert (_bits(C[1, 23:]) == _bits(Rin[1, 23:])).all() and (Lout[1, 23:] == 0).all()
    assert not (_bits(C[1, :23]) == _bits(Rin[1, :23])).all()
    other = Rin.copy()
    other[1, 23:] = 1e3                                       # neither the peak nor the sums look past T_b
    C2, peak2, Lout2, _ = R.smooth(other, R.taps(10.0), (1.0, 1.0), (50, 23))
    assert (_bits(C2[1, :23]) == _bits(C[1, :23])).all() and peak2[1] == peak[1]


@pytest.mark.parametrize("Tb", [1, 2, 5])
def test_edges_are_replicated(Tb):
    """under J = 64 every sum reaches far past both ends of a row of 1, 2 or 5 frames: what it reads there is the
    end frame's L, so the result equals the filter run over the explicitly padded trajectory"""
    Rin = R.spectrum(1, 9, 5 + Tb)
    h = R.case_taps(64)
    C, _, Lout, _ = R.smooth(Rin, h, (1.0,), (Tb,))
    L = R.log_mag(Rin, (Tb,))[0][0, :Tb]
    padded = np.concatenate([np.repeat(L[:1], 64, 0), L, np.repeat(L[-1:], 64, 0)])
    full = np.concatenate([h[:0:-1], h])
    s = np.stack([(full[:, None] * padded[t:t + 129]).sum(0) for t in range(Tb)])
    gmax = float(np.float32(40.0 * R.LN10_OVER_20))          # (the frame under the floor is lifted into the clamp)
    assert np.abs((Lout[0, :Tb] - L) - np.clip(s - L, -gmax, gmax)).max() <= 1e-12
    if Tb == 1:                                              # one frame: every tap reads it, s = L up to rounding
        assert np.abs(Lout[0, :1] - L).max() <= 1e-13
    assert (_bits(C[0, Tb:]) == _bits(Rin[0, Tb:])).all()


def test_the_gain_clamp_and_the_floor_are_reached():
    Rin = np.full((1, 41, R.NBIN), 1.0 + 0j, dtype=np.complex64)
    Rin[0, 20, :] = 1e-3                                      # a 60 dB notch of one frame: the sum lifts it by > 3 dB
    h = R.taps(10.0)
    C, _, Lout, _ = R.smooth(Rin, h, (1.0,), (41,), max_gain_db=3.0)
    gmax = float(np.float32(3.0 * R.LN10_OVER_20))
    g = Lout[0] - R.log_mag(Rin, (41,))[0][0]
    assert np.abs(g[20] - gmax).max() <= 1e-14 and np.abs(g).max() <= gmax + 1e-14
    assert np.abs(np.abs(C[0, 20]) / 1e-3 - np.exp(gmax)).max() <= 1e-6
    # the floor: at floor_rel 1e-2 the notch is read as 1e-2 of the peak, not as 1e-3
    L = R.log_mag(Rin, (41,), floor_rel=1e-2)[0]
    assert np.abs(L[0, 20] - np.log(float(np.float32(1e-2)))).max() <= 1e-15 and (L[0, 19] == 0).all()
    # exact zeros stay zeros
    Rin[0, 3, 7] = 0
    assert R.smooth(Rin, h, (1.0,), (41,))[0][0, 3, 7] == 0


def test_mod_depth_reads_the_modulation_of_the_end_to_end_rows():
    rows = R.e2e_rows()
    assert rows.shape == (2, 32000) and rows.dtype == np.float32
    for b, fm in enumerate(R.E2E_FM):
        assert R.mod_depth(rows[b], fm) > 10 * R.mod_depth(rows[b], fm + 7.0) > 0


# ---- options ---------------------------------------------------------------------------------------------
def _one_line(fn, *args):
    with pytest.raises(SystemExit) as e:
        fn(*args)
    text = str(e.value)
    assert text and "\n" not in text and not text.isdigit(), text
    return text


def test_check_modspec_options_returns_the_class_arguments():
    assert modspec.check_modspec_options({"modspec_cutoff_hz": 8}) == {
        "cutoff_hz": 8.0, "depth": 1.0, "floor_rel": 1e-4, "max_gain_db": 40.0}
    block = {"cutoff_hz": 5.0, "depth": 0.25, "floor_rel": 1e-3, "max_gain_db": 20}
    assert modspec.check_modspec_options({"modspec_options": block}) == {
        "cutoff_hz": 5.0, "depth": 0.25, "floor_rel": 1e-3, "max_gain_db": 20.0}
    assert modspec.check_modspec_options({"modspec_options": block, "modspec_depth": 1, "modspec_cutoff_hz": 50}) == {
        "cutoff_hz": 50.0, "depth": 1.0, "floor_rel": 1e-3, "max_gain_db": 20.0}
    assert modspec.check_modspec_options({"modspec_options": block, "modspec_depth": 0.5})["depth"] == 0.5
    assert modspec.check_modspec_options({}) == {"cutoff_hz": 10.0, "depth": 1.0, "floor_rel": 1e-4,
                                                 "max_gain_db": 40.0}


@pytest.mark.parametrize("settings", [
    {"modspec_cutoff_hz": 3.0}, {"modspec_cutoff_hz": 51}, {"modspec_cutoff_hz": "low"}, {"modspec_cutoff_hz": True},
    {"modspec_cutoff_hz": float("nan")}, {"modspec_depth": 0.5},
    {"modspec_cutoff_hz": 10, "modspec_depth": -0.1}, {"modspec_cutoff_hz": 10, "modspec_depth": 1.5},
    {"modspec_cutoff_hz": 10, "modspec_depth": "deep"}, {"modspec_cutoff_hz": 10, "modspec_depth": True},
    {"modspec_options": {"cutoff_hz": 2.0}}, {"modspec_options": {"depth": 2.0}},
    {"modspec_options": {"floor_rel": 0.0}}, {"modspec_options": {"floor_rel": 1.0}},
    {"modspec_options": {"max_gain_db": 0.0}}, {"modspec_options": {"max_gain_db": "loud"}}])
def test_check_modspec_options_refuses_in_one_line(settings):
    _one_line(modspec.check_modspec_options, settings)


def test_the_class_refuses_what_the_options_refuse():
    for kw in ({"cutoff_hz": 3.0}, {"cutoff_hz": True}, {"depth": 1.01}, {"depth": float("nan")}, {"floor_rel": 0.0},
               {"max_gain_db": -1.0}):
        with pytest.raises(ValueError) as e:
            modspec.ModulationSmoother(**kw)
        assert "\n" not in str(e.value)
    ms = modspec.ModulationSmoother()
    assert (ms.cutoff_hz, ms.depth, ms.J) == (10.0, 1.0, 20)
    with pytest.raises(_lib.SaHipError):
        ms(torch.zeros(1, 1600), torch.ones(1))              # no CPU fallback


BASE = {"out_dir": "o", "synthetic": 4, "modspec_cutoff_hz": 10}
OTHERS = [("resynth", True), ("resynth_pitch_hz", 170), ("aspiration", 0.3), ("formant_norm", True),
          ("formant_norm_ratio", 0.9), ("formant_target", "550,1650,2750"), ("formant_q_min", 0.9),
          ("formant_q_max", 1.1), ("mcadams", 0.8), ("mcadams_min", 0.5), ("mcadams_max", 0.9), ("pitch_norm", True),
          ("pitch_target_hz", 170), ("formant_ratio", 1.15), ("preserve_formants", True), ("phase", "vocoder"),
          ("psola", True), ("contour_scale", 1.0), ("contour_smooth", 2), ("lifter", 30), ("recon_ckpt", "dir"),
          ("passthrough", True)]


def test_the_mode_is_selected_by_its_flag_and_runs_the_reports():
    assert vocoder.anonymize_mode(BASE) == "modspec"
    assert vocoder.anonymize_mode(dict(BASE, resynth=True, pitch_norm=True)) == "modspec"
    assert vocoder.anonymize_mode({"out_dir": "o"}) == "model"
    vocoder.check_anonymize_options(dict(BASE, modspec_depth=0.5), {}, {})
    vocoder.check_anonymize_options(dict(BASE, report_f0=True, report_stoi=True, report_prosody=True, report_mcd=True,
                                         report_formants=True, f0_method="viterbi"), {}, {})


@pytest.mark.parametrize("key,value", OTHERS, ids=[k for k, _ in OTHERS])
def test_the_mode_excludes_every_other_modes_flags(key, value):
    text = _one_line(vocoder.check_anonymize_options, dict(BASE, **{key: value}), {}, {})
    assert "--modspec_cutoff_hz" in text or key in text


def test_the_modes_other_refusals():
    text = _one_line(vocoder.check_anonymize_options, {"out_dir": "o", "synthetic": 4, "passthrough": True,
                                                      "modspec_depth": 0.5}, {}, {})
    assert "--modspec_depth goes with --modspec_cutoff_hz" in text
    for more, run_opts, env in (({"modspec_cutoff_hz": 2}, {}, {}), ({"modspec_depth": 3}, {}, {}),
                                ({"f0_method": "viterbi"}, {}, {}), ({"hip_graph": True}, {}, {}),
                                ({}, {"distributed_launch": True}, {}), ({}, {}, {"WORLD_SIZE": "2"}),
                                ({"out_dir": None}, {}, {}), ({"synthetic": None}, {}, {})):
        _one_line(vocoder.check_anonymize_options, dict(BASE, **more), run_opts, env)
    for run_opts, env, more in (({"distributed_launch": True}, {}, {}), ({}, {"WORLD_SIZE": "2"}, {}),
                                ({"hip_graph": True}, {}, {}), ({}, {}, {"hip_graph": True}),
                                ({}, {}, {"modspec_cutoff_hz": 1})):
        text = _one_line(modspec.check_recipe_options, dict({"modspec_options": {"cutoff_hz": 10.0}}, **more), run_opts,
                         env)
    assert modspec.check_recipe_options({"modspec_options": {"cutoff_hz": 6.0}}, {}, {})["cutoff_hz"] == 6.0


def test_the_recipes_settings_file_gives_the_defaults():
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    with open(os.path.join(ROOT, "speechbrain_configs", "gender_classifier_modspec.yaml")) as f:
        settings = load_hyperpyyaml(f, {})
    assert modspec.check_recipe_options(settings, {}, {}) == {"cutoff_hz": 10.0, "depth": 1.0, "floor_rel": 1e-4,
                                                              "max_gain_db": 40.0}


def test_the_older_option_walk_still_reproduces_its_golden_file():
    import hashlib
    import json
    tool = _tool("option_refusals")
    with open(os.path.join(ROOT, "tests", "golden", "option_refusals.json")) as f:
        golden = json.load(f)
    now = tool.walk_all()
    assert sum(len(w) for w in now.values()) == golden["cases"]
    for name, walk in now.items():
        assert hashlib.sha256("\n".join(walk).encode()).hexdigest() == golden[name]["settings_sha256"], name
        assert [golden["outcomes"][i] for i in golden[name]["outcome"]] == list(walk.values()), name


# ---- the recorded figures ------------------------------------------------------------------------------
def test_the_delta_file_holds_what_the_tool_computes():
    rec, now = R.load_delta(), _tool("modspec_delta").measure()
    assert rec["a"] == now["a"] and rec["a"]["share_worst"] <= 1e-3 / 16.0
    for key in ("class", "e2e"):
        assert set(rec[key]) == set(now[key])
        for k, v in now[key].items():
            assert np.allclose(rec[key][k], v, rtol=1e-6, atol=1e-12), (key, k)
    assert rec["e2e"]["ratio"][0] > 0.95 and rec["e2e"]["ratio"][1] < 0.3
