"""WSOLA time-scale modification without a GPU: the restatement of tests/wsola_ref.py on hand-made
rows, the host logic of ops and timescale, the options of anonymize.py and of the recipe, and the figures of
profiles/wsola_delta.json (which tools/wsola_delta.py measures on that restatement, and which the GPU test reads)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from speech_anonymization_amd import _lib, ops, timescale, vocoder
from tests import wsola_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, D, ONE = R.H, R.W, R.D, R.ONE
BASE = {"out_dir": "o", "synthetic": 4, "tempo": 0.8}


def _one_line(fn, *args, **kw):
    with pytest.raises(SystemExit) as e:
        fn(*args, **kw)
    text = str(e.value)
    assert text and "\n" not in text
    return text


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _nominal(k, tq):
    return (k * H * tq + (ONE >> 1)) >> 16


# ---- the restatement's invariants ----------------------------------------------------------------------
def test_tempo_one_is_the_identity_bit_for_bit():
    wav, nv, _, _ = R.edge_case()
    for b in range(wav.shape[0]):
        out, _, pos, K, n_out = R.wsola(wav[b], nv[b], ONE, wav.shape[1])
        assert n_out == nv[b] and pos == [k * H for k in range(K)]
        assert (_bits(out[:n_out]) == _bits(wav[b, :n_out])).all() and not out[n_out:].any()


@pytest.mark.parametrize("tempo", [0.5, 0.8, 1.25, 2.0])
def test_zero_and_constant_rows_follow_the_nominal_positions(tempo):
    tq, N = R.q_of(tempo), 3000
    for row in (np.zeros(N, dtype=np.float32), np.full(N, -0.5, dtype=np.float32)):
        out, q, pos, K, n_out = R.wsola(row, N, tq, 2 * N)
        assert n_out == R.out_len(N, tq) and K == (n_out - 1) // H + 1
        # every cost ties: the candidate nearest the nominal position wins, the nominal position itself while it is
        # a candidate (a constant row's windows differ once they reach past the last valid sample: q is 0 there)
        inside = [k for k in range(1, K) if _nominal(k, tq) + W <= N and pos[k - 1] + H + W <= N]
        assert inside and all(pos[k] == _nominal(k, tq) for k in inside)
        assert not row.any() or set(q.tolist()) == {-16383}


@pytest.mark.parametrize("tempo", [0.8, 1.25])
def test_a_pulse_train_keeps_its_spacing(tempo):
    N, P = 6400, 100
    wav = np.zeros(N, dtype=np.float32)
    wav[37::P] = 1.0
    out, _, pos, K, n_out = R.wsola(wav, N, R.q_of(tempo), 2 * N)
    assert n_out == R.out_len(N, R.q_of(tempo)) and R.jumps(pos) >= 3
    peaks = np.flatnonzero(out[:n_out - W] > 0.5)
    assert len(peaks) >= (n_out - W) // P - 1 and set(np.diff(peaks).tolist()) == {P}
    assert out[peaks].min() >= 0.999                          # the pulses overlap themselves: the windows sum to one


def test_lengths_follow_the_formula_and_out_of_range_tempos_read_as_the_bounds():
    for n in (0, 1, 159, 160, 161, 4000, 1 << 24):
        for tq, expect in ((1 << 15, 2 * n), (ONE - 1, None), (ONE, n), (ONE + 1, None), (1 << 17, (n + 1) // 2)):
            got = R.out_len(n, tq)
            assert got == ((n * ONE + tq // 2) // tq if n else 0) == ops.wsola_out_len(n, tq)
            assert expect is None or got == expect
            nv, n_out, K = R.lengths(n, tq, max(n, 1), 1 << 25)
            assert n_out == got and K == ((got - 1) // H + 1 if got else 0)
        for tq, bound in ((0, 1 << 15), (-5, 1 << 15), (1 << 14, 1 << 15), (1 << 20, 1 << 17), ((1 << 17) + 1, 1 << 17)):
            assert R.out_len(n, tq) == R.out_len(n, bound) == ops.wsola_out_len(n, tq)
    assert R.lengths(4000, 1 << 15, 4000, 3001)[1:] == (3001, 19)          # the cap
    assert R.lengths(9999, ONE, 4000, 8000)[0] == 4000 and R.lengths(-3, ONE, 4000, 8000) == (0, 0, 0)
    assert ops.wsola_out_len(1 << 24, 1 << 15) == 1 << 25
    for bad in (-1, (1 << 24) + 1):
        with pytest.raises(_lib.SaHipError):
            ops.wsola_out_len(bad, ONE)


def test_ties_go_to_the_nominal_position_and_then_to_the_smaller_candidate():
    assert R.choose(np.array([5, 3, 3, 3, 9]), 100, 102) == 102              # the least cost nearest a
    assert R.choose(np.array([5, 3, 7, 3, 9]), 100, 102) == 101              # equal distance: the smaller c
    assert R.choose(np.array([2, 3, 3, 3, 9]), 100, 102) == 100              # cost first
    assert R.choose(np.array([4, 4]), 100, 500) == 101 and R.choose(np.array([4, 4]), 100, 0) == 100
    # on a hand-made q: period 40, so the candidates a - 160 + 40 j + phase all cost 0 and the one nearest a wins
    N, tq = 4000, R.q_of(0.8)
    q = np.tile(np.arange(40, dtype=np.int16) * 100, N // 40)
    pos, n_out = R.positions(q, N, tq, 2 * N)
    for k in range(1, len(pos)):
        a, t = _nominal(k, tq), pos[k - 1] + H
        if a + D + W > N:
            break
        zero = [c for c in range(a - D, a + D + 1) if (c - t) % 40 == 0]
        best = min(zero, key=lambda c: (abs(c - a), c))
        assert pos[k] == best and abs(pos[k] - a) <= 20
    assert k > 10
    # hi < lo: the nominal position lies more than D past the last valid sample -- the one candidate is hi
    pos, _ = R.positions(np.ones(4000, dtype=np.int16), 700, 1 << 15, 8000)
    assert len(pos) == 9 and pos[1:4] == [80, 160, 240]
    pos, _ = R.positions(np.ones(400, dtype=np.int16), 1, 1 << 15, 700)
    assert pos == [0]


def test_non_finite_samples_count_as_zero_in_q():
    wav = np.array([0.5, np.nan, -np.inf, 1.0, np.inf, -0.25, 2.0], dtype=np.float32)
    assert R.quant(wav, 6).tolist() == [8192, 0, 0, 16383, 0, -4096, 0]     # (8191.5 rounds to even; 2.0 does not count)
    assert R.quant(wav, 7).tolist() == [4096, 0, 0, 8192, 0, -2048, 16383]
    assert not R.quant(np.full(5, np.nan, dtype=np.float32), 5).any()
    assert not R.quant(np.array([0.0, -0.0, np.inf], dtype=np.float32), 3).any()
    tiny = np.array([3, -1, 2], dtype=np.float64) * 2.0 ** -149
    assert R.quant(tiny.astype(np.float32), 3).tolist() == [16383, -5461, 10922]
    assert R.quant(wav, 0).tolist() == [0] * 7 and R.quant(wav, -4).tolist() == [0] * 7


def test_the_window_is_the_fp64_hann_rounded_once_and_overlaps_to_one():
    h = R.window()
    assert h.dtype == np.float32 and h[0] == 0.0 and h[H] == 1.0 and (h[1:] == h[:0:-1]).all()
    assert np.abs(h[:H].astype(np.float64) + h[H:].astype(np.float64) - 1.0).max() <= 2.0 ** -24
    assert (ops.wsola_window("cpu").numpy() == h).all() and ops.wsola_window("cpu") is ops.wsola_window("cpu")


def test_a_nan_of_the_overlap_add_is_the_canonical_one_and_copies_keep_their_bits():
    wav, nv, tq, Nout = R.edge_case()
    out, _, pos, K, n_out = R.wsola(wav[4], nv[4], tq[4], Nout)
    nan = np.isnan(out)
    copied = np.zeros(Nout, dtype=bool)
    for k in range(K):
        if k == 0 or pos[k] == pos[k - 1] + H:
            copied[k * H:min(k * H + H, n_out)] = True
    assert nan[~copied].any() and (_bits(out)[nan & ~copied] == 0x7FC00000).all()
    assert _bits(out)[7] == 0xFFC00001 and copied[7]


def test_the_cases_of_the_gpu_test_reach_the_paths_they_are_there_for():
    cases = R.kernel_cases()
    ref = {name: R.reference(case) for name, case in cases.items()}
    assert [r[3] for r in ref["short"]] == [1]
    assert [r[4] for r in ref["multiple"]] == [1600, 1601, 1600, 1601]
    assert ref["cap"][0][4] == 3001 and ref["batch"][4][3:] == (0, 0) and ref["empty_fast"][0][3:] == (0, 0)
    assert all(R.jumps(r[2]) > 0 for r in ref["low"]) and all(R.jumps(r[2]) > 10 for r in ref["long"])
    assert max(r[2][-1] for r in ref["long"]) > 2 * 8192                     # the search stages more than two chunks
    assert R.jumps(ref["odd"][3][2]) == 0                                    # tempo_q = 2^16 + 1 is still the identity


# ---- host logic ----------------------------------------------------------------------------------------
def test_workspace_bytes_are_q_and_the_partial_maxima():
    assert ops.wsola_workspace_bytes(1, 1) == 16 + 16
    assert ops.wsola_workspace_bytes(5, 4000) == 40000 + 32                  # one partial maximum a row: 20 bytes -> 32
    assert ops.wsola_workspace_bytes(3, 4093) == (3 * 4093 * 2 + 15) // 16 * 16 + 16
    assert ops.wsola_workspace_bytes(3, 4094) == (3 * 4094 * 2 + 15) // 16 * 16 + 32


def test_wrappers_refuse_cpu_tensors_before_the_library_is_loaded(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    wav = torch.zeros(2, 1000)
    nv, tq = torch.full((2,), 1000, dtype=torch.int32), torch.full((2,), ONE, dtype=torch.int32)
    q = torch.zeros(2, 1000, dtype=torch.int16)
    pos, count = torch.zeros(2, 13, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for call in (lambda: ops.wsola_quant(wav, nv), lambda: ops.wsola_search(q, tq, nv, 2000),
                 lambda: ops.wsola_ola(wav, pos, count, tq, nv, 2000), lambda: ops.wsola(wav, tq, nv, 2000),
                 lambda: timescale.TimeScaler()(wav, torch.ones(2))):
        with pytest.raises(_lib.SaHipError) as e:
            call()
        assert "GPU" in str(e.value) and "\n" not in str(e.value)
    for bad in ((0, 100), (65536, 100), (1, 0), (1, (1 << 24) + 1)):
        with pytest.raises(_lib.SaHipError):
            ops.wsola_workspace(*bad, "cpu")


def test_time_scaler_settings_and_draws():
    ts = timescale.TimeScaler()
    assert ts.tempo == 1.0 and ts.tempo_range is None and ts.seed == 1 and ts.last is None
    assert ts.draw(3) == [ONE] * 3
    assert timescale.TimeScaler(0.8).draw(2) == [52429, 52429] and timescale.tempo_to_q(1.25) == 81920
    assert timescale.tempo_to_q(0.5) == 1 << 15 and timescale.tempo_to_q(2) == 1 << 17
    a, b = timescale.TimeScaler(tempo_range=(0.8, 1.25), seed=7), timescale.TimeScaler(tempo_range=[0.8, 1.25], seed=7)
    first, second = a.draw(5), a.draw(5)
    assert first == b.draw(5) and second == b.draw(5) and first != second     # the seed and the number of calls
    assert all(52429 <= v <= 81920 for v in first + second) and len(set(first)) > 1
    assert timescale.TimeScaler(tempo_range=(0.8, 1.25), seed=8).draw(5) != first
    assert timescale.TimeScaler(tempo_range=(1.1, 1.1)).draw(2) == [timescale.tempo_to_q(1.1)] * 2
    for kw in ({"tempo": 0.49}, {"tempo": 2.01}, {"tempo": "fast"}, {"tempo": None}, {"tempo": True},
               {"tempo": float("nan")}, {"tempo_range": (0.8,)}, {"tempo_range": 0.8}, {"tempo_range": (1.2, 0.9)},
               {"tempo_range": (0.4, 1.0)}, {"tempo_range": (0.8, 2.5)}, {"tempo_range": (0.8, 1.0, 1.2)}):
        with pytest.raises(ValueError) as e:
            timescale.TimeScaler(**kw)
        assert str(e.value).startswith("TimeScaler: ") and "\n" not in str(e.value)


def test_check_tempo_options_returns_the_class_arguments():
    check = timescale.check_tempo_options
    assert check({}) == {"seed": 1, "tempo": 1.0}
    assert check({"tempo": 0.8}) == {"seed": 1, "tempo": 0.8}
    assert check({"tempo_min": 0.8, "tempo_max": 1.25}) == {"seed": 1, "tempo_range": (0.8, 1.25)}
    block = {"tempo_options": {"tempo": 1.1, "seed": 5}}
    assert check(block) == {"seed": 5, "tempo": 1.1}
    assert check(dict(block, tempo=0.9)) == {"seed": 5, "tempo": 0.9}
    assert check(dict(block, tempo_min=0.9, tempo_max=1.0)) == {"seed": 5, "tempo_range": (0.9, 1.0)}
    ranged = {"tempo_options": {"tempo_min": 0.7, "tempo_max": 1.4}}
    assert check(ranged) == {"seed": 1, "tempo_range": (0.7, 1.4)}
    assert check(dict(ranged, tempo=1.2)) == {"seed": 1, "tempo": 1.2}        # a flag outranks the block's range
    assert check({}, block={"tempo": 2}) == {"seed": 1, "tempo": 2.0}
    for opts in (check({"tempo": 0.8}), check(ranged)):
        timescale.TimeScaler(**opts)


@pytest.mark.parametrize("settings", [
    {"tempo": 0.4}, {"tempo": 2.5}, {"tempo": "x"}, {"tempo": True}, {"tempo_min": 0.8}, {"tempo_max": 1.2},
    {"tempo": 1.0, "tempo_min": 0.8, "tempo_max": 1.2}, {"tempo_min": 1.2, "tempo_max": 0.8},
    {"tempo_min": 0.3, "tempo_max": 0.8}, {"tempo_min": 0.8, "tempo_max": 3}, {"tempo_options": {"tempo": 9}},
    {"tempo_options": {"tempo_min": 0.9}}], ids=str)
def test_check_tempo_options_refuses_in_one_line(settings):
    _one_line(timescale.check_tempo_options, settings)


def test_the_recipe_refuses_graphs_and_data_parallelism_and_reads_its_settings_file():
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    for run_opts, env, more in (({"distributed_launch": True}, {}, {}), ({}, {"WORLD_SIZE": "2"}, {}),
                                ({"hip_graph": True}, {}, {}), ({}, {}, {"hip_graph": True}), ({}, {}, {"tempo": 3})):
        text = _one_line(timescale.check_recipe_options, dict({"tempo_options": {"tempo": 0.8}}, **more), run_opts, env)
        assert "gender_classifier_train_tempo" in text or "--tempo" in text
    with open(os.path.join(ROOT, "speechbrain_configs", "gender_classifier_tempo.yaml")) as f:
        settings = load_hyperpyyaml(f, {})
    assert timescale.check_recipe_options(settings, {}, {}) == {"seed": 1, "tempo": 0.8}
    assert timescale.check_recipe_options(dict(settings, tempo_min=0.8, tempo_max=1.25), {}, {}) == \
        {"seed": 1, "tempo_range": (0.8, 1.25)}


# ---- anonymize.py's options ------------------------------------------------------------------------------
OTHERS = [("modspec_cutoff_hz", 10.0), ("modspec_depth", 0.5), ("resynth", True), ("resynth_pitch_hz", 150.0),
          ("aspiration", 0.3), ("formant_norm", True), ("formant_norm_ratio", 1.1), ("formant_target", "500,1500,2500"),
          ("mcadams", 0.8), ("mcadams_min", 0.7), ("pitch_norm", True), ("pitch_target_hz", 150.0),
          ("formant_ratio", 1.1), ("preserve_formants", True), ("phase", "vocoder"), ("psola", True),
          ("contour_scale", 1.0), ("contour_smooth", 2), ("lifter", 30), ("recon_ckpt", "d"), ("passthrough", True)]


def test_the_mode_is_selected_by_its_flags_and_takes_the_f0_report():
    assert vocoder.anonymize_mode(BASE) == "tempo"
    assert vocoder.anonymize_mode({"tempo_min": 0.8, "tempo_max": 1.2}) == "tempo"
    assert vocoder.anonymize_mode(dict(BASE, modspec_cutoff_hz=10.0, resynth=True)) == "tempo"
    assert vocoder.anonymize_mode({"out_dir": "o"}) == "model" and "tempo" in vocoder.TEMPO_FLAGS
    for more in ({}, {"report_f0": True}, {"report_f0": True, "f0_method": "viterbi"}, {"seed": 3},
                 {"report_stoi": False}):
        vocoder.check_anonymize_options(dict(BASE, **more), {}, {})
    vocoder.check_anonymize_options({"out_dir": "o", "synthetic": 4, "tempo_min": 0.8, "tempo_max": 1.25}, {}, {})


@pytest.mark.parametrize("key,value", OTHERS, ids=[k for k, _ in OTHERS])
def test_the_mode_excludes_every_other_modes_flags(key, value):
    text = _one_line(vocoder.check_anonymize_options, dict(BASE, **{key: value}), {}, {})
    assert text.startswith(f"--tempo takes no --{key}:")


@pytest.mark.parametrize("key", vocoder.TEMPO_REPORTS)
def test_the_mode_refuses_the_reports_that_need_an_alignment(key):
    text = _one_line(vocoder.check_anonymize_options, dict(BASE, **{key: True}), {}, {})
    assert text.startswith(f"--tempo takes no --{key} true:") and "frame against frame" in text


def test_the_modes_other_refusals():
    for more, run_opts, env in (({"tempo": 3}, {}, {}), ({"tempo_min": 0.8}, {}, {}), ({"f0_method": "viterbi"}, {}, {}),
                                ({"hip_graph": True}, {}, {}), ({}, {"distributed_launch": True}, {}),
                                ({}, {}, {"WORLD_SIZE": "2"}), ({"out_dir": None}, {}, {}), ({"synthetic": None}, {}, {}),
                                ({"prosody_max_lag": 4}, {}, {})):
        _one_line(vocoder.check_anonymize_options, dict(BASE, **more), run_opts, env)


def test_the_older_option_walk_still_reproduces_its_golden_file():
    import hashlib
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
    with open(os.path.join(ROOT, "profiles", "wsola_delta.json")) as f:
        rec = json.load(f)
    now = _tool("wsola_delta").measure()
    assert set(rec) == set(now) and rec["tempos"] == [0.8, 1.25] and rec["fundamentals_hz"] == now["fundamentals_hz"]
    for key in ("f0_delta_hz", "tracker_delta_hz", "f0_bar_hz", "f0_mean_in_hz"):
        assert np.allclose(rec[key], now[key], rtol=1e-9, atol=1e-9), key
    for tempo in ("tempo_0.8", "tempo_1.25"):
        assert rec[tempo]["n_out"] == now[tempo]["n_out"]
        for key in ("f0_mean_out_hz", "rms_ratio"):
            assert np.allclose(rec[tempo][key], now[tempo][key], rtol=1e-9, atol=1e-9), (tempo, key)
        assert max(abs(r - 1.0) for r in rec[tempo]["rms_ratio"]) < 0.02
    assert rec["f0_bar_hz"] == pytest.approx(2.0 * (rec["f0_delta_hz"] + rec["tracker_delta_hz"]))
    assert rec["f0_bar_hz"] < 1.0                             # a bar that would tell a 1 % change of pitch at 95 Hz
