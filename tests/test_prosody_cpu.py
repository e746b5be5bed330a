"""CPU checks of the pitch-correlation scorer: the properties of the fp64 restatement
tests/prosody_ref.py, the conditions the GPU test's inputs have to meet (no lag choice and no validity decision near
its threshold, the ties exact), the constants held to tools/prosody_delta.py, and the plumbing that needs no GPU."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import prosody_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 61


def f32(v):
    return np.asarray(v, dtype=np.float32)


def one(ref, deg, frames=T, **kw):
    """a single row through the restatement -> (rho, lag, common, shift_st, dev_st, voicing)"""
    r = R.compare(f32(ref)[None], f32(deg)[None], [frames], **kw)
    return tuple(float(getattr(r, k)[0]) for k in ("rho", "lag", "common", "shift_st", "dev_st", "voicing"))


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def test_walk_order():
    assert R.walk(0) == [0] and R.walk(2) == [0, -1, 1, -2, 2] and len(R.walk(32)) == 65


def test_identical_tracks_score_exactly_one():
    ref = R.gapped()
    n = int((ref > 0).sum())
    assert n == T - 7
    assert one(ref, ref) == (1.0, 0.0, float(n), 0.0, 0.0, 1.0)


def test_a_scaled_track_keeps_the_correlation_and_reports_the_shift():
    ref = f32(R.gapped())
    rho, lag, common, shift, dev, voicing = one(ref, f32(1.2 * ref.astype(np.float64)))
    print("scaled by 1.2: 1 - rho", 1.0 - rho, "shift", shift, "dev", dev)
    assert abs(rho - 1.0) <= 1e-12 and lag == 0 and voicing == 1.0
    assert abs(shift - 12.0 * math.log2(1.2)) <= 1e-6 and dev < 1e-5


def test_a_delay_is_found_as_a_positive_lag_and_an_advance_as_a_negative_one():
    ref = R.gapped()
    assert one(ref, R.shifted(ref, 3))[:2] == (1.0, 3.0)
    assert one(ref, R.shifted(ref, -2))[:2] == (1.0, -2.0)


def test_an_inverted_contour_reads_minus_one_only_without_lags():
    ref = f32(R.gapped())
    deg = 300.0 - ref.astype(np.float64)
    rho = one(ref, deg, max_lag=0)[0]
    assert abs(rho + 1.0) <= 1e-12
    assert one(ref, deg, max_lag=8)[0] > rho                # a maximum over lags


def test_min_common_is_a_threshold_on_the_common_frames():
    ref = R.gapped()
    deg = 1.1 * ref + np.where(ref > 0, np.random.default_rng(0).standard_normal(T), 0.0)
    assert (ref[:8] > 0).all()
    assert one(ref, deg, frames=7, max_lag=0, min_common=8) == (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    rho, lag, common = one(ref, deg, frames=8, max_lag=0, min_common=8)[:3]
    assert common == 8.0 and rho > 0.9


def test_a_constant_track_scores_nothing_but_reports_the_voicing_of_lag_zero():
    ref = R.gapped()
    got = one(ref, np.full(T, 150.0))
    assert got == (0.0, 0.0, 0.0, 0.0, 0.0, (T - 7) / T)


def test_no_frames_give_six_zeros():
    ref = R.gapped()
    assert one(ref, ref, frames=0) == (0.0,) * 6
    assert one(ref, ref, frames=-3) == (0.0,) * 6


def test_frames_beyond_the_count_are_ignored():
    ref = R.gapped()
    deg = R.shifted(1.1 * ref, 1) + np.where(R.shifted(ref, 1) > 0, np.random.default_rng(1).standard_normal(T), 0.0)
    want = one(ref[:40], deg[:40], frames=40)
    bad_ref, bad_deg = ref.copy(), deg.copy()
    bad_ref[40:], bad_deg[40:] = np.nan, np.nan
    assert one(ref, deg, frames=40) == want and one(bad_ref, bad_deg, frames=40) == want
    assert one(ref, deg, frames=1000) == one(ref, deg, frames=T)            # clamped to T


# ---------------------------------------------------------------------------------------------------
# the GPU test's inputs
# ---------------------------------------------------------------------------------------------------
def test_exact_ties_go_to_the_smaller_lag_then_to_the_negative_one():
    for name, (winner, tied) in R.TIE_CASES.items():
        r = R.case_ref(name)
        exact = sorted(lag for lag, v in r.lags[0].items() if v[5] == 1.0)
        print(name, "exactly 1.0 at", exact, "winner", int(r.lag[0]))
        assert tuple(exact) == tied and int(r.lag[0]) == winner and r.rho[0] == 1.0
        assert r.shift_st[0] == 0.0 and r.dev_st[0] == 0.0 and r.voicing[0] == 1.0
        assert all(v[5] < 1.0 - 1e-3 for lag, v in r.lags[0].items() if lag not in tied and v[5] is not None)


def test_gpu_cases_keep_clear_of_every_decision():
    """the winning lag of every row leads every other valid lag by more than 1e-6 (the tied lags of the two tie cases
    apart), and no s_xx or s_yy is within 1e-9 (relative) of 0 without being exactly 0: no case is left out"""
    cases = R.gpu_cases()
    assert [c[0] for c in cases] == ["rows", "one", "shrink", "wide", "inverted", "flat", "tie4", "tie8"]
    shapes = {c[0]: (c[1].shape, c[3].tolist(), c[4]) for c in cases}
    assert shapes["rows"] == ((3, 61), [61, 40, 0], 8) and shapes["one"][0] == (1, 1)
    assert shapes["shrink"] == ((1, 9), [9], 8) and shapes["wide"] == ((2, 1030), [1030, 1030], 32)
    assert shapes["inverted"] == ((1, 300), [300], 0)
    for name, ref, deg, frames, Lg, m in cases:
        assert ref.dtype == deg.dtype == np.float32 and frames.dtype == np.int32 and ref.shape == deg.shape
        r = R.case_ref(name)
        lead, rel = R.margins(r, skip=R.TIE_CASES.get(name, (0, ()))[1])
        print(name, "lag", r.lag.tolist(), "common", r.common.tolist(), "rho", r.rho.tolist(), "lead", lead,
              "smallest relative s", rel)
        assert lead > R.RHO_MARGIN and rel > R.S_MARGIN, name
    rows = R.case_ref("rows")
    assert rows.lag.tolist() == [3, -2, 0] and rows.common[2] == 0 and rows.common[0] > 8 and rows.common[1] > 8
    assert R.case_ref("one").common[0] == 0 and R.case_ref("one").voicing[0] == 1.0
    shrink = R.case_ref("shrink")
    assert sorted(l for l, v in shrink.lags[0].items() if v[5] is not None) == [-1, 0, 1] and shrink.lag[0] == 1
    assert shrink.lags[0][8][0] == 1 and shrink.lags[0][-8][0] == 1          # the overlap shrinks to one frame
    assert R.case_ref("wide").lag.tolist() == [-20, 32]
    assert abs(R.case_ref("inverted").rho[0] + 1.0) <= 1e-12
    flat = R.case_ref("flat")
    assert flat.common[0] == 0 and all(v[2] == 0.0 for v in flat.lags[0].values())


@pytest.fixture(scope="module")
def delta():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prosody_delta.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_bar_is_the_one_the_delta_tool_measures(delta):
    """tools/prosody_delta.py: the four perturbed evaluations; the bar the GPU test uses is 16 x their worst"""
    print("worst", delta["worst"])
    for k in R.OUTPUTS:
        d = R.DELTA_MEASURED[k]
        assert d * 0.9 <= delta["worst"][k] <= d * 1.001, k
    assert R.DELTA_MEASURED["voicing"] == 0.0 and R.BAR_FACTOR == delta["factor"] == 16.0
    assert delta["smallest_lead"] > R.RHO_MARGIN and delta["smallest_relative_s"] > R.S_MARGIN
    assert max(R.bar(k, 1.0) for k in R.OUTPUTS) <= 1e-7


def test_the_end_to_end_figures_are_the_ones_the_delta_tool_measures(delta):
    """the glide and the vibrato row through the fp64 path, and the margin: four times the spread between that path
    and its fp32 variant"""
    print("table", delta["table"], "spread", delta["spread"])
    for g, want in R.E2E_MEASURED.items():
        for k in ("rho", "dev_st"):
            assert np.abs(np.array(delta["table"][g]["plain"][k]) - np.array(want[k])).max() <= 1e-9, (g, k)
    for k, m in R.E2E_MARGIN.items():
        assert m * 0.9 <= delta["e2e_margin"][k] <= m * 1.001 and delta["e2e_margin"][k] == 4.0 * delta["spread"][k]
    # the pair separates the three settings of the contour option
    dev = [R.E2E_MEASURED[g]["dev_st"] for g in ("1", "0.5", "0")]
    assert all(a < b < c for a, b, c in zip(*dev))
    assert min(R.E2E_MEASURED["1"]["rho"]) > 0.99 > 0.7 > max(R.E2E_MEASURED["0"]["rho"])


# ---------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------
def test_f0cmp_dim_exports_the_constants():
    from speech_anonymization_amd import _lib, ops, vocoder
    lib = _lib.load()
    assert [lib.sa_f0cmp_dim(i) for i in range(3)] == [160, 32, 1024]
    assert lib.sa_f0cmp_dim(3) == -22 and lib.sa_f0cmp_dim(-1) == -22
    assert ops.F0CMP_MAX_LAG == vocoder.PROSODY_MAX_LAG == 32 and ops.F0CMP_MAX_T == 104858
    assert vocoder.PROSODY_LAG_DEFAULT == R.MAX_LAG == 8


def test_binding_refuses_before_it_loads_anything(monkeypatch):
    from speech_anonymization_amd import _lib, ops

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    x, fr = torch.zeros(2, 61), torch.full((2,), 61, dtype=torch.int32)
    with pytest.raises(_lib.SaHipError, match="f0_ref: the F0 comparison kernels take GPU tensors"):
        ops.f0_compare(x, x, fr)
    with pytest.raises(_lib.SaHipError, match="f0_ref: the F0 comparison kernels take GPU tensors"):
        ops.f0_compare(x.numpy(), x, fr)


def test_prosody_stats_average_the_scored_rows():
    from speech_anonymization_amd.metrics import ProsodyStats
    st = ProsodyStats()
    assert st.summarize() == {"f0_corr": None, "f0_dev_st": None, "voicing_agreement": None, "scored": 0,
                              "unscored": 0}
    st.append(["a", "b", "c"], torch.tensor([0.5, 0.0, 0.75]), torch.tensor([30, 0, 9], dtype=torch.int32),
              torch.tensor([1.0, 0.0, 2.0]), torch.tensor([1.0, 0.5, 0.75]))
    st.append(["d"], torch.tensor([-0.25]), torch.tensor([8], dtype=torch.int32), torch.tensor([0.0]),
              torch.tensor([0.25]))
    st.append(["e"], torch.tensor([float("nan")]), torch.tensor([0], dtype=torch.int32), torch.tensor([float("nan")]),
              torch.tensor([0.0]))
    assert st.summarize() == {"f0_corr": 1.0 / 3.0, "f0_dev_st": 1.0, "voicing_agreement": 0.5, "scored": 3,
                              "unscored": 2}
    assert st.ids == ["a", "b", "c", "d", "e"]
    st.clear()
    assert st.summarize()["scored"] == 0 and st.ids == []


MODES = [dict(model_type="convae", recon_ckpt="/x"), dict(model_type="fcae", passthrough=True), dict(pitch_norm=True),
         dict(pitch_norm=True, preserve_formants=True), dict(formant_ratio=1.15), dict(mcadams=0.8)]


@pytest.mark.parametrize("mode", MODES)
def test_report_prosody_is_accepted_in_every_mode(mode):
    from speech_anonymization_amd import vocoder
    base = dict({"out_dir": "o", "synthetic": 2}, **mode)
    assert vocoder.check_anonymize_options(dict(base), {}, {}) is None      # as before without the new keys
    for extra in (dict(report_prosody=True), dict(report_prosody=False), dict(report_prosody=True, prosody_max_lag=0),
                  dict(report_prosody=True, prosody_max_lag=32), dict(report_prosody=True, report_stoi=True),
                  dict(report_prosody=True, f0_method="viterbi"), dict(report_prosody=False, sample_rate=8000)):
        assert vocoder.check_anonymize_options(dict(base, **extra), {}, {}) is None
    with pytest.raises(SystemExit, match="^--report_prosody 'yes': true or false$"):
        vocoder.check_anonymize_options(dict(base, report_prosody="yes"), {}, {})
    with pytest.raises(SystemExit, match="^--report_prosody true tracks the pitch of 16 kHz waveforms only$"):
        vocoder.check_anonymize_options(dict(base, report_prosody=True, sample_rate=8000), {}, {})
    for bad in (-1, 33, 2.5, "4", True):
        with pytest.raises(SystemExit, match=r"^--prosody_max_lag .*: a count of frames in 0\.\.32$"):
            vocoder.check_anonymize_options(dict(base, report_prosody=True, prosody_max_lag=bad), {}, {})
    for flag in (dict(), dict(report_prosody=False)):
        with pytest.raises(SystemExit, match="^--prosody_max_lag needs --report_prosody true: nothing else compares "
                                             "two pitch tracks$"):
            vocoder.check_anonymize_options(dict(base, prosody_max_lag=4, **flag), {}, {})


def test_f0_method_alone_is_still_refused_in_its_own_words():
    from speech_anonymization_amd import vocoder
    base = {"out_dir": "o", "synthetic": 2, "mcadams": 0.8, "f0_method": "viterbi"}
    line = "--f0_method goes with --pitch_norm true or --report_f0 true: nothing else tracks F0"
    for extra in (dict(), dict(report_prosody=False)):
        with pytest.raises(SystemExit) as e:
            vocoder.check_anonymize_options(dict(base, **extra), {}, {})
        assert str(e.value) == line
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "option_refusals.json")))
    assert line in json.dumps(golden)
