"""CPU checks of the formant report: the conditions the GPU test's inputs have to meet (no frame
near a decision), the properties of the fp64 restatement tests/lpcformant_ref.py, the constants held to what
tools/formant_report_delta.py wrote into profiles/formant_report_delta.json, and the plumbing that needs no GPU."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import lpcformant_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 41


def test_gpu_cases_leave_out_no_frame():
    """no frame of the tracks test's cases is near a decision (a nearly real root, a reflection coefficient near 1, r_0
    near the floor, a candidate near a gate), so every status and every value is compared; and the cases have the
    shapes and the statuses they are there for"""
    cases = R.gpu_cases()
    assert [c[0] for c in cases] == ["odd", "one_frame", "empty_row", "synthetic", "zeros"]
    shapes = {c[0]: (c[1].shape, c[2].tolist()) for c in cases}
    assert shapes["odd"] == ((3, 1687), [1687, 1687, 1000]) and R.n_frames(1687) == 11
    assert shapes["one_frame"] == ((1, 50), [50]) and R.n_frames(50) == 1
    assert shapes["empty_row"] == ((2, 1600), [0, 1600]) and shapes["synthetic"] == ((1, 4800), [4800])
    assert not cases[4][1].any()
    for name, wav, nv in cases:
        assert wav.dtype == np.float32 and nv.dtype == np.int32
        ref = R.case_ref(name)
        counts = [int((ref.status == s).sum()) for s in range(4)]
        print(name, "frames", ref.status.size, "status counts", counts, "near a decision", int(ref.near.sum()))
        assert int(ref.near.sum()) == 0, name
        assert ((ref.freq == 0).all(-1) == (ref.status != R.OK)).all() and ((ref.bw == 0) == (ref.freq == 0)).all()
    odd = R.case_ref("odd")
    assert [int((odd.status == s).sum()) for s in range(4)] == [29, 3, 0, 1]
    assert (odd.status[2, 8:] == R.SILENT).all() and (odd.status[2, :8] != R.SILENT).all()
    assert (R.case_ref("empty_row").status[0] == R.SILENT).all() and (R.case_ref("zeros").status == R.SILENT).all()
    assert R.case_ref("one_frame").status.tolist() == [[R.OK]]
    assert (R.case_ref("synthetic").status == R.SHORT).any()                # bare harmonics: poles on harmonics


def test_tracks_find_the_resonances_of_the_voiced_rows():
    """F1 and F2 of the pulse-train rows land within a few per cent of 700 and 1220 Hz, the median F3 within 6 % of
    2600 Hz, in ascending order and inside the gates"""
    ref = R.case_ref("odd")
    for b in range(2):
        ok = ref.status[b] == R.OK
        med = [float(R.lower_median(ref.freq[b, ok, k])) for k in range(3)]
        print("row", b, "scored", int(ok.sum()), "of", ok.size, "medians", med)
        assert abs(med[0] / 700.0 - 1.0) < 0.08 and abs(med[1] / 1220.0 - 1.0) < 0.05
        assert abs(med[2] / 2600.0 - 1.0) < 0.06
        f, bw = ref.freq[b, ok], ref.bw[b, ok]
        assert (np.diff(f, axis=-1) > 0).all() and f.min() >= R.F_LOW and f.max() <= R.F_HIGH
        assert bw.max() <= R.B_HIGH and bw.min() > 0


# ---------------------------------------------------------------------------------------------------
# the restatement of the comparison
# ---------------------------------------------------------------------------------------------------
def tracks(T=T, seed=0):
    rng = np.random.default_rng(seed)
    F = (np.array([700.0, 1220.0, 2600.0]) * (1.0 + 0.05 * rng.standard_normal((1, T, 3)))).astype(np.float32)
    return F, np.zeros((1, T), np.int32), np.full((1, T), 120.0, np.float32)


def one(F_ref, F_deg, st_ref, st_deg, f0_ref, f0_deg, frames, **kw):
    r = R.compare(F_ref, F_deg, st_ref, st_deg, f0_ref, f0_deg, [frames], **kw)
    return r.med[0].tolist(), r.ratio[0].tolist(), float(r.shift[0]), int(r.common[0])


def test_identical_inputs_give_ratios_and_shift_of_exactly_one():
    F, st, f0 = tracks()
    med, ratio, shift, common = one(F, F, st, st, f0, f0, T)
    assert ratio == [1.0, 1.0, 1.0] and shift == 1.0 and common == T
    assert med == [float(np.sort(F[0, :, k])[(T - 1) // 2]) for k in range(3)]


def test_lower_median_on_odd_and_even_counts():
    assert R.lower_median(np.array([5.0, 1.0, 3.0])) == 3.0
    assert R.lower_median(np.array([5.0, 1.0, 3.0, 4.0])) == 3.0             # the lower of the middle two
    assert R.lower_median(np.array([2.0])) == 2.0 and R.lower_median(np.array([2.0, 1.0])) == 1.0
    F, st, f0 = tracks()
    for n in (8, 9):
        med = one(F, F, st, st, f0, f0, n)[0]
        assert med == [float(np.sort(F[0, :n, k])[(n - 1) // 2]) for k in range(3)]


def test_min_common_is_a_threshold():
    F, st, f0 = tracks()
    assert one(F, F, st, st, f0, f0, 7) == ([0.0] * 3, [0.0] * 3, 0.0, 0)
    assert one(F, F, st, st, f0, f0, 8)[3] == 8
    assert one(F, F, st, st, f0, f0, 7, min_common=7)[3] == 7
    assert one(F, F, st, st, f0, f0, 1, min_common=1)[1:] == ([1.0] * 3, 1.0, 1)
    assert one(F, F, st, st, f0, f0, 0, min_common=1) == ([0.0] * 3, [0.0] * 3, 0.0, 0)


def test_frames_cut_the_tail():
    F, st, f0 = tracks()
    bad = F.copy()
    bad[0, 20:] = np.nan
    want = one(F[:, :20], F[:, :20], st[:, :20], st[:, :20], f0[:, :20], f0[:, :20], 20)
    assert one(F, bad, st, st, f0, f0, 20) == one(F, F, st, st, f0, f0, 20) == want
    assert one(F, F, st, st, f0, f0, 1000) == one(F, F, st, st, f0, f0, T)  # clamped to T
    assert one(F, F, st, st, f0, f0, -3)[3] == 0


@pytest.mark.parametrize("status", [R.SILENT, R.FALLBACK, R.SHORT])
@pytest.mark.parametrize("side", ["ref", "deg"])
def test_every_other_status_excludes_its_frame(status, side):
    F, st, f0 = tracks()
    deg = F.copy()
    deg[0, 5] = 9e9                                        # would move a median if it were read
    marked = st.copy()
    marked[0, 5] = status
    args = (F, deg, marked, st, f0, f0) if side == "ref" else (F, deg, st, marked, f0, f0)
    med, ratio, shift, common = one(*args, T)
    keep = np.arange(T) != 5
    assert common == T - 1 and ratio == [1.0] * 3 and shift == 1.0
    assert med == [float(R.lower_median(F[0, keep, k])) for k in range(3)]


@pytest.mark.parametrize("side", ["ref", "deg"])
def test_an_unvoiced_frame_in_either_track_is_excluded(side):
    F, st, f0 = tracks()
    deg = F.copy()
    deg[0, 7] = 9e9
    for unvoiced in (0.0, -1.0):
        gap = f0.copy()
        gap[0, 7] = unvoiced
        args = (F, deg, st, st, gap, f0) if side == "ref" else (F, deg, st, st, f0, gap)
        med, ratio, shift, common = one(*args, T)
        assert common == T - 1 and ratio == [1.0] * 3 and shift == 1.0


def test_rescaled_tracks_report_the_scale():
    F, st, f0 = tracks()
    scale = np.array([1.25, 1.1, 0.9])
    deg = (F.astype(np.float64) * scale).astype(np.float32)
    med, ratio, shift, common = one(F, deg, st, st, f0, f0, T)
    print("ratios", ratio, "shift", shift)
    assert np.abs(np.array(ratio) / scale - 1.0).max() <= 2.0 ** -23
    assert abs(shift / math.exp(np.log(scale).mean()) - 1.0) <= 2.0 ** -22
    assert med == [float(R.lower_median(deg[0, :, k])) for k in range(3)]


# ---------------------------------------------------------------------------------------------------
# the bars
# ---------------------------------------------------------------------------------------------------
def test_the_bars_are_the_ones_the_delta_json_holds():
    """profiles/formant_report_delta.json, as tools/formant_report_delta.py wrote it: the spread of the restatement's
    tracks, no frame near a decision anywhere, and the end-to-end distances"""
    d = R.recorded()
    print("spread", d["spread_hz"], "left out", d["left_out_share"])
    assert R.SPREAD_FACTOR == d["factor"] == 16.0
    for k, v in R.SPREAD_HZ.items():
        assert v * 0.9 <= d["spread_hz"][k] <= v * 1.001, k
    assert d["left_out_share"] == 0.0 <= 0.01 and not any(d["near"].values())
    assert sorted(d["per_case"]) == sorted(c[0] for c in R.gpu_cases())
    for alpha, want in R.E2E_MCADAMS.items():
        got = d["e2e"]["mcadams"][str(alpha)]
        print("alpha", alpha, "ratios", got["ratio"], "theory", got["theory"], "worst distance", got["worst"])
        assert got["near"] == 0 and min(got["common"]) >= 28
        for k in range(3):
            assert want[k] * 0.9 <= got["worst"][k] <= want[k] * 1.001, (alpha, k)
    for beta, want in R.E2E_SHIFT.items():
        got = d["e2e"]["shift"][str(beta)]
        print("formant ratio", beta, "ratios", got["ratio"], "worst distance", got["worst"])
        assert got["near"] == 0 and min(got["common"]) >= 28
        for k in range(3):
            assert want[k] * 0.9 <= got["worst"][k] <= want[k] * 1.001, (beta, k)
    assert max(R.bar("f", 5500.0), R.bar("b", 700.0)) <= 5500.0 * 2.0 ** -24 + 1e-9


# ---------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------
def test_formant_dim_exports_the_constants():
    from speech_anonymization_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsa_hip.so has not been built")
    lib = _lib.load()
    assert [lib.sa_formant_dim(i) for i in range(8)] == [400, 160, 18, 3, 64, 64, 104858, 1024]
    assert lib.sa_formant_dim(8) == -22 and lib.sa_formant_dim(-1) == -22
    assert (ops.FORMANT_W, ops.FORMANT_P, ops.FORMANTS) == (R.W, R.P, R.NF) == (400, 18, 3)
    assert ops.FORMANT_MAX_T == R.MAX_T == 104858 and ops.FORMANT_MAX_N == 1 << 24
    assert R.ABERTH_MAX == 64 and ops.YIN_HOP == R.H


def test_bindings_refuse_before_they_load_anything(monkeypatch):
    from speech_anonymization_amd import _lib, metrics, ops

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    wav, nv = torch.zeros(2, 800), torch.full((2,), 800, dtype=torch.int32)
    with pytest.raises(_lib.SaHipError, match="wav: the formant kernels take GPU tensors"):
        ops.formant_tracks(wav, nv)
    with pytest.raises(_lib.SaHipError, match="wav: the formant kernels take GPU tensors"):
        ops.formant_tracks(wav.numpy(), nv)
    F, st, f0 = torch.zeros(2, 6, 3), torch.zeros(2, 6, dtype=torch.int32), torch.zeros(2, 6)
    fr = torch.full((2,), 6, dtype=torch.int32)
    with pytest.raises(_lib.SaHipError, match="F_ref: the formant kernels take GPU tensors"):
        ops.formant_compare(F, F, st, st, f0, f0, fr)
    with pytest.raises(_lib.SaHipError, match="wav: the formant kernels take GPU tensors"):
        metrics.formant_shift(wav, wav, nv, f0, f0, fr)


def test_formant_stats_average_the_scored_rows():
    from speech_anonymization_amd.metrics import FormantStats
    st = FormantStats()
    none = dict.fromkeys(("formant_shift", "f1_shift", "f2_shift", "f3_shift"))
    assert st.summarize() == dict(none, scored=0, unscored=0)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    st.append(["a", "b", "c"], torch.tensor([1.5, 0.0, 1.0]), torch.tensor([1.25, 0.0, 0.75]),
              torch.tensor([2.0, 0.0, 1.0]), torch.tensor([1.0, 0.0, 1.0]), i32([30, 0, 9]))
    st.append(["d"], torch.tensor([0.5]), torch.tensor([1.0]), torch.tensor([0.0]), torch.tensor([1.0]), i32([8]))
    nan = torch.tensor([float("nan")])
    st.append(["e"], nan, nan, nan, nan, i32([0]))
    assert st.summarize() == {"formant_shift": 1.0, "f1_shift": 1.0, "f2_shift": 1.0, "f3_shift": 1.0, "scored": 3,
                              "unscored": 2}
    assert st.ids == ["a", "b", "c", "d", "e"]
    st.clear()
    assert st.summarize()["scored"] == 0 and st.ids == []


def test_report_row_names_the_documented_keys():
    from speech_anonymization_amd import reports
    row = reports.REPORTS["report_formants"]
    assert row.options == {"f0_method": "yin"}
    assert [k[0] for k in row.keys] == ["f1_hz", "f2_hz", "f3_hz", "f1_shift", "f2_shift", "f3_shift",
                                        "formant_shift", "formant_frames"]
    assert all(gate == 7 for name, col, gate, kind in row.keys if name != "formant_frames")
    assert row.keys[-1][1:] == (7, None, int)
    assert [k[0] for k in row.summary] == ["formant_shift_mean", "f1_shift_mean", "f2_shift_mean", "f3_shift_mean",
                                           "formants_scored"]
    rep = reports.Report("report_formants", {"report_formants": True, "f0_method": "viterbi"})
    assert rep.opts == {"f0_method": "viterbi"}
    z, o = torch.zeros(2), torch.ones(2)
    cols = (700 * o, 1200 * o, 2600 * o, o, o, o, o, torch.tensor([12, 0], dtype=torch.int32))
    rep.collect(["a", "b"], cols)
    rep.fetch()
    assert rep.keys(0) == {"f1_hz": 700.0, "f2_hz": 1200.0, "f3_hz": 2600.0, "f1_shift": 1.0, "f2_shift": 1.0,
                           "f3_shift": 1.0, "formant_shift": 1.0, "formant_frames": 12}
    assert rep.keys(1) == dict(dict.fromkeys(k[0] for k in row.keys), formant_frames=0)
    assert rep.summary() == {"formant_shift_mean": 1.0, "f1_shift_mean": 1.0, "f2_shift_mean": 1.0,
                             "f3_shift_mean": 1.0, "formants_scored": 1}
    assert list(reports.REPORTS)[-1] == "report_formants"


def test_f0_tracks_are_tracked_once_per_window_and_method(monkeypatch):
    from speech_anonymization_amd import pitchnorm, reports
    calls = []

    def fake(wav, method="yin", lens=None):
        calls.append(method)
        return torch.zeros(wav.shape[0], wav.shape[1] // 160 + 1)

    monkeypatch.setattr(pitchnorm, "f0_track", fake)
    w = reports.Window(800, torch.full((2,), 800, dtype=torch.int32), torch.zeros(2, 800), torch.zeros(2, 800))
    a = reports.f0_tracks(w, "yin")
    assert reports.f0_tracks(w, "yin") is a and calls == ["yin", "yin"]      # ref and deg, once each
    reports.f0_tracks(w, "viterbi")
    assert calls == ["yin", "yin", "viterbi", "viterbi"]
    other = reports.Window(800, w.nv, w.ref, w.deg)
    assert reports.f0_tracks(other, "yin") is not a and len(calls) == 6


MODES = [dict(model_type="convae", recon_ckpt="/x"), dict(model_type="fcae", passthrough=True), dict(pitch_norm=True),
         dict(pitch_norm=True, preserve_formants=True), dict(formant_ratio=1.15), dict(mcadams=0.8)]


@pytest.mark.parametrize("mode", MODES)
def test_report_formants_is_accepted_in_every_mode(mode):
    from speech_anonymization_amd import vocoder
    base = dict({"out_dir": "o", "synthetic": 2}, **mode)
    assert vocoder.check_anonymize_options(dict(base), {}, {}) is None      # as before without the new key
    for extra in (dict(report_formants=True), dict(report_formants=False), dict(report_formants=True, report_stoi=True),
                  dict(report_formants=True, report_prosody=True, prosody_max_lag=4),
                  dict(report_formants=True, f0_method="viterbi"), dict(report_formants=False, sample_rate=8000)):
        assert vocoder.check_anonymize_options(dict(base, **extra), {}, {}) is None
    with pytest.raises(SystemExit, match="^--report_formants 'yes': true or false$"):
        vocoder.check_anonymize_options(dict(base, report_formants="yes"), {}, {})
    with pytest.raises(SystemExit, match="^--report_formants true tracks the formants of 16 kHz waveforms only$"):
        vocoder.check_anonymize_options(dict(base, report_formants=True, sample_rate=8000), {}, {})


def test_f0_method_goes_with_report_formants_and_alone_is_refused_in_its_own_words():
    from speech_anonymization_amd import vocoder
    base = {"out_dir": "o", "synthetic": 2, "mcadams": 0.8, "f0_method": "viterbi"}
    assert vocoder.check_anonymize_options(dict(base, report_formants=True), {}, {}) is None
    line = "--f0_method goes with --pitch_norm true or --report_f0 true: nothing else tracks F0"
    for extra in (dict(), dict(report_formants=False)):
        with pytest.raises(SystemExit) as e:
            vocoder.check_anonymize_options(dict(base, **extra), {}, {})
        assert str(e.value) == line
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "option_refusals.json")))
    assert line in json.dumps(golden)
