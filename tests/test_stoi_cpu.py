"""CPU checks of the STOI / ESTOI scorer: the fp64 restatement tests/stoi_ref.py against what is
independent of it (the band rule, scipy's polyphase resampler, the measures' own properties), the condition the GPU
test's inputs have to meet (no keep decision near its threshold), and the plumbing that needs no GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import stoi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16000


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def test_band_table_follows_from_the_rule():
    assert R.band_table() == R.BANDS
    assert R.BANDS == ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69),
                       (69, 87), (87, 109), (109, 138), (138, 174), (174, 219))


def test_window_is_numpy_hanning():
    assert np.abs(R.WINDOW - np.hanning(258)[1:-1]).max() <= 1e-15
    assert R.TAPS.shape == (161,) and R.TAPS[80] == 0.625 and np.array_equal(R.TAPS, R.TAPS[::-1])


def test_resampler_equals_scipy_resample_poly():
    """the one independent check of the resampling indices (scipy multiplies the taps by ``up`` itself)"""
    import scipy.signal
    x = np.random.default_rng(0).standard_normal(8000)
    got = R.resample(x, 8000)
    want = scipy.signal.resample_poly(x, 5, 8, window=R.TAPS / 5)
    assert got.shape == want.shape == (5000,)
    print("resampler against scipy:", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-12
    x[6001:] = 0.0                                          # a sample at or beyond n_valid reads as 0
    short = R.resample(x, 6001)
    assert short.shape == (R.n10_of(6001),) == (3751,)
    assert np.abs(short - scipy.signal.resample_poly(x, 5, 8, window=R.TAPS / 5)[:3751]).max() <= 1e-12


@pytest.fixture(scope="module")
def clean():
    x = R.harmonic_row(N, 1)[None]
    return x, R.stoi(x, x, [N])


def test_identical_signals_score_one(clean):
    x, same = clean
    print("score(x, x):", same.stoi[0], "1 -", 1.0 - same.estoi[0])
    assert same.frames[0] == 77 and same.segments[0] == 48
    assert same.stoi[0] >= 1.0 - 1e-9 and same.estoi[0] >= 1.0 - 1e-9


def test_scores_do_not_depend_on_the_level(clean):
    x, same = clean
    loud = R.stoi(x, 3.0 * x, [N])
    assert abs(loud.stoi[0] - same.stoi[0]) <= 1e-9 and abs(loud.estoi[0] - same.estoi[0]) <= 1e-9


def test_both_measures_increase_with_the_snr(clean):
    x, _ = clean
    noise = R.white(N, 99)
    got = [R.stoi(x, R.at_snr(x[0], noise, snr)[None], [N]) for snr in (-5.0, 0.0, 10.0, 20.0)]
    st, es = [float(g.stoi[0]) for g in got], [float(g.estoi[0]) for g in got]
    print("STOI", st, "ESTOI", es)
    assert all(a < b for a, b in zip(st, st[1:])) and all(a < b for a, b in zip(es, es[1:]))


def test_rows_without_a_segment_score_zero():
    x = R.harmonic_row(8000, 1)[None]
    for ref, deg, nv in ((x, x, [0]), (np.zeros_like(x), x, [8000]), (x[:, :6346], x[:, :6346], [6346]),
                         (x[:, :300], x[:, :300], [300])):
        r = R.stoi(ref, deg, nv)
        assert r.segments[0] == 0 and r.stoi[0] == 0.0 and r.estoi[0] == 0.0
    assert R.stoi(x, np.zeros_like(x), [8000]).stoi[0] == 0.0


# ---------------------------------------------------------------------------------------------------
# the GPU test's inputs
# ---------------------------------------------------------------------------------------------------
def test_gpu_cases_keep_clear_of_every_keep_decision():
    """a flipped keep decision changes the whole row: no frame energy within 1 +- 1e-6 of its row's threshold, in no
    row of no case, and the kept-frame counts are the ones each case is meant to exercise"""
    names = [c[0] for c in R.gpu_cases()]
    assert names == ["rows", "one", "none", "empty", "zero_deg", "mcadams"]
    for name, ref, deg, nv, want in R.gpu_cases():
        r = R.case_ref(name)
        assert ref.dtype == deg.dtype == np.float32 and nv.dtype == np.int32 and ref.shape == deg.shape
        print(name, "frames", r.frames.tolist(), "segments", r.segments.tolist(), "margin", r.margin.tolist())
        assert tuple(r.frames.tolist()) == want, name
        assert tuple(r.segments.tolist()) == tuple(max(k - 29, 0) for k in want), name
        assert (r.margin > R.MARGIN).all(), name
    rows = R.case_ref("rows")
    kept = np.nonzero(rows.energies[1] > R.RANGE * rows.energies[1].max())[0]
    assert (np.diff(kept) > 1).sum() == 1 and np.diff(kept).max() >= 4          # compaction joins frames 3+ apart
    assert rows.frames[1] >= 30
    one, none = R.case_ref("one"), R.case_ref("none")
    assert R.n10_of(6348) == 3968 and one.segments[0] == 1 and none.segments[0] == 0 and none.stoi[0] == 0.0
    assert not R.case_ref("zero_deg").stoi.any() and not R.case_ref("zero_deg").estoi.any()


def test_the_bar_is_the_one_the_delta_tool_measures():
    """tools/stoi_delta.py: the four perturbed evaluations; the bar the GPU test uses is 16 x their worst and stays
    under 1e-4"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stoi_delta.py")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for m in ("stoi", "estoi"):
        assert 0.0 < out["worst"][m] <= R.DELTA_MEASURED[m] * 1.001 and out["worst"][m] >= R.DELTA_MEASURED[m] * 0.9
        assert R.bar(m, 1.0) <= 1e-4
    assert out["smallest_margin"] > R.MARGIN


# ---------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------
def test_stoi_dim_exports_the_constants():
    from speech_anonymization_amd import _lib, ops
    lib = _lib.load()
    assert [lib.sa_stoi_dim(i) for i in range(7)] == [10000, 256, 128, 512, 15, 30, 161]
    assert lib.sa_stoi_dim(7) >= 1 and lib.sa_stoi_dim(8) >= 1 and lib.sa_stoi_dim(9) % 64 == 0
    assert lib.sa_stoi_dim(10) == -22 and lib.sa_stoi_dim(-1) == -22
    assert (ops.STOI_W, ops.STOI_H, ops.STOI_SEG, 2 * ops.STOI_HALF + 1) == (256, 128, 30, 161)
    assert ops.stoi_frames(160000) == (100000, 780) and ops.stoi_frames(100) == (63, 1)
    M, F = ops.stoi_frames(8001)
    assert ops.stoi_workspace(3, 8001, "cpu").numel() * 8 >= 8 * 3 * (2 * M + 33 * F) + 4 * 3 * (F + 2)


def test_taps_of_the_binding_are_the_restatement_s():
    from speech_anonymization_amd import ops
    t = ops.stoi_taps("cpu")
    assert t.dtype == torch.float64 and t.shape == (161,) and ops.stoi_taps("cpu") is t
    assert np.abs(t.numpy() - R.TAPS).max() <= 4e-16


def test_binding_refuses_before_it_loads_anything(monkeypatch):
    from speech_anonymization_amd import _lib, ops

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    x, nv = torch.zeros(2, 800), torch.full((2,), 800, dtype=torch.int32)
    with pytest.raises(_lib.SaHipError, match="ref: the STOI kernels take GPU tensors"):
        ops.stoi(x, x, nv)
    with pytest.raises(_lib.SaHipError, match="ref: the STOI kernels take GPU tensors"):
        ops.stoi(x.numpy(), x, nv)


@pytest.mark.parametrize("mode", [dict(model_type="convae", recon_ckpt="/x"), dict(model_type="fcae", passthrough=True),
                                  dict(pitch_norm=True), dict(pitch_norm=True, preserve_formants=True),
                                  dict(formant_ratio=1.15), dict(mcadams=0.8)])
def test_report_stoi_is_accepted_in_every_mode(mode):
    from speech_anonymization_amd import vocoder
    base = dict({"out_dir": "o", "synthetic": 2}, **mode)
    vocoder.check_anonymize_options(dict(base, report_stoi=True), {}, {})
    vocoder.check_anonymize_options(dict(base, report_stoi=False), {}, {})
    vocoder.check_anonymize_options(dict(base, report_stoi=True, report_f0=True), {}, {})
    with pytest.raises(SystemExit, match="--report_stoi 'yes': true or false"):
        vocoder.check_anonymize_options(dict(base, report_stoi="yes"), {}, {})
    with pytest.raises(SystemExit, match="16 kHz"):
        vocoder.check_anonymize_options(dict(base, report_stoi=True, sample_rate=8000), {}, {})
    vocoder.check_anonymize_options(dict(base, report_stoi=False, sample_rate=8000), {}, {})


def test_intelligibility_stats_average_the_scored_rows():
    from speech_anonymization_amd.metrics import IntelligibilityStats
    st = IntelligibilityStats()
    assert st.summarize() == {"stoi": None, "estoi": None, "scored": 0, "unscored": 0}
    st.append(["a", "b", "c"], torch.tensor([0.5, 0.0, 0.75]), torch.tensor([0.25, 0.0, 0.5]),
              torch.tensor([3, 0, 1], dtype=torch.int32))
    st.append(["d"], torch.tensor([1.0]), torch.tensor([0.0]), torch.tensor([7], dtype=torch.int32))
    st.append(["e"], torch.tensor([float("nan")]), torch.tensor([float("nan")]), torch.tensor([0], dtype=torch.int32))
    assert st.summarize() == {"stoi": 0.75, "estoi": 0.25, "scored": 3, "unscored": 2}
    assert st.ids == ["a", "b", "c", "d", "e"]
    st.clear()
    assert st.summarize()["scored"] == 0 and st.ids == []
