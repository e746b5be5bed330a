"""CPU checks of the mel-cepstral distortion scorer: the fp64 restatement tests/mcd_ref.py against
closed forms, its constants held to tools/mcd_delta.py, the option checks, and the plumbing that needs no GPU."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mcd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(ref, deg, order=R.ORDER, band=R.BAND, n_ref=None, n_deg=None, **kw):
    """a single row through the restatement -> (mcd, mcd_sync, frames)"""
    ref, deg = np.asarray(ref, dtype=np.float64), np.asarray(deg, dtype=np.float64)
    r = R.score(ref[None], deg[None], [ref.shape[0] if n_ref is None else n_ref],
                [deg.shape[0] if n_deg is None else n_deg], order, band, **kw)
    return float(r.mcd[0]), float(r.mcd_sync[0]), int(r.frames[0])


def pair(N=40, M=40, seed=5):
    f = R.mel_field(N, seed)
    return f, R.warped(f, M, seed + 1)


# ---------------------------------------------------------------------------------------------------
# the restatement against closed forms
# ---------------------------------------------------------------------------------------------------
def test_identical_inputs_score_exactly_zero():
    ref, _ = pair()
    assert one(ref, ref) == (0.0, 0.0, 80)
    assert one(ref, ref, band=0, order=32) == (0.0, 0.0, 80)


def test_a_gain_changes_neither_figure():
    ref, deg = pair()
    a, b = one(ref, deg), one(ref, deg + 7.25)
    print("gain 7.25 dB: mcd", a[0], b[0], "mcd_sync", a[1], b[1])
    assert a[0] > 1.0 and abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-12 and a[2] == b[2] == 80


def test_alignment_never_costs_more_than_none_at_equal_counts():
    for seed, band in ((5, 16), (9, 1), (13, 63)):
        ref, deg = pair(seed=seed)
        mcd, sync, _ = one(ref, deg, band=band)
        print("band", band, "mcd", mcd, "mcd_sync", sync)
        assert mcd <= sync


def test_symmetric_in_its_inputs():
    ref, deg = pair(40, 33)
    a, b = one(ref, deg), one(deg, ref)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] == 73 and a[0] > 0


def _ramp(levels):
    """[len, 4] Mel rows whose only cepstrum c_1 is levels / sqrt(2), so that d(i, j) = |x_i - y_j| at order 1"""
    basis = np.cos(np.pi * (np.arange(4) + 0.5) / 4.0)                 # sum of squares: n_mels / 2
    return 2.0 * math.sqrt(2.0) * np.asarray(levels, dtype=np.float64)[:, None] * basis[None, :]


def test_a_three_by_three_case_by_hand():
    """x = (0, 1, 3), y = (0, 3, 3):  d = [[0, 3, 3], [1, 2, 2], [3, 0, 0]];  g = [[0, 3, 6], [1, 3, 5], [4, 1, 1]]
    (g(1,1) = min(0 + 4, 3 + 2, 1 + 2), g(2,1) = min(1 + 0, 3 + 0, 4 + 0), g(2,2) = min(3, 5, 1) + 0):
    mcd = 1 / 6, mcd_sync = (0 + 2 + 0) / 3.  Band 1 takes g(0,2) and g(2,0) away and changes nothing; band 0 leaves
    the diagonal: (0 + 2 x 2 + 0) / 6."""
    ref, deg = _ramp([0.0, 1.0, 3.0]), _ramp([0.0, 3.0, 3.0])
    d = R.distances(R.cepstra(ref, 1), R.cepstra(deg, 1))
    assert np.abs(d - np.array([[0.0, 3.0, 3.0], [1.0, 2.0, 2.0], [3.0, 0.0, 0.0]])).max() <= 1e-12
    for band, want in ((2, 1.0 / 6.0), (1, 1.0 / 6.0), (0, 2.0 / 3.0)):
        mcd, sync, frames = one(ref, deg, order=1, band=band)
        assert abs(mcd - want) <= 1e-12 and abs(sync - 2.0 / 3.0) <= 1e-12 and frames == 6, band


def test_band_zero_is_the_frame_synchronous_figure():
    ref, deg = pair(seed=21)
    mcd, sync, _ = one(ref, deg, band=0)
    assert sync > 1.0 and abs(mcd - sync) <= 1e-12
    # (g = 2 sum d over 2 N frames against sum d over N)


def test_counts_decide_what_is_scored_and_what_is_read():
    ref, deg = pair(40, 40)
    assert one(ref, deg, band=3, n_deg=36) == (0.0, 0.0, 0)             # |N - M| = 4 > R
    assert one(ref, deg, band=4, n_deg=36)[2] == 76
    assert one(ref, deg, n_ref=0) == (0.0, 0.0, 0) and one(ref, deg, n_deg=-2) == (0.0, 0.0, 0)
    want = one(ref[:30], deg[:28])
    bad_ref, bad_deg = ref.copy(), deg.copy()
    bad_ref[30:], bad_deg[28:] = np.nan, np.nan
    assert one(bad_ref, bad_deg, n_ref=30, n_deg=28) == want
    assert one(ref, deg, n_ref=1000, n_deg=1000) == one(ref, deg)       # clamped to T


def test_a_delay_within_the_band_costs_nothing():
    f = R.mel_field(30, 3)
    for s in (1, 7):
        ref, deg = R.delayed(f, s)
        mcd, sync, _ = one(ref, deg, band=s)
        assert mcd == 0.0 and sync > 0.5
        assert one(ref, deg, band=s - 1)[0] > 0.0


def test_the_front_end_is_the_projects():
    """mcd_ref.log_mel against the CPU oracle of the feature front end on the waveform case (fp32 there: 1e-3 dB is
    far above its rounding and far below a wrong window, filter or clamp)"""
    from oracle import features as O
    ref, _, _ = R.wave_case()
    mine = R.log_mel(ref)
    theirs = O.Fbank()(torch.from_numpy(ref)).double().numpy()
    assert mine.shape == theirs.shape == (2, 151, 80)
    print("log_mel against the oracle: worst", np.abs(mine - theirs).max(), "dB")
    assert np.abs(mine - theirs).max() <= 1e-3


def test_gpu_cases_cover_what_they_are_meant_to():
    cases = R.gpu_cases()
    assert len(cases) == 2 * len(R.BANDS) * len(R.ORDERS)
    for band in R.BANDS:
        for order in R.ORDERS:
            rows = R.case_rows(band, order)
            assert sorted({n - m for n, m in rows}) == sorted({-band, -1, 0, 1, band, band + 1})
            assert all(n >= 1 and m >= 1 and (n in R.LENGTHS or m in R.LENGTHS) for n, m in rows)
        counts = {c for order in R.ORDERS for row in R.case_rows(band, order) for c in row}
        assert set(R.LENGTHS) <= counts, band                           # every length at every band
    for name, ref, deg, n_ref, n_deg, order, band in cases:
        assert ref.dtype == deg.dtype == np.float32 and n_ref.dtype == n_deg.dtype == np.int32
        assert ref.shape == (4, int(n_ref.max()) + 2, 80) and deg.shape == (4, int(n_deg.max()) + 2, 80)
        want = R.case_ref(name)
        for b in range(4):
            assert np.isnan(ref[b, n_ref[b]:]).all() and np.isfinite(ref[b, :n_ref[b]]).all()
            assert np.isnan(deg[b, n_deg[b]:]).all() and np.isfinite(deg[b, :n_deg[b]]).all()
            scored = abs(int(n_ref[b]) - int(n_deg[b])) <= band
            assert want.frames[b] == (n_ref[b] + n_deg[b] if scored else 0)
            assert (want.mcd[b] > 0.5 and want.mcd_sync[b] > 0.5) if scored else \
                (want.mcd[b] == 0.0 and want.mcd_sync[b] == 0.0)
    unscored = sum(int((R.case_ref(c[0]).frames == 0).sum()) for c in cases)
    assert unscored >= len(R.BANDS) * len(R.ORDERS)                     # the row at R + 1 of every setting


@pytest.fixture(scope="module")
def delta():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mcd_delta.py")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_bars_are_the_ones_the_delta_tool_measures(delta):
    """tools/mcd_delta.py: the perturbed evaluations; the bars the GPU tests use are 16 x their worst"""
    print("worst", delta["worst"], "worst_wave", delta["worst_wave"])
    for k in R.OUTPUTS:
        for held, got in ((R.DELTA_MEASURED[k], delta["worst"][k]), (R.DELTA_WAVE_MEASURED[k], delta["worst_wave"][k])):
            assert held * 0.9 <= got <= held * 1.001, k
    assert R.BAR_FACTOR == delta["factor"] == 16.0
    assert set(delta["by_perturbation"]) == set(R.PERTURBATIONS) == {"cep32", "cos32", "sum32", "reverse"}
    assert set(delta["by_perturbation_wave"]) == set(R.PERTURBATIONS) | {"front32"}
    assert delta["by_perturbation_wave"]["front32"]["mcd"] > 0.0
    assert max(R.bar(k, 4.0, wave) for k in R.OUTPUTS for wave in (False, True)) <= 2e-5     # dB


# ---------------------------------------------------------------------------------------------------
# option checks
# ---------------------------------------------------------------------------------------------------
MODES = [dict(model_type="convae", recon_ckpt="/x"), dict(model_type="fcae", passthrough=True), dict(pitch_norm=True),
         dict(pitch_norm=True, preserve_formants=True), dict(formant_ratio=1.15), dict(mcadams=0.8)]


@pytest.mark.parametrize("mode", MODES)
def test_report_mcd_is_accepted_in_every_mode(mode):
    from speech_anonymization_amd import vocoder
    base = dict({"out_dir": "o", "synthetic": 2}, **mode)
    assert vocoder.check_anonymize_options(dict(base), {}, {}) is None      # as before without the new keys
    for extra in (dict(report_mcd=True), dict(report_mcd=False), dict(report_mcd=True, mcd_band=0),
                  dict(report_mcd=True, mcd_band=63), dict(report_mcd=True, mcd_order=1),
                  dict(report_mcd=True, mcd_order=32, mcd_band=7), dict(report_mcd=True, report_stoi=True),
                  dict(report_mcd=True, report_prosody=True, prosody_max_lag=4),
                  dict(report_mcd=False, sample_rate=8000)):
        assert vocoder.check_anonymize_options(dict(base, **extra), {}, {}) is None
    with pytest.raises(SystemExit, match="^--report_mcd 'yes': true or false$"):
        vocoder.check_anonymize_options(dict(base, report_mcd="yes"), {}, {})
    with pytest.raises(SystemExit, match="^--report_mcd true scores 16 kHz waveforms only$"):
        vocoder.check_anonymize_options(dict(base, report_mcd=True, sample_rate=8000), {}, {})
    for bad in (-1, 64, 2.5, "4", True):
        with pytest.raises(SystemExit, match=r"^--mcd_band .*: a count of frames in 0\.\.63$"):
            vocoder.check_anonymize_options(dict(base, report_mcd=True, mcd_band=bad), {}, {})
    for bad in (0, 33, 2.5, "4", True):
        with pytest.raises(SystemExit, match=r"^--mcd_order .*: a count of cepstral coefficients in 1\.\.32$"):
            vocoder.check_anonymize_options(dict(base, report_mcd=True, mcd_order=bad), {}, {})
    for flag in (dict(), dict(report_mcd=False)):
        for key in ("mcd_band", "mcd_order"):
            with pytest.raises(SystemExit, match=f"^--{key} needs --report_mcd true: nothing else compares two "
                                                 "spectral envelopes$"):
                vocoder.check_anonymize_options(dict(base, **{key: 4}, **flag), {}, {})


def test_the_new_checks_come_after_the_prosody_ones():
    """an older refusal still wins: no existing text changes its place"""
    from speech_anonymization_amd import vocoder
    base = {"out_dir": "o", "synthetic": 2, "mcadams": 0.8, "report_mcd": "yes"}
    with pytest.raises(SystemExit, match="^--prosody_max_lag needs --report_prosody true"):
        vocoder.check_anonymize_options(dict(base, prosody_max_lag=4), {}, {})
    with pytest.raises(SystemExit, match="^--report_mcd 'yes': true or false$"):
        vocoder.check_anonymize_options(dict(base, n_iter=-1), {}, {})


# ---------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------
def test_mcd_dim_exports_the_constants():
    from speech_anonymization_amd import _lib, ops, vocoder
    lib = _lib.load()
    assert [lib.sa_mcd_dim(i) for i in range(4)] == [63, 32, 128, 104858]
    assert lib.sa_mcd_dim(4) == -22 and lib.sa_mcd_dim(-1) == -22
    assert ops.MCD_MAX_BAND == vocoder.MCD_MAX_BAND == R.MAX_BAND == 63
    assert ops.MCD_MAX_ORDER == vocoder.MCD_MAX_ORDER == R.MAX_ORDER == 32
    assert (vocoder.MCD_BAND_DEFAULT, vocoder.MCD_ORDER_DEFAULT) == (R.BAND, R.ORDER) == (16, 13)
    assert ops.mcd_workspace(2, 5, 7, 13, 16, "cpu").numel() == 2 * (13 * 12 + 17 * 11)
    # a null pointer or a bad size is refused before anything is launched (no GPU is needed to be told so)
    assert lib.sa_mcd(None, None, None, None, 1, 5, 5, 80, 13, 16, None, None, None, None, None) == -22


def test_binding_refuses_cpu_tensors_before_it_loads_anything(monkeypatch):
    from speech_anonymization_amd import _lib, ops

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    x, n = torch.zeros(2, 9, 80), torch.full((2,), 9, dtype=torch.int32)
    with pytest.raises(_lib.SaHipError, match="mel_ref: the MCD kernels take GPU tensors"):
        ops.mcd(x, x, n, n)
    with pytest.raises(_lib.SaHipError, match="mel_ref: the MCD kernels take GPU tensors"):
        ops.mcd(x.numpy(), x, n, n)


def test_cepstral_stats_average_the_scored_rows():
    from speech_anonymization_amd.metrics import CepstralStats
    st = CepstralStats()
    assert st.summarize() == {"mcd": None, "mcd_sync": None, "scored": 0, "unscored": 0}
    st.append(["a", "b", "c"], torch.tensor([2.0, 0.0, 4.0]), torch.tensor([3.0, 0.0, 4.5]),
              torch.tensor([300, 0, 12], dtype=torch.int32))
    st.append(["d"], torch.tensor([0.0]), torch.tensor([0.75]), torch.tensor([2], dtype=torch.int32))
    st.append(["e"], torch.tensor([float("nan")]), torch.tensor([float("nan")]), torch.tensor([0], dtype=torch.int32))
    assert st.summarize() == {"mcd": 2.0, "mcd_sync": 2.75, "scored": 3, "unscored": 2}
    assert st.ids == ["a", "b", "c", "d", "e"]
    st.clear()
    assert st.summarize()["scored"] == 0 and st.ids == []
