"""CPU: tests/fbank_ref.py (the fp64 arbiter of tests/test_frontend_gpu.py) against oracle.features run in
fp64, the direct DFT, numpy's FFT, the reference's normalizer pin and hand values; the bars of the GPU test
against tools/fbank_delta.py; and the sensitivity of the GPU test's metrics: every deliberately wrong variant of
the restatement below exceeds the bar on at least one of the GPU test's own cases."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import features as OF
from tests import fbank_ref as R
from tests import test_frontend_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "profiles", "fbank_delta.json")) as _f:
    DELTA = json.load(_f)


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


# ---- the tables are the kernel's -----------------------------------------------------------------
def test_window_and_mel_matrix_are_what_the_kernel_receives():
    from speech_anonymization_amd import features as HF
    assert np.array_equal(R.window().numpy(), HF._hamming(400).astype(np.float64))
    ow = OF.hamming_window(400)
    # torch evaluates the formula in fp32 (a few roundings: up to 2 ulp at 1); the kernel's table is the fp64 formula rounded
    assert float((R.window() - ow.double()).abs().max()) <= 3 * float(np.spacing(np.float32(1.0)))
    fb = R.mel_matrix32()
    assert fb.shape == (201, 80) and fb.dtype == torch.float32
    assert torch.equal(fb, OF.mel_filterbank())
    padded = HF._mel_matrix(80, 400, 16000)
    assert torch.equal(padded[:201, :80], fb) and float(padded[201:].abs().max()) == 0.0
    assert float(padded[:, 80:].abs().max()) == 0.0


# ---- Fbank ----------------------------------------------------------------------------------------
def test_power_equals_the_direct_dft_and_the_fft():
    wav = OF.synthetic_wave(2, 4000, seed=3)
    i = np.arange(400, dtype=np.float64)
    win64 = torch.from_numpy(0.54 - 0.46 * np.cos(2 * np.pi * i / 400))
    got = R.power(R.frames(wav) * win64)
    assert got.shape == (2, 26, 201)
    assert _rel(got, OF.power_spectrum_direct_dft(wav)) < 1e-12
    fft = np.abs(np.fft.rfft((R.frames(wav) * R.window()).numpy(), axis=-1)) ** 2
    assert _rel(R.power(R.frames(wav) * R.window()), fft) < 1e-12


@pytest.mark.parametrize("mode", ["utterance", "batch"])
@pytest.mark.parametrize("N", [1, 161, 401, 5119])
def test_fbank_equals_the_oracle_in_fp64(N, mode):
    wav = R.gpu_cases()[f"zero-{N}"]
    ofb = OF.Fbank(top_db_mode=mode)
    ofb.window, ofb.fb = R.window(), ofb.fb.double()
    want = ofb(wav.double())
    raw = R.raw_db(R.mel_energies(wav))
    got = R.clamped(raw, mode)
    assert got.shape == want.shape == (3, 1 + N // 160, 80)
    # the oracle clamps at the double 1e-10, the kernel (and the restatement) at 1e-10f: 5.8e-8 dB apart
    assert float((got - want).abs().max()) < 2e-7
    assert float(got[1].max()) == float(got[1].min())                    # the all-zero row is flat
    fl = R.floors(raw, mode)
    silence = 10.0 * np.log10(R.AMIN)                                    # -100 + 5.8e-8: 1e-10f is not 1e-10
    assert float(got[1].min()) == (silence if mode == "utterance" else max(silence, float(raw.max()) - 80.0))
    assert float(fl[1]) == (silence - 80.0 if mode == "utterance" else float(raw.max()) - 80.0)
    assert torch.equal(got, torch.maximum(raw, fl[:, None, None]))


def test_impulse_and_dc_by_hand():
    N = 5120
    rows = R.gpu_cases()[f"rows-{N}"]
    M = R.case_ref(f"rows-{N}")
    w, fb = R.window(), R.mel_matrix()
    # impulse of 1 at N // 2: frame t sees it at i = N // 2 + 200 - 160 t; the spectrum is flat, w[i]^2
    imp = M[R.SIGNALS.index("impulse")]
    for t in range(33):
        i = N // 2 + 200 - 160 * t
        want = (w[i] ** 2 if 0 <= i < 400 else 0.0) * fb.sum(0)
        assert float((imp[t] - want).abs().max()) <= 1e-13 * float(fb.sum(0).max())
    assert float(R.raw_db(imp[0]).max()) == float(R.raw_db(imp[0]).min()) == 10.0 * np.log10(R.AMIN)
    # DC 0.5: an inner frame is 0.5 w, its spectrum 0.5 W (the window's own transform, here by numpy's FFT)
    dc = M[R.SIGNALS.index("dc")]
    W2 = torch.from_numpy(np.abs(np.fft.rfft(w.numpy())) ** 2)
    assert _rel(dc[16], 0.25 * W2 @ fb) < 1e-12
    assert abs(float(R.power((0.5 * w)[None, None])[0, 0, 0]) - float(0.5 * w.sum()) ** 2) < 1e-9
    # the first frame holds 200 zeros and then the signal: bin 0 of its spectrum is the half window's sum
    P0 = R.power(R.frames(rows[R.SIGNALS.index("dc")][None]) * w)[0, 0]
    assert abs(float(P0[0]) - float(0.5 * w[200:].sum()) ** 2) < 1e-9


def test_frame_count_and_tiles():
    for N, T in zip(R.FBANK_N, (1, 1, 2, 2, 3, 3, 3, 32, 32, 33, 64, 65, 72)):
        assert R.case_ref(f"zero-{N}").shape == (3, T, 80) and R.gpu_cases()[f"rows-{N}"].shape == (9, N)
    fr = R.frames(torch.arange(1.0, 402.0)[None])                       # N = 401: T = 3
    assert fr.shape == (1, 3, 400)
    assert float(fr[0, 0, 199]) == 0.0 and float(fr[0, 0, 200]) == 1.0 and float(fr[0, 0, 399]) == 200.0
    assert float(fr[0, 2, 0]) == 121.0 and float(fr[0, 2, 280]) == 401.0 and float(fr[0, 2, 281]) == 0.0


# ---- normalisation --------------------------------------------------------------------------------
def test_round_half_even_of_the_fp32_product():
    assert list(R.frame_counts([0.5], 73)) == [36] and list(R.frame_counts([0.5], 75)) == [38]
    assert list(R.frame_counts([0.5, 0.5], 33)) == [16, 16] and list(R.frame_counts([0.5], 17)) == [8]
    assert list(R.frame_counts([0.25, 1.01, 1.0], 72)) == [18, 72, 72]
    assert list(R.frame_counts([1.04], 17)) == [17] and list(R.frame_counts([0.07, 0.125], 15)) == [1, 2]
    # the product is rounded to fp32 first: 0.7f * 15 = 10.499999523 in exact arithmetic, 10.5f in fp32 -> 10
    assert float(np.float32(0.7)) * 15 < 10.5 and list(R.frame_counts([0.7], 15)) == [10]
    for name, (xs, lens) in R.norm_cases().items():
        T = xs[0].shape[1]
        want = [min(int(torch.round(l * T)), T) for l in lens]
        assert list(R.frame_counts(lens.numpy(), T)) == want, name


def _oracle64(xs, lens, calls, state=None):
    nrm = OF.InputNormalization(update_until_epoch=R.UNTIL)
    if state is not None:
        nrm.count, nrm.glob_mean, nrm.glob_std = state[0], state[1].double(), state[2].double()
    res = []
    for i, (training, epoch) in enumerate(calls):
        nrm.training = training
        out = OF.pad_to_multiple(nrm(xs[i % len(xs)].double(), lens, epoch=epoch), 36)
        res.append((out, nrm.count, nrm.glob_mean.clone(), nrm.glob_std.clone()))
    return res


@pytest.mark.parametrize("name", [n for n in R.norm_cases() if "n1" not in n])
def test_normalisation_equals_the_oracle_in_fp64(name):
    xs, lens = R.norm_cases()[name]
    fresh, loaded = R.norm_case_ref(name)
    want = _oracle64(xs, lens, R.CALLS) + _oracle64(xs, lens, R.LOAD_CALL, R.loaded_state())
    assert [r[1] for r in fresh + loaded] == [1, 2, 3, 3, 6] == [w[1] for w in want]
    for (out, _, gm, gs), (wout, _, wgm, wgs) in zip(fresh + loaded, want):
        assert out.shape == wout.shape and out.shape[1] % 36 == 0
        assert _rel(gm, wgm) < 1e-12 and _rel(gs, wgs) < 1e-12
        # the constant column divides by 1e-10: compare what the division amplifies, not the quotient
        assert float(((out - wout).abs() * gs).max()) < 1e-11
        assert float(out[:, xs[0].shape[1]:].abs().max() if out.shape[1] > xs[0].shape[1] else 0.0) == 0.0
    assert torch.equal(fresh[2][2], fresh[1][2]) and torch.equal(fresh[3][3], fresh[1][3])       # frozen, eval


def test_one_frame_utterance_is_finite_with_the_floor():
    xs, lens = R.norm_cases()["B2-T15-n1"]
    assert list(R.frame_counts(lens.numpy(), 15)) == [15, 1]
    m, s = R.norm_stats(xs[0], lens)
    x = xs[0].double()
    assert torch.isfinite(m).all() and torch.isfinite(s).all()
    assert _rel(m, (x[0].mean(0) + x[1, 0]) / 2) < 1e-14
    assert _rel(s, (x[0].std(0) + R.AMIN) / 2) < 1e-14
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # torch says so itself: degrees of freedom <= 0
        bad = OF.InputNormalization()(xs[0], lens, epoch=1)              # the reference: NaN for good
    assert torch.isnan(bad).all()


def test_constant_row_and_column_hit_the_floor():
    xs, lens = R.norm_cases()["B2-T17-constcol"]
    m, s = R.norm_stats(xs[0], lens)
    assert float(s[11]) == R.AMIN and float(m[11]) == -30.25
    xs, lens = R.norm_cases()["B3-T33-constrow"]
    x = xs[0].double()
    _, s = R.norm_stats(xs[0], lens)
    assert _rel(s, (x[0].std(0) + R.AMIN + x[2, :23].std(0)) / 3) < 1e-14


def test_against_the_normalizer_pin(golden_dir):
    """the reference's own state loaded and frozen: the output undoes to the input, the count advances, and the
    state's keys are the ones the GPU test asks of state_dict()"""
    pins = json.load(open(os.path.join(golden_dir, "reference_pins.json")))["normalizer"]
    assert sorted(G.STATE_KEYS) == pins["keys"]
    gm, gs = torch.tensor(pins["glob_mean"]), torch.tensor(pins["glob_std"])
    xs, lens = R.norm_cases()["B3-T75-tie"]
    (out, count, gm2, gs2), = R.norm_sequence(xs, lens, [(True, 7)], R.UNTIL, (pins["count"], gm, gs))
    assert count == pins["count"] + 1 and torch.equal(gm2, gm.double()) and torch.equal(gs2, gs.double())
    assert out.shape == (3, 108, 80) and _rel(out[:, :75] * gs.double() + gm.double(), xs[0]) < 1e-14


# ---- the bars ---------------------------------------------------------------------------------------
def test_the_bars_are_the_ones_the_delta_tool_measured():
    assert DELTA["margin"] == 8.0
    assert DELTA["mel_delta"] == max(DELTA["mel_delta_stft"], DELTA["mel_delta_matmul"])
    assert G.MEL_DELTA_WORST == DELTA["mel_delta"] and G.MEL_BAR == 8.0 * DELTA["mel_delta"] == DELTA["mel_bar"]
    assert DELTA["norm_delta_u"] == max(DELTA["norm_delta_mean_u"], DELTA["norm_delta_std_u"], DELTA["norm_delta_out_u"])
    assert G.NORM_DELTA_WORST_U == DELTA["norm_delta_u"] and G.NORM_BAR_U == 8.0 * DELTA["norm_delta_u"]
    assert DELTA["floor_bar_db"] == pytest.approx(R.floor_bound(G.MEL_BAR), rel=1e-12)


def test_the_delta_tool_measures_them_again():
    """fp32 matmul and FFT results depend on the BLAS blocking and thread count of the machine, so the figures
    are held to a factor of two, not to the digit"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fbank_delta", os.path.join(ROOT, "tools", "fbank_delta.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with torch.no_grad():
        res = tool.measure()
    for key in ("mel_delta_stft", "mel_delta_matmul", "norm_delta_mean_u", "norm_delta_std_u", "norm_delta_out_u"):
        assert 0.5 * DELTA[key] <= res[key] <= 2.0 * DELTA[key], key


# ---- sensitivity: wrong variants of the restatement against the GPU test's metric and bar -----------
def _mel_from_frames(fr, win=None, fb=None, plane=False):
    x = fr * (R.window() if win is None else win)
    if plane:
        x = x.to(torch.bfloat16).double()
    return R.power(x) @ (R.mel_matrix() if fb is None else fb)


def _shifted(wav):
    w = wav.double()
    return _mel_from_frames(R.frames(torch.cat([torch.zeros(w.shape[0], 1, dtype=torch.float64), w[:, :-1]], 1)))


def _symmetric(wav):
    i = np.arange(400, dtype=np.float64)
    win = torch.from_numpy((0.54 - 0.46 * np.cos(2 * np.pi * i / 399)).astype(np.float32)).double()
    return _mel_from_frames(R.frames(wav), win=win)


def _reflect(wav):
    B, N = wav.shape
    if N <= 200:
        return None
    p = torch.nn.functional.pad(wav.double()[None], (200, 200), mode="reflect")[0]
    T = 1 + N // 160
    idx = (torch.arange(T) * 160)[:, None] + torch.arange(400)[None, :]
    return _mel_from_frames(p[:, idx])


def _stale_tile(wav):
    M = R.mel_energies(wav).clone()
    T = M.shape[1]
    t0 = (T - 1) // 32 * 32
    if T % 32 == 0 or t0 == 0:
        return None
    M[:, t0:] = M[:, t0 - 32:T - 32]
    return M


def _mel_one_plane(wav):
    return _mel_from_frames(R.frames(wav), fb=R.mel_matrix32().to(torch.bfloat16).double())


def _frames_one_plane(wav):
    return _mel_from_frames(R.frames(wav), plane=True)


MEL_VARIANTS = {"frame start off by one": _shifted, "symmetric window": _symmetric, "reflect padding": _reflect,
                "last partial tile from the tile before": _stale_tile, "Mel matrix in one bf16 plane": _mel_one_plane,
                "frames in one bf16 plane": _frames_one_plane}


def test_the_restatement_itself_scores_zero():
    for name in ("rows-401", "zero-5120"):
        assert float(R.mel_error(R.raw_db(R.case_ref(name)), R.case_ref(name)).max()) < 1e-12


@pytest.mark.parametrize("variant", list(MEL_VARIANTS))
def test_a_wrong_fbank_exceeds_the_bar(variant):
    worst = 0.0
    for name, wav in R.gpu_cases().items():
        M = MEL_VARIANTS[variant](wav)
        if M is None:
            continue
        worst = max(worst, float(R.mel_error(R.raw_db(M), R.case_ref(name)).max()))
        if worst > G.MEL_BAR:
            break
    print(f"{variant}: e = {worst:.3e} at {name}, bar {G.MEL_BAR:.3e}")
    assert worst > G.MEL_BAR


def test_the_batch_maximum_for_the_utterance_maximum_exceeds_the_floor_bar():
    raw = R.raw_db(R.case_ref("zero-5120"))
    d = (R.floors(raw, "batch") - R.floors(raw, "utterance")).abs()
    assert float(d.max()) > R.floor_bound(G.MEL_BAR)
    assert float(d[1]) > 100.0                                            # the all-zero row: -180 or the batch's floor


def _wrong_stats(kind):
    def stats(x, lens):
        x = R._t(x)
        B, T, _ = x.shape
        per = -(-T // R.CHUNKS)
        means, stds = [], []
        for b, n in enumerate(R.frame_counts(lens, T)):
            n = int(n)
            if kind == "floor":
                n = min(int(np.floor(np.float32(lens[b]) * np.float32(T))), T)
            v = x[b, :n]
            if kind == "chunk15":                                         # its frames never reach the sums
                v = x[b, :min(n, 15 * per)]
            m = v.sum(0) / n
            var = ((v * v).sum(0) - v.sum(0) * m) / ((n if kind == "biased" else n - 1)) if n > 1 else torch.zeros_like(m)
            means.append(m)
            stds.append(torch.sqrt(var.clamp(min=0.0)).clamp(min=R.AMIN))
        keep = 8 if kind == "lanes" else B                                # utterances 8.. never reach the batch mean
        return torch.stack(means[:keep]).sum(0) / B, torch.stack(stds[:keep]).sum(0) / B
    return stats


@pytest.mark.parametrize("kind", ["floor", "biased", "lanes", "chunk15"])
def test_wrong_statistics_exceed_the_bar(kind):
    worst, where = 0.0, None
    for name, (xs, lens) in R.norm_cases().items():
        got = R.norm_sequence(xs, lens, R.CALLS[:1], R.UNTIL, stats=_wrong_stats(kind))[0]
        e = max(R.norm_errors(got[0], got[2], got[3], xs[0], R.norm_case_ref(name)[0][0]))
        if e > worst:
            worst, where = e, name
    print(f"{kind}: {worst / G.U:.3e} u at {where}, bar {G.NORM_BAR_U:.1f} u")
    assert worst > G.NORM_BAR_U * G.U
    if kind == "chunk15":
        assert where in ("B3-T16-n2", "B32-T16-full", "B1-T1001-long")


def test_the_right_statistics_by_the_kernels_formula_score_zero():
    """the sum-of-squares form the kernel uses (fp64 partials) is the restatement's two-pass form to 0.01 u (0.002 u
    at offset -80 with std 0.05, where sq - s * m cancels eleven digits of fp64's sixteen)"""
    for name, (xs, lens) in R.norm_cases().items():
        got = R.norm_sequence(xs, lens, R.CALLS[:1], R.UNTIL, stats=_wrong_stats("none"))[0]
        e = max(R.norm_errors(got[0], got[2], got[3], xs[0], R.norm_case_ref(name)[0][0]))
        assert e < 1e-2 * G.U, name
