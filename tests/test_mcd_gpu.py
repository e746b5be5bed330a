"""GPU checks of the mel-cepstral distortion scorer (csrc/sa_mcd.hip, ops.mcd, metrics.
mel_cepstral_distortion) against the fp64 restatement tests/mcd_ref.py: a matrix product for the cepstra and a plain
row-by-row recurrence over the full matrix, not the kernel's anti-diagonals.

The bar, per output:   |value - ref| <= 16 x D + 2^-24 |ref|

  D             tools/mcd_delta.py re-evaluates the restatement on these same cases with the cepstra rounded to fp32,
                the cosine table rounded to fp32, the sums and the recurrence in fp32 and the sum over the
                coefficients reversed: the worst |delta| is 8.0e-7 dB for mcd and 6.5e-7 dB for mcd_sync; on the
                waveform-level case, with the log-Mel front end in fp32 as a fifth, 6.1e-7 and 2.1e-7 dB
                (tests/test_mcd_cpu.py holds mcd_ref.DELTA_MEASURED and DELTA_WAVE_MEASURED to the tool's output)
  2^-24 |ref|   the fp32 rounding of the value that is returned

frames is exact.  Nothing here is measured on the kernel."""
import ctypes
import errno
import os

import numpy as np
import pytest
import torch

from tests import anon_cli
from tests import mcd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
POISON = -7
gpu = pytest.mark.gpu


def _f(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(*arrays):
    return [torch.as_tensor(np.asarray(v)).to(DEV).contiguous() for v in arrays]


def _poisoned(B):
    return (torch.full((B,), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV),
            torch.full((B,), POISON, dtype=torch.int32, device=DEV))


def _launch(ref, deg, n_ref, n_deg, order, band):
    """sa_mcd through the library itself, into outputs poisoned with NaN and -7 and a workspace of NaN -> a dict of
    CPU tensors"""
    from speech_anonymization_amd import _lib, ops
    ref, deg, n_ref, n_deg = _dev(ref, deg, n_ref, n_deg)
    B, T_ref, n_mels = ref.shape
    T_deg = deg.shape[1]
    mcd, sync, frames = _poisoned(B)
    ws = ops.mcd_workspace(B, T_ref, T_deg, order, band, DEV).fill_(float("nan"))
    rc = _lib.load().sa_mcd(_f(ref), _f(deg), _f(n_ref), _f(n_deg), B, T_ref, T_deg, n_mels, order, band, _f(ws),
                            _f(mcd), _f(sync), _f(frames), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return {"mcd": mcd.cpu(), "mcd_sync": sync.cpu(), "frames": frames.cpu()}


def _bound(ref, deg, n_ref, n_deg, order, band):
    from speech_anonymization_amd import ops
    out = ops.mcd(*_dev(ref, deg, n_ref, n_deg), order=order, band=band)
    assert all(v.is_cuda for v in out)
    return dict(zip(("mcd", "mcd_sync", "frames"), (v.cpu() for v in out)))


def _bits(t):
    return t.view(torch.int32)


def _within(name, got, want, wave=False):
    """every scored row within the bar, every other row three zeros, frames exact; each figure printed first"""
    np.testing.assert_array_equal(got["frames"].numpy(), want.frames)
    for k in R.OUTPUTS:
        ref = getattr(want, k)
        assert bool(torch.isfinite(got[k]).all()), k                               # written over the NaN
        for b in range(len(ref)):
            bar, err = R.bar(k, ref[b], wave), abs(float(got[k][b]) - ref[b])
            print(f"{name} row {b}: {k} {float(got[k][b]):.9f} ref {ref[b]:.9f} error {err:.3e} bar {bar:.3e}")
            assert err <= bar, (name, b, k, err, bar)
            if want.frames[b] == 0:
                assert float(got[k][b]) == 0.0                                     # exactly 0, not merely near


CASES = R.gpu_cases()


@pytest.fixture(scope="module", params=range(len(CASES)), ids=lambda i: CASES[i][0])
def case(request):
    """(the case, its restatement, the raw call's outputs): computed once per case, left unchanged"""
    c = CASES[request.param]
    return c, R.case_ref(c[0]), _launch(*c[1:])


@gpu
def test_raw_call_against_fp64(case):
    (name, *_), want, got = case
    _within(name, got, want)


@gpu
def test_binding_against_fp64_and_two_runs_give_the_same_bits(case):
    (name, *args), want, first = case
    bound = _bound(*args)
    _within(name + " (ops.mcd)", bound, want)
    again = _launch(*args)
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(again[k])), k
        assert torch.equal(_bits(first[k]), _bits(bound[k])), k


@gpu
def test_symmetric_within_the_bar(case):
    (name, ref, deg, n_ref, n_deg, order, band), want, first = case
    swapped = _launch(deg, ref, n_deg, n_ref, order, band)
    assert torch.equal(swapped["frames"], first["frames"])
    for k in R.OUTPUTS:
        for b in range(len(n_ref)):
            diff = abs(float(first[k][b]) - float(swapped[k][b]))
            print(f"{name} row {b}: {k} {float(first[k][b]):.9f} swapped {float(swapped[k][b]):.9f}")
            assert diff <= R.bar(k, getattr(want, k)[b]), (name, b, k)


# ---------------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------------
@gpu
def test_identical_inputs_score_exactly_zero():
    name, ref, _, n_ref, _, order, band = next(c for c in CASES if c[0] == "R16_K13_0")
    got = _launch(ref, ref, n_ref, n_ref, order, band)
    assert got["mcd"].tolist() == [0.0] * 4 and got["mcd_sync"].tolist() == [0.0] * 4
    assert got["frames"].tolist() == (2 * n_ref).tolist()


@gpu
@pytest.mark.parametrize("band", [7, 63])
def test_a_delay_of_the_band_costs_exactly_nothing_and_one_more_frame_something(band):
    """deg = ref delayed by s frames with the first frame repeated, the last s + 1 frames of ref equal: the path
    (0, 0..s), the offset s, (T-s-1..T-1, T-1) has d = 0 at every cell and lies in the band iff s <= R"""
    T = 130
    f = R.mel_field(T, 77 + band)
    n = np.array([T, T], np.int32)
    pairs = [R.delayed(f, band), R.delayed(f, band + 1)]
    ref, deg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    got = _launch(ref, deg, n, n, R.ORDER, band)
    want = R.score(ref, deg, n, n, R.ORDER, band)
    print("band", band, "mcd", got["mcd"].tolist(), "mcd_sync", got["mcd_sync"].tolist(), "fp64", want.mcd.tolist())
    assert want.mcd[0] == 0.0 and want.mcd[1] > 0.0
    assert float(got["mcd"][0]) == 0.0 and float(got["mcd"][1]) > 0.0
    assert float(got["mcd_sync"][0]) > 0.0 and float(got["mcd_sync"][1]) > 0.0
    _within(f"delay {band}", got, want)


# ---------------------------------------------------------------------------------------------------
# the waveform-level figure
# ---------------------------------------------------------------------------------------------------
@gpu
def test_waveforms_against_the_fp64_front_end():
    """the glide and the vibrato row against their tilted, delayed copy: features.Fbank, the clamp and sa_mcd against
    mcd_ref.log_mel and the restatement"""
    from speech_anonymization_amd import metrics
    ref, deg, nv = R.wave_case()
    out = metrics.mel_cepstral_distortion(*_dev(ref, deg, nv))
    got = dict(zip(("mcd", "mcd_sync", "frames"), (v.cpu() for v in out)))
    want = R.wave_ref()
    assert want.frames.tolist() == [302, 252] and bool((want.mcd < want.mcd_sync).all())
    _within("wave", got, want, wave=True)


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
@gpu
def test_entry_point_refuses_before_it_launches():
    """-EINVAL, and the poisoned outputs untouched"""
    from speech_anonymization_amd import _lib, ops
    lib, E = _lib.load(), -errno.EINVAL
    B, T = 2, 9
    mel = torch.zeros(B, T, 80, device=DEV)
    n = torch.full((B,), T, dtype=torch.int32, device=DEV)
    mcd, sync, frames = _poisoned(B)
    ws = ops.mcd_workspace(B, T, T, 32, 63, DEV)

    def call(ref=mel, deg=mel, n_ref=n, n_deg=n, B=B, T_ref=T, T_deg=T, n_mels=80, order=13, band=16, ws=ws, mcd=mcd,
             sync=sync, frames=frames):
        return lib.sa_mcd(_f(ref), _f(deg), _f(n_ref), _f(n_deg), B, T_ref, T_deg, n_mels, order, band, _f(ws),
                          _f(mcd), _f(sync), _f(frames), _lib.stream())

    for bad in (dict(ref=None), dict(deg=None), dict(n_ref=None), dict(n_deg=None), dict(ws=None), dict(mcd=None),
                dict(sync=None), dict(frames=None), dict(B=0), dict(B=-1), dict(B=65536), dict(T_ref=0),
                dict(T_deg=0), dict(T_ref=104859), dict(T_deg=-3), dict(n_mels=1), dict(n_mels=129),
                dict(order=0), dict(order=33), dict(order=13, n_mels=13), dict(band=-1), dict(band=64)):
        assert call(**bad) == E, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(mcd).all()) and bool(torch.isnan(sync).all()) and bool((frames == POISON).all())


@gpu
def test_binding_refuses_before_it_launches(monkeypatch):
    from speech_anonymization_amd import _lib, ops, vocoder
    real = _lib.load()
    assert (vocoder.MCD_MAX_BAND, vocoder.MCD_MAX_ORDER) == (real.sa_mcd_dim(0), real.sa_mcd_dim(1))

    class NoLaunch:
        def __getattr__(self, name):
            if name == "sa_mcd":
                raise AssertionError("sa_mcd was reached")
            return getattr(real, name)

    monkeypatch.setattr(_lib, "load", lambda: NoLaunch())
    S = _lib.SaHipError
    mel = torch.zeros(2, 9, 80, device=DEV)
    n = torch.full((2,), 9, dtype=torch.int32, device=DEV)
    with pytest.raises(S, match=r"mel_ref: expected \[B, T, n_mels\]"):
        ops.mcd(mel[0], mel[0], n, n)
    with pytest.raises(S, match=r"mel_deg: expected \[B, T, n_mels\]"):
        ops.mcd(mel, mel[0], n, n)
    with pytest.raises(S, match=r"mel_deg: expected \[2, T, 80\]"):
        ops.mcd(mel, mel[:1], n, n)
    with pytest.raises(S, match=r"mel_deg: expected \[2, T, 80\]"):
        ops.mcd(mel, mel[:, :, :40].contiguous(), n, n)
    with pytest.raises(S, match="n_deg: expected shape"):
        ops.mcd(mel, mel, n, n[:1])
    with pytest.raises(S, match="n_ref: expected torch.int32"):
        ops.mcd(mel, mel, n.long(), n)
    with pytest.raises(S, match="mel_deg: expected torch.float32"):
        ops.mcd(mel, mel.double(), n, n)
    with pytest.raises(S, match="mel_ref: expected a contiguous tensor"):
        ops.mcd(mel.transpose(0, 1).contiguous().transpose(0, 1), mel, n, n)
    with pytest.raises(S, match="mel_deg: the MCD kernels take GPU tensors"):
        ops.mcd(mel, mel.cpu(), n, n)
    with pytest.raises(S, match="n_ref: the MCD kernels take GPU tensors"):
        ops.mcd(mel, mel, n.cpu(), n)
    for kw in (dict(order=0), dict(order=33), dict(band=-1), dict(band=64), dict(order=True), dict(band=2.0)):
        with pytest.raises(S, match=r"order in 1\.\.32 and below n_mels = 80, band in 0\.\.63"):
            ops.mcd(mel, mel, n, n, **kw)
    with pytest.raises(S, match="below n_mels = 8"):
        ops.mcd(mel[:, :, :8].contiguous(), mel[:, :, :8].contiguous(), n, n, order=8)
    with pytest.raises(AssertionError, match="sa_mcd was reached"):                 # the guard itself
        ops.mcd(mel, mel, n, n)


# ---------------------------------------------------------------------------------------------------
# end to end: anonymize.py in fresh child processes
# ---------------------------------------------------------------------------------------------------
ROWS = anon_cli.ROWS
UTT_KEYS = {"mcd_db", "mcd_sync_db", "mcd_frames"}
SUM_KEYS = {"mcd_mean", "mcd_sync_mean", "mcd_scored"}


@gpu
def test_anonymize_reports_an_identity(tmp_path):
    """--mcadams 1.0 copies every row bit for bit: the two spectra are the same"""
    res, utts = anon_cli.child(tmp_path, "on", ["--mcadams", "1.0", "--report_mcd", "true"])
    assert sorted(utts) == sorted(ROWS)
    for u in utts.values():
        assert UTT_KEYS <= set(u)
        assert u["mcd_db"] == 0.0 == u["mcd_sync_db"] and u["mcd_frames"] > 200
    assert SUM_KEYS <= set(res)
    assert res["mcd_mean"] == 0.0 and res["mcd_sync_mean"] == 0.0 and res["mcd_scored"] == 2
    plain, putts = anon_cli.child(tmp_path, "off", ["--mcadams", "1.0"])
    assert not SUM_KEYS & set(plain) and not any(UTT_KEYS & set(u) for u in putts.values())
    assert sorted(putts) == sorted(utts)


@gpu
def test_anonymize_reports_a_moved_envelope(tmp_path):
    """--formant_ratio 1.15 --phase vocoder: the envelope moves, and at equal counts an alignment cannot cost more
    than none.  No absolute figure is asserted: synthetic glides say nothing about speech."""
    res, utts = anon_cli.child(tmp_path, "f", ["--formant_ratio", "1.15", "--phase", "vocoder", "--report_mcd", "true",
                                               "--mcd_band", "16", "--mcd_order", "13"])
    for name in ROWS:
        u = utts[name]
        print(f"formant_ratio 1.15 {name}: mcd_db {u['mcd_db']!r} mcd_sync_db {u['mcd_sync_db']!r} frames "
              f"{u['mcd_frames']}")
        assert 0.0 < u["mcd_db"] <= u["mcd_sync_db"] + R.bar("mcd", u["mcd_sync_db"], wave=True), name
        assert u["mcd_frames"] > 200
    assert res["mcd_scored"] == 2 and 0.0 < res["mcd_mean"] <= res["mcd_sync_mean"] + R.bar("mcd", 4.0, wave=True)
