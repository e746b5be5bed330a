"""GPU checks of the pitch-correlation scorer (csrc/sa_prosody.hip, ops.f0_compare) against the
fp64 restatement tests/prosody_ref.py, which sums with numpy over fancy-indexed vectors, not in the kernel's order.

The bar, per real output:   |value - ref| <= 16 x D + 2^-24 |ref|

  D             tools/prosody_delta.py re-evaluates the restatement on these same cases with every sum from the far
                end, in numpy.longdouble, with log2 as ln / ln 2 and with every per-frame shift moved by 2 ulp: the
                worst |delta| is 1.2e-15 for rho, 5.3e-15 for shift_st, 8.9e-16 for dev_st and 0 for voicing
                (tests/test_prosody_cpu.py holds prosody_ref.DELTA_MEASURED to the tool's output)
  2^-24 |ref|   the fp32 rounding of the value that is returned

lag and common are exact: tests/test_prosody_cpu.py checks that the winning lag of every row leads every other valid
lag by more than 1e-6 (the exactly tied lags of the two tie cases apart) and that no s_xx, s_yy is near 0.

The end-to-end tests run anonymize.py in fresh child processes on the glide and the vibrato row of
tests/contour_ref.py; their margin (prosody_ref.E2E_MARGIN) is four times the spread between the fp64 path and its
fp32 variant, measured by the delta tool on the restatement."""
import ctypes
import errno
import os

import numpy as np
import pytest
import torch

from tests import anon_cli
from tests import prosody_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
POISON = -7
gpu = pytest.mark.gpu
REAL = ("rho", "shift_st", "dev_st", "voicing")


def _f(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _poisoned(B):
    real = [torch.full((B,), float("nan"), device=DEV) for _ in range(4)]
    ints = [torch.full((B,), POISON, dtype=torch.int32, device=DEV) for _ in range(2)]
    return real, ints


def _launch(ref, deg, frames, Lg, m, want=(True,) * 5):
    """sa_f0_compare through the library itself, into outputs poisoned with NaN and -7 -> a dict of CPU tensors;
    want: which of lag, common, shift_st, dev_st, voicing get a pointer"""
    from speech_anonymization_amd import _lib
    ref, deg, frames = (torch.as_tensor(np.asarray(v)).to(DEV).contiguous() for v in (ref, deg, frames))
    B, T = ref.shape
    (rho, shift, dev, voi), (lag, com) = _poisoned(B)
    opt = [t if w else None for t, w in zip((lag, com, shift, dev, voi), want)]
    rc = _lib.load().sa_f0_compare(_f(ref), _f(deg), _f(frames), B, T, Lg, m, _f(rho), *(_f(t) for t in opt),
                                   _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return {"rho": rho.cpu(), "lag": lag.cpu(), "common": com.cpu(), "shift_st": shift.cpu(), "dev_st": dev.cpu(),
            "voicing": voi.cpu()}


def _bits(t):
    return t.view(torch.int32)


CASES = R.gpu_cases()


@pytest.fixture(scope="module", params=range(len(CASES)), ids=lambda i: CASES[i][0])
def case(request):
    """(the case, its restatement, the GPU outputs): computed once per case, left unchanged"""
    c = CASES[request.param]
    return c, R.case_ref(c[0]), _launch(*c[1:])


@gpu
def test_lag_and_common_equal_the_restatement(case):
    (name, *_), want, got = case
    np.testing.assert_array_equal(got["lag"].numpy(), want.lag)
    np.testing.assert_array_equal(got["common"].numpy(), want.common)


@gpu
def test_real_outputs_against_fp64(case):
    (name, *_), want, got = case
    for k in REAL:
        assert bool(torch.isfinite(got[k]).all()), k                               # written over the NaN
        ref = getattr(want, k)
        for b in range(len(ref)):
            bar, err = R.bar(k, ref[b]), abs(float(got[k][b]) - ref[b])
            print(f"{name} row {b}: {k} {float(got[k][b]):.9f} ref {ref[b]:.9f} error {err:.3e} bar {bar:.3e}")
            assert err <= bar, (name, b, k, err, bar)
    for b in range(len(want.rho)):
        if want.common[b] == 0:                                                    # exactly 0, not merely near
            assert all(float(got[k][b]) == 0.0 for k in ("rho", "shift_st", "dev_st"))
            assert int(got["lag"][b]) == 0 and int(got["common"][b]) == 0
    if name in R.TIE_CASES:
        assert float(got["rho"][0]) == 1.0 and int(got["lag"][0]) == R.TIE_CASES[name][0]
        assert float(got["shift_st"][0]) == 0.0 and float(got["dev_st"][0]) == 0.0 and float(got["voicing"][0]) == 1.0


@gpu
def test_two_runs_the_binding_and_null_outputs_give_the_same_bits(case):
    from speech_anonymization_amd import ops
    (name, ref, deg, frames, Lg, m), _, first = case
    again = _launch(ref, deg, frames, Lg, m)
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(again[k])), k
    dev = [torch.as_tensor(v).to(DEV) for v in (ref, deg, frames)]
    bound = ops.f0_compare(*dev, max_lag=Lg, min_common=m)
    assert all(v.is_cuda for v in bound)
    for k, v in zip(("rho", "lag", "common", "shift_st", "dev_st", "voicing"), bound):
        assert torch.equal(_bits(first[k]), _bits(v.cpu())), k
    bare = _launch(ref, deg, frames, Lg, m, want=(False,) * 5)                      # all five may be NULL
    assert torch.equal(_bits(bare["rho"]), _bits(first["rho"]))
    assert bool((bare["lag"] == POISON).all()) and bool((bare["common"] == POISON).all())
    assert all(bool(torch.isnan(bare[k]).all()) for k in ("shift_st", "dev_st", "voicing"))
    some = _launch(ref, deg, frames, Lg, m, want=(True, False, False, True, False))
    assert torch.equal(some["lag"], first["lag"]) and torch.equal(_bits(some["dev_st"]), _bits(first["dev_st"]))
    assert bool((some["common"] == POISON).all()) and bool(torch.isnan(some["voicing"]).all())


@gpu
def test_identical_tracks_score_exactly_one():
    _, ref, _, frames, Lg, m = CASES[0]
    ref = np.nan_to_num(ref, nan=0.0)
    got = _launch(ref, ref, frames, Lg, m)
    want = R.compare(ref, ref, frames, Lg, m)
    assert want.rho.tolist() == [1.0, 1.0, 0.0]
    np.testing.assert_array_equal(got["common"].numpy(), want.common)
    assert got["rho"].tolist() == [1.0, 1.0, 0.0] and got["lag"].tolist() == [0, 0, 0]
    assert got["shift_st"].tolist() == [0.0, 0.0, 0.0] and got["dev_st"].tolist() == [0.0, 0.0, 0.0]
    assert got["voicing"].tolist() == [1.0, 1.0, 0.0]


@gpu
def test_entry_point_and_binding_refuse():
    """only arguments the library rejects before launching: -EINVAL, and the poisoned outputs untouched"""
    from speech_anonymization_amd import _lib, ops, vocoder
    lib, E = _lib.load(), -errno.EINVAL
    assert vocoder.PROSODY_MAX_LAG == lib.sa_f0cmp_dim(1)
    B, T = 2, 61
    ref = torch.full((B, T), 150.0, device=DEV)
    fr = torch.full((B,), T, dtype=torch.int32, device=DEV)
    (rho, shift, dev, voi), (lag, com) = _poisoned(B)

    def call(ref=ref, deg=ref, fr=fr, B=B, T=T, Lg=8, m=8, rho=rho):
        return lib.sa_f0_compare(_f(ref), _f(deg), _f(fr), B, T, Lg, m, _f(rho), _f(lag), _f(com), _f(shift), _f(dev),
                                 _f(voi), _lib.stream())

    for bad in (dict(ref=None), dict(deg=None), dict(fr=None), dict(rho=None), dict(B=0), dict(B=-2), dict(B=65536),
                dict(T=0), dict(T=-1), dict(T=104859), dict(Lg=-1), dict(Lg=33), dict(m=1), dict(m=0), dict(m=-5)):
        assert call(**bad) == E, bad
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (rho, shift, dev, voi))
    assert bool((lag == POISON).all()) and bool((com == POISON).all())
    S = _lib.SaHipError
    with pytest.raises(S, match=r"\[B, T\]"):
        ops.f0_compare(ref[0], ref[0], fr)
    with pytest.raises(S, match="f0_deg: expected shape"):
        ops.f0_compare(ref, ref[:, :30].contiguous(), fr)
    with pytest.raises(S, match="frames: expected torch.int32"):
        ops.f0_compare(ref, ref, fr.long())
    with pytest.raises(S, match="f0_deg: expected torch.float32"):
        ops.f0_compare(ref, ref.double(), fr)
    with pytest.raises(S, match="contiguous"):
        ops.f0_compare(ref.t().contiguous().t(), ref, fr)
    with pytest.raises(S, match="f0_deg: the F0 comparison kernels take GPU tensors"):
        ops.f0_compare(ref, ref.cpu(), fr)
    for kw in (dict(max_lag=33), dict(max_lag=-1), dict(min_common=1)):
        with pytest.raises(S, match="max_lag in 0..32 and min_common >= 2"):
            ops.f0_compare(ref, ref, fr, **kw)


# ---------------------------------------------------------------------------------------------------
# end to end: anonymize.py in fresh child processes
# ---------------------------------------------------------------------------------------------------
ROWS = anon_cli.ROWS
UTT_KEYS = {"f0_corr", "f0_dev_st", "f0_shift_st", "f0_lag_frames", "f0_common_frames", "voicing_agreement"}
SUM_KEYS = {"f0_corr_mean", "f0_dev_st_mean", "voicing_agreement_mean", "prosody_scored"}


@gpu
def test_anonymize_reports_an_identity(tmp_path):
    """--mcadams 1.0 copies every row bit for bit: the two tracks are the same"""
    res, utts = anon_cli.child(tmp_path, "on", ["--mcadams", "1.0", "--report_prosody", "true"])
    assert sorted(utts) == sorted(ROWS)
    for u in utts.values():
        assert UTT_KEYS <= set(u)
        assert u["f0_corr"] == 1.0 and u["f0_lag_frames"] == 0 and u["f0_shift_st"] == 0.0 and u["f0_dev_st"] == 0.0
        assert u["voicing_agreement"] == 1.0 and u["f0_common_frames"] > 100
    assert SUM_KEYS <= set(res)
    assert res["f0_corr_mean"] == 1.0 and res["f0_dev_st_mean"] == 0.0 and res["voicing_agreement_mean"] == 1.0
    assert res["prosody_scored"] == 2
    plain, putts = anon_cli.child(tmp_path, "off", ["--mcadams", "1.0"])
    assert not SUM_KEYS & set(plain) and not any(UTT_KEYS & set(u) for u in putts.values())
    assert sorted(putts) == sorted(utts)


def _contour_child(tmp_path, gamma):
    res, utts = anon_cli.child(tmp_path, "c", ["--pitch_norm", "true", "--phase", "vocoder", "--contour_scale", gamma,
                                               "--report_prosody", "true"])
    want = R.E2E_MEASURED[gamma]
    for i, name in enumerate(ROWS):
        u = utts[name]
        print(f"gamma {gamma} {name}: f0_corr {u['f0_corr']!r} (fp64 path {want['rho'][i]!r}, margin "
              f"{R.E2E_MARGIN['rho']:.3e}), f0_dev_st {u['f0_dev_st']!r} (fp64 path {want['dev_st'][i]!r}, distance "
              f"{abs(u['f0_dev_st'] - want['dev_st'][i]):.3e}, margin {R.E2E_MARGIN['dev_st']:.3e}), lag "
              f"{u['f0_lag_frames']}, common {u['f0_common_frames']}, voicing {u['voicing_agreement']!r}")
    return utts, want


@gpu
def test_anonymize_reports_a_kept_contour(tmp_path):
    """--contour_scale 1: the correlation at least the fp64 path's less the margin, the deviation within the margin;
    the lag is not asserted (on a linear glide every lag is nearly perfect)"""
    utts, want = _contour_child(tmp_path, "1")
    for i, name in enumerate(ROWS):
        assert utts[name]["f0_corr"] >= want["rho"][i] - R.E2E_MARGIN["rho"], name
        assert abs(utts[name]["f0_dev_st"] - want["dev_st"][i]) <= R.E2E_MARGIN["dev_st"], name


@gpu
def test_anonymize_reports_a_flattened_contour(tmp_path):
    """--contour_scale 0: the deviation within the margin of the fp64 path's; the correlation of a monotone track is
    the tracker's jitter and is printed only"""
    utts, want = _contour_child(tmp_path, "0")
    for i, name in enumerate(ROWS):
        assert abs(utts[name]["f0_dev_st"] - want["dev_st"][i]) <= R.E2E_MARGIN["dev_st"], name
