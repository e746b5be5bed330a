"""GPU checks of the formant report (csrc/sa_formants.hip, ops.formant_tracks, ops.formant_compare,
metrics.formant_shift, --report_formants) against the fp64 restatement tests/lpcformant_ref.py, which takes its roots
from numpy.roots and its medians from a sort, not by the kernels' methods.

The bar of the tracks, per frequency and bandwidth:   |value - ref| <= 2^-24 |ref| + 16 x D

  2^-24 |ref|   the fp32 rounding of the value that is returned
  D             tools/formant_report_delta.py re-evaluates the restatement on these same cases with its own fp64 Aberth
                iteration and with the lag sums from the far end: the worst |delta| is 1.96e-11 Hz for a frequency and
                5.13e-11 Hz for a bandwidth (tests/test_formant_report_cpu.py holds lpcformant_ref.SPREAD_HZ to the
                tool's output); the factor 16 covers the kernel's summation order and its atan2 and log

Every status is compared: tests/test_formant_report_cpu.py checks that no frame of the cases is near a decision.
The comparison's medians and counts are exact; its ratios and shift are within one fp32 ulp.  The end-to-end bars are
twice the restatement's own distance from theory, recorded by the same tool.

Measured on an MI355X: the worst error over bar of the tracks is 0.98 (the "odd" case; 0.52, 0.80 and 0.92 for the
other three with a scored frame) -- the fp32 rounding of the returned value itself, which may take all of 2^-24 |ref|;
the ratios and the shift of the comparison came out 0 ulp off the restatement's at every T."""
import ctypes
import errno

import numpy as np
import pytest
import torch

from tests import anon_cli
from tests import lpcformant_ref as R

DEV = "cuda:0"
POISON = -7
gpu = pytest.mark.gpu


def _f(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(*arrays):
    return [torch.as_tensor(np.asarray(v)).to(DEV).contiguous() for v in arrays]


def _tracks(wav, nv, want_bw=True, want_status=True):
    """sa_formant_tracks through the library itself, into outputs poisoned with NaN and -7 -> a dict of CPU tensors"""
    from speech_anonymization_amd import _lib
    wav, nv = _dev(wav, nv)
    B, N = wav.shape
    T = N // 160 + 1
    freq, bw = (torch.full((B, T, 3), float("nan"), device=DEV) for _ in range(2))
    status = torch.full((B, T), POISON, dtype=torch.int32, device=DEV)
    rc = _lib.load().sa_formant_tracks(_f(wav), _f(nv), B, N, _f(freq), _f(bw if want_bw else None),
                                       _f(status if want_status else None), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return {"freq": freq.cpu(), "bw": bw.cpu(), "status": status.cpu()}


def _compare(F_ref, F_deg, st_ref, st_deg, f0_ref, f0_deg, frames, m=R.MIN_COMMON, want=(True, True, True)):
    """sa_formant_compare through the library itself, into poisoned outputs; want: which of med, ratio, common get a
    pointer"""
    from speech_anonymization_amd import _lib
    args = _dev(F_ref, F_deg, st_ref, st_deg, f0_ref, f0_deg, frames)
    B, T, _ = args[0].shape
    med, ratio = (torch.full((B, 3), float("nan"), device=DEV) for _ in range(2))
    shift = torch.full((B,), float("nan"), device=DEV)
    common = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    opt = [t if w else None for t, w in zip((med, ratio, common), want)]
    rc = _lib.load().sa_formant_compare(*(_f(t) for t in args), B, T, m, _f(opt[0]), _f(opt[1]), _f(shift), _f(opt[2]),
                                        _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return {"med": med.cpu(), "ratio": ratio.cpu(), "shift": shift.cpu(), "common": common.cpu()}


# ---------------------------------------------------------------------------------------------------
# tracks
# ---------------------------------------------------------------------------------------------------
CASES = R.gpu_cases()


@pytest.fixture(scope="module", params=range(len(CASES)), ids=lambda i: CASES[i][0])
def case(request):
    """(the case, its restatement, the GPU outputs): computed once per case, left unchanged"""
    c = CASES[request.param]
    return c, R.case_ref(c[0]), _tracks(*c[1:])


@gpu
def test_every_status_equals_the_restatement(case):
    (name, *_), want, got = case
    np.testing.assert_array_equal(got["status"].numpy(), want.status)


@gpu
def test_frequencies_and_bandwidths_against_fp64(case):
    (name, *_), want, got = case
    worst = 0.0
    for kind, key, ref in (("f", "freq", want.freq), ("b", "bw", want.bw)):
        val = got[key].double().numpy()
        assert np.isfinite(val).all(), key                                     # written over the NaN
        assert (val[want.status != R.OK] == 0.0).all(), key                    # exactly 0, not merely near
        for b, t, k in zip(*np.nonzero(ref)):
            err, bar = abs(val[b, t, k] - ref[b, t, k]), R.bar(kind, ref[b, t, k])
            worst = max(worst, err / bar)
            assert err <= bar, (name, key, b, t, k, val[b, t, k], ref[b, t, k], err, bar)
    print(f"{name}: worst error over bar {worst:.3f} over {int((want.status == R.OK).sum())} scored frames")


@gpu
def test_tracks_twice_the_binding_and_null_outputs_give_the_same_bits(case):
    from speech_anonymization_amd import ops
    (name, wav, nv), _, first = case
    again = _tracks(wav, nv)
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(again[k])), k
    freq, status, bw = ops.formant_tracks(*_dev(wav, nv), return_bw=True)
    assert freq.is_cuda and status.is_cuda and bw.is_cuda
    for k, v in (("freq", freq), ("status", status), ("bw", bw)):
        assert torch.equal(_bits(first[k]), _bits(v.cpu())), k
    assert len(ops.formant_tracks(*_dev(wav, nv))) == 2
    bare = _tracks(wav, nv, want_bw=False, want_status=False)                   # both may be NULL
    assert torch.equal(_bits(bare["freq"]), _bits(first["freq"]))
    assert bool(torch.isnan(bare["bw"]).all()) and bool((bare["status"] == POISON).all())


@gpu
def test_a_row_does_not_depend_on_its_batch():
    name, wav, nv = CASES[0]
    whole = _tracks(wav, nv)
    alone = _tracks(wav[1:2], nv[1:2])
    for k in whole:
        assert torch.equal(_bits(whole[k][1:2]), _bits(alone[k])), k


# ---------------------------------------------------------------------------------------------------
# comparison, on given tracks
# ---------------------------------------------------------------------------------------------------
COMPARE_T = (1, 7, 8, 9, 300, 5000)


@pytest.fixture(scope="module", params=COMPARE_T, ids=lambda T: f"T{T}")
def given(request):
    c = R.compare_case(request.param)
    return c, R.compare(*c), _compare(*c)


def _ulps(got, ref):
    return abs(float(got) - float(ref)) / R.ulp32(ref) if ref != 0.0 else (0.0 if float(got) == 0.0 else np.inf)


@gpu
def test_medians_and_counts_equal_the_restatement(given):
    c, want, got = given
    T = c[0].shape[1]
    print(f"T {T}: common {got['common'].tolist()} ratios {got['ratio'].tolist()} shift {got['shift'].tolist()}")
    np.testing.assert_array_equal(got["common"].numpy(), want.common)
    assert torch.equal(_bits(got["med"]), _bits(torch.from_numpy(want.med)))
    assert want.common[3] == 0 and got["shift"][3] == 0.0                      # the row without a common frame
    if T >= 300:
        assert (want.common[:3] >= R.MIN_COMMON).all() and want.common[1] < want.common[0] == T


@gpu
def test_ratios_and_shift_within_one_ulp(given):
    c, want, got = given
    for b in range(len(want.shift)):
        u = [_ulps(got["ratio"][b, k], want.ratio[b, k]) for k in range(3)] + [_ulps(got["shift"][b], want.shift[b])]
        print(f"T {c[0].shape[1]} row {b}: ulps off {u}")
        assert max(u) <= 1.0, (b, u)
        if want.common[b] == 0:
            assert not got["ratio"][b].any() and not got["med"][b].any() and got["shift"][b] == 0.0


@gpu
def test_compare_twice_the_binding_and_null_outputs_give_the_same_bits(given):
    from speech_anonymization_amd import ops
    c, _, first = given
    again = _compare(*c)
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(again[k])), k
    cols = ops.formant_compare(*_dev(*c))
    assert len(cols) == 8 and all(v.is_cuda and v.shape == (4,) for v in cols)
    for k in range(3):
        assert torch.equal(_bits(first["med"][:, k]), _bits(cols[k].cpu()))
        assert torch.equal(_bits(first["ratio"][:, k]), _bits(cols[3 + k].cpu()))
    assert torch.equal(_bits(first["shift"]), _bits(cols[6].cpu())) and torch.equal(first["common"], cols[7].cpu())
    bare = _compare(*c, want=(False, False, False))                             # all but shift may be NULL
    assert torch.equal(_bits(bare["shift"]), _bits(first["shift"]))
    assert bool(torch.isnan(bare["med"]).all()) and bool(torch.isnan(bare["ratio"]).all())
    assert bool((bare["common"] == POISON).all())
    some = _compare(*c, want=(False, True, False))
    assert torch.equal(_bits(some["ratio"]), _bits(first["ratio"])) and bool(torch.isnan(some["med"]).all())


@gpu
def test_identical_tracks_and_min_common_on_the_gpu():
    F_ref, _, st_ref, _, f0_ref, _, frames = R.compare_case(300)
    got = _compare(F_ref, F_ref, st_ref, st_ref, f0_ref, f0_ref, frames)
    want = R.compare(F_ref, F_ref, st_ref, st_ref, f0_ref, f0_ref, frames)
    np.testing.assert_array_equal(got["common"].numpy(), want.common)
    assert (want.common > 100).all()
    assert bool((got["ratio"] == 1.0).all()) and bool((got["shift"] == 1.0).all())
    assert torch.equal(_bits(got["med"]), _bits(torch.from_numpy(want.med)))
    n = int(want.common[1])
    at = _compare(F_ref, F_ref, st_ref, st_ref, f0_ref, f0_ref, frames, m=n)
    above = _compare(F_ref, F_ref, st_ref, st_ref, f0_ref, f0_ref, frames, m=n + 1)
    assert at["common"][1] == n and at["shift"][1] == 1.0
    assert above["common"][1] == 0 and above["shift"][1] == 0.0 and not above["med"][1].any()


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
@gpu
def test_tracks_entry_point_and_binding_refuse():
    """only arguments the library rejects before launching: -EINVAL, and the poisoned outputs untouched"""
    from speech_anonymization_amd import _lib, ops
    lib, E = _lib.load(), -errno.EINVAL
    B, N = 2, 800
    wav = torch.zeros(B, N, device=DEV)
    nv = torch.full((B,), N, dtype=torch.int32, device=DEV)
    freq, bw = (torch.full((B, 6, 3), float("nan"), device=DEV) for _ in range(2))
    status = torch.full((B, 6), POISON, dtype=torch.int32, device=DEV)

    def call(wav=wav, nv=nv, B=B, N=N, freq=freq):
        return lib.sa_formant_tracks(_f(wav), _f(nv), B, N, _f(freq), _f(bw), _f(status), _lib.stream())

    for bad in (dict(wav=None), dict(nv=None), dict(freq=None), dict(B=0), dict(B=-1), dict(B=65536), dict(N=0),
                dict(N=-5), dict(N=(1 << 24) + 1)):
        assert call(**bad) == E, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(freq).all()) and bool(torch.isnan(bw).all()) and bool((status == POISON).all())
    S = _lib.SaHipError
    with pytest.raises(S, match=r"wav: expected \[B, N\]"):
        ops.formant_tracks(wav[0], nv)
    with pytest.raises(S, match="wav: expected torch.float32"):
        ops.formant_tracks(wav.double(), nv)
    with pytest.raises(S, match="wav: expected a contiguous"):
        ops.formant_tracks(wav.t().contiguous().t(), nv)
    with pytest.raises(S, match="n_valid: expected torch.int32"):
        ops.formant_tracks(wav, nv.long())
    with pytest.raises(S, match="n_valid: expected shape"):
        ops.formant_tracks(wav, nv[:1])
    with pytest.raises(S, match="n_valid: the formant kernels take GPU tensors"):
        ops.formant_tracks(wav, nv.cpu())


@gpu
def test_compare_entry_point_and_binding_refuse():
    from speech_anonymization_amd import _lib, ops
    lib, E = _lib.load(), -errno.EINVAL
    assert lib.sa_formant_dim(6) == ops.FORMANT_MAX_T
    B, T = 2, 20
    F = torch.full((B, T, 3), 500.0, device=DEV)
    st = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    f0 = torch.full((B, T), 120.0, device=DEV)
    fr = torch.full((B,), T, dtype=torch.int32, device=DEV)
    med, ratio = (torch.full((B, 3), float("nan"), device=DEV) for _ in range(2))
    shift = torch.full((B,), float("nan"), device=DEV)
    common = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    names = ("Fr", "Fd", "sr", "sd", "pr", "pd", "fr")

    def call(B=B, T=T, m=8, shift=shift, **kw):
        ptrs = dict(zip(names, (F, F, st, st, f0, f0, fr)), **kw)
        return lib.sa_formant_compare(*(_f(ptrs[k]) for k in names), B, T, m, _f(med), _f(ratio), _f(shift),
                                      _f(common), _lib.stream())

    for bad in [{k: None} for k in names] + [dict(shift=None), dict(B=0), dict(B=-2), dict(B=65536), dict(T=0),
                                             dict(T=-1), dict(T=104859), dict(m=0), dict(m=-3)]:
        assert call(**bad) == E, bad
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (med, ratio, shift)) and bool((common == POISON).all())
    S = _lib.SaHipError
    with pytest.raises(S, match=r"F_ref: expected \[B, T, 3\]"):
        ops.formant_compare(F[0], F[0], st, st, f0, f0, fr)
    with pytest.raises(S, match=r"F_ref: expected \[B, T, 3\]"):
        ops.formant_compare(F[:, :, :2].contiguous(), F, st, st, f0, f0, fr)
    with pytest.raises(S, match="F_deg: expected shape"):
        ops.formant_compare(F, F[:, :10].contiguous(), st, st, f0, f0, fr)
    with pytest.raises(S, match="st_deg: expected torch.int32"):
        ops.formant_compare(F, F, st, st.long(), f0, f0, fr)
    with pytest.raises(S, match="f0_deg: expected torch.float32"):
        ops.formant_compare(F, F, st, st, f0, f0.double(), fr)
    with pytest.raises(S, match="f0_ref: expected a contiguous"):
        ops.formant_compare(F, F, st, st, f0.t().contiguous().t(), f0, fr)
    with pytest.raises(S, match="frames: the formant kernels take GPU tensors"):
        ops.formant_compare(F, F, st, st, f0, f0, fr.cpu())
    for m in (0, -1, True, 2.5):
        with pytest.raises(S, match="min_common, a count of frames, 1 or more"):
            ops.formant_compare(F, F, st, st, f0, f0, fr, min_common=m)


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def _shift_of(anonymiser):
    """the report of metrics.formant_shift on the three voiced rows against anonymiser(rows), every frame counted as
    voiced as in the recorded figures (lpcformant_ref.known_f0) -> (ratios [3 rows][3], shift [3], common [3])"""
    from speech_anonymization_amd import metrics
    rows = torch.from_numpy(R.e2e_rows()).to(DEV)
    B, N = rows.shape
    T = N // 160 + 1
    out = anonymiser(rows, torch.ones(B))
    assert out.shape == rows.shape and out.dtype == torch.float32
    f0 = torch.from_numpy(R.known_f0(T)).to(DEV)
    nv = torch.full((B,), N, dtype=torch.int32, device=DEV)
    cols = metrics.formant_shift(rows, out.contiguous(), nv, f0, f0, torch.full((B,), T, dtype=torch.int32, device=DEV))
    cols = [c.cpu() for c in cols]
    return torch.stack(cols[3:6], 1).double().numpy(), cols[6].tolist(), cols[7].tolist()


@gpu
@pytest.mark.parametrize("alpha", [0.8, 0.6])
def test_mcadams_moves_each_formant_by_its_own_ratio(alpha):
    """each per-formant ratio within twice the restatement's recorded distance from phi^alpha / phi"""
    from speech_anonymization_amd import mcadams
    from tests import mcadams_ref as M
    ratio, shift, common = _shift_of(mcadams.McAdams(alpha=alpha))
    theory = [M.expected_peak(F, alpha) / F for F, _ in R.FORMANTS]
    recorded = R.recorded()["e2e"]["mcadams"][str(alpha)]
    for b in range(3):
        d = [abs(ratio[b, k] / theory[k] - 1.0) for k in range(3)]
        print(f"alpha {alpha} row {b}: ratios {ratio[b].tolist()} (restatement {recorded['ratio'][b]}) theory {theory} "
              f"distance {d} bars {[2.0 * v for v in R.E2E_MCADAMS[alpha]]} shift {shift[b]} common {common[b]}")
    assert min(common) >= 28
    for b in range(3):
        for k in range(3):
            assert abs(ratio[b, k] / theory[k] - 1.0) <= 2.0 * R.E2E_MCADAMS[alpha][k], (b, k)
    assert ratio[:, 0].min() > ratio[:, 1].max() > ratio[:, 1].min() > ratio[:, 2].max()     # F1 moves most, F3 least


@gpu
def test_formant_shifter_moves_the_formants():
    """FormantShifter(1.15): each per-formant ratio within twice the restatement's recorded distance from 1.15.  The
    restatement itself is far from 1.15 (the cepstral warp moves a 30-coefficient envelope, the
    LPC poles follow it only in part, and F3 of two rows jumps to another pole), so the bars are wide by measurement,
    not by choice"""
    from speech_anonymization_amd import pitchnorm
    ratio, shift, common = _shift_of(pitchnorm.FormantShifter(1.15))
    recorded = R.recorded()["e2e"]["shift"]["1.15"]
    for b in range(3):
        d = [abs(ratio[b, k] / 1.15 - 1.0) for k in range(3)]
        print(f"formant ratio 1.15 row {b}: ratios {ratio[b].tolist()} (restatement {recorded['ratio'][b]}) distance "
              f"{d} bars {[2.0 * v for v in R.E2E_SHIFT[1.15]]} shift {shift[b]} common {common[b]}")
    assert min(common) >= R.MIN_COMMON
    for b in range(3):
        for k in range(3):
            assert abs(ratio[b, k] / 1.15 - 1.0) <= 2.0 * R.E2E_SHIFT[1.15][k], (b, k)


UTT_KEYS = {"f1_hz", "f2_hz", "f3_hz", "f1_shift", "f2_shift", "f3_shift", "formant_shift", "formant_frames"}
SUM_KEYS = {"formant_shift_mean", "f1_shift_mean", "f2_shift_mean", "f3_shift_mean", "formants_scored"}


@gpu
def test_anonymize_reports_an_identity_on_the_synthetic_rows(tmp_path):
    """--mcadams 1.0 copies every row bit for bit: every scored utterance has ratios of exactly 1.
    The synthetic rows are bare harmonic series: what is checked here is the plumbing, not a formant"""
    res = anon_cli.run_child(["--device", DEV, "--synthetic", "4", "--out_dir", str(tmp_path / "on"), "--mcadams",
                              "1.0", "--report_formants", "true"])
    assert len(res["utterances"]) == 4 and SUM_KEYS <= set(res)
    scored = 0
    for u in res["utterances"]:
        assert UTT_KEYS <= set(u) and isinstance(u["formant_frames"], int)
        print(u["id"], {k: u[k] for k in sorted(UTT_KEYS)})
        if u["formant_frames"]:
            scored += 1
            assert u["f1_shift"] == u["f2_shift"] == u["f3_shift"] == u["formant_shift"] == 1.0
            assert 90.0 <= u["f1_hz"] < u["f2_hz"] < u["f3_hz"] <= 5500.0 and u["formant_frames"] >= R.MIN_COMMON
        else:
            assert all(u[k] is None for k in UTT_KEYS - {"formant_frames"})
    assert res["formants_scored"] == scored
    if scored:
        assert all(res[k] == 1.0 for k in SUM_KEYS - {"formants_scored"})
    else:
        assert all(res[k] is None for k in SUM_KEYS - {"formants_scored"})
    keys = list(res)
    assert keys[-5:] == ["formant_shift_mean", "f1_shift_mean", "f2_shift_mean", "f3_shift_mean", "formants_scored"]


@gpu
def test_prosody_and_formants_together_print_what_each_prints_alone(tmp_path, capsys):
    """the F0 tracks are taken once per batch when both reports are on, and every key keeps its bits"""
    from speech_anonymization_amd import pitchnorm
    from tests import contour_ref as Cr
    csv = anon_cli.manifest(tmp_path, anon_cli.ROWS, [row[:n] for row, n in zip(Cr.case_rows(), (16037, 12000))])
    calls, real = [], pitchnorm.f0_track

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    def run(name, flags):
        argv = ["--device", DEV, "--csv", csv, "--out_dir", str(tmp_path / name), "--mcadams", "0.8"]
        for flag in flags:
            argv += [f"--{flag}", "true"]
        return anon_cli.run(capsys, argv)

    pitchnorm.f0_track = counted
    try:
        both = run("both", ("report_prosody", "report_formants"))
        n_both = len(calls)
        alone = {flag: run(flag, (flag,)) for flag in ("report_prosody", "report_formants")}
    finally:
        pitchnorm.f0_track = real
    assert n_both == 2 and len(calls) == 6                                      # one batch: ref and deg, once
    for i, u in enumerate(both["utterances"]):
        merged = dict(alone["report_prosody"]["utterances"][i], **alone["report_formants"]["utterances"][i])
        assert u == merged and list(u) == list(merged), u["id"]
        assert UTT_KEYS <= set(u) and u["formant_frames"] > 0
    merged = dict(alone["report_prosody"], **alone["report_formants"])
    assert {k: v for k, v in both.items() if k not in ("out_dir", "utterances")} == \
        {k: v for k, v in merged.items() if k not in ("out_dir", "utterances")}
