"""GPU checks of the STOI / ESTOI scorer (csrc/sa_stoi.hip, ops.stoi) against the fp64
restatement tests/stoi_ref.py, which transforms with numpy.fft, not with the kernel's direct sum.

The bar, per score:   |score - ref| <= 16 x D + 2^-24 |ref|

  D             tools/stoi_delta.py re-evaluates the restatement on these same cases with the resampled signals
                rounded to fp32, with the band magnitudes rounded to fp32, with the DFT as a direct sum in reverse
                order and with the frame energies summed from the far end: the worst |delta| is 1.28e-8 for STOI
                and 9.03e-8 for ESTOI (tests/test_stoi_cpu.py holds stoi_ref.DELTA_MEASURED to the tool's output)
  2^-24 |ref|   the fp32 rounding of the score that is returned

16 x D + 2^-24 is 2.6e-7 and 1.5e-6 at a score of 1, under the 1e-4 the scores are read to.  frames and segments are
exact: tests/test_stoi_cpu.py checks that no frame energy of these rows lies within 1 +- 1e-6 of its threshold."""
import ctypes
import errno
import os

import numpy as np
import pytest
import torch

from tests import anon_cli
from tests import stoi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
POISON = -7
gpu = pytest.mark.gpu


def _f(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _launch(ref, deg, n_valid, want=(True, True, True)):
    """sa_stoi through the library itself, into outputs and a workspace poisoned with NaN ->
    (stoi, estoi, frames, segments) on the CPU"""
    from speech_anonymization_amd import _lib, ops
    ref, deg, n_valid = (torch.as_tensor(np.asarray(v)).to(DEV).contiguous() for v in (ref, deg, n_valid))
    B, N = ref.shape
    st = torch.full((B,), float("nan"), device=DEV)
    es = torch.full((B,), float("nan"), device=DEV)
    fr = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    sg = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    ws = ops.stoi_workspace(B, N, DEV).fill_(float("nan"))
    rc = _lib.load().sa_stoi(_f(ref), _f(deg), _f(n_valid), B, N, _f(ops.stoi_taps(DEV)), _f(st),
                             _f(es if want[0] else None), _f(fr if want[1] else None), _f(sg if want[2] else None),
                             _f(ws), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return st.cpu(), es.cpu(), fr.cpu(), sg.cpu()


def _within(name, got, ref, measure):
    for b in range(len(ref)):
        bar, err = R.bar(measure, ref[b]), abs(float(got[b]) - ref[b])
        print(f"{name} row {b}: {measure} {float(got[b]):.9f} ref {ref[b]:.9f} error {err:.3e} bar {bar:.3e}")
        assert err <= bar, (name, b, measure, err, bar)


CASES = R.gpu_cases()


@pytest.fixture(scope="module", params=range(len(CASES)), ids=lambda i: CASES[i][0])
def case(request):
    """(name, ref, deg, n_valid, restatement, GPU outputs): computed once per case, left unchanged"""
    name, ref, deg, nv, _ = CASES[request.param]
    return name, ref, deg, nv, R.case_ref(name), _launch(ref, deg, nv)


@gpu
def test_frames_and_segments_equal_the_restatement(case):
    name, _, _, _, want, (st, es, fr, sg) = case
    np.testing.assert_array_equal(fr.numpy(), want.frames)
    np.testing.assert_array_equal(sg.numpy(), want.segments)


@gpu
def test_scores_against_fp64(case):
    name, _, _, _, want, (st, es, fr, sg) = case
    assert bool(torch.isfinite(st).all()) and bool(torch.isfinite(es).all())       # written over the NaN
    _within(name, st, want.stoi, "stoi")
    _within(name, es, want.estoi, "estoi")
    for b in range(len(want.stoi)):
        if want.segments[b] == 0:                                                  # exactly 0, not merely near
            assert float(st[b]) == 0.0 and float(es[b]) == 0.0 and int(sg[b]) == 0


@gpu
def test_two_runs_the_binding_and_null_outputs_give_the_same_bits(case):
    from speech_anonymization_amd import ops
    name, ref, deg, nv, _, first = case
    for a, b in zip(first, _launch(ref, deg, nv)):
        assert torch.equal(a, b)
    dev = [torch.as_tensor(v).to(DEV) for v in (ref, deg, nv)]
    bound = ops.stoi(*dev)
    assert all(v.is_cuda for v in bound)
    for a, b in zip(first, bound):
        assert torch.equal(a.view(torch.int32), b.cpu().view(torch.int32))
    st, es, fr, sg = ops.stoi(*dev, extended=False)
    assert es is None and torch.equal(st.cpu().view(torch.int32), first[0].view(torch.int32))
    st, es, fr, sg = _launch(ref, deg, nv, want=(False, False, False))             # all three may be NULL
    assert torch.equal(st.view(torch.int32), first[0].view(torch.int32))
    assert bool(torch.isnan(es).all()) and bool((fr == POISON).all()) and bool((sg == POISON).all())
    st, es, fr, sg = _launch(ref, deg, nv, want=(False, True, True))
    assert torch.equal(fr, first[2]) and torch.equal(sg, first[3])


@gpu
def test_identical_inputs_score_one():
    _, ref, _, nv, _ = CASES[0]
    want = R.stoi(ref, ref, nv)
    st, es, fr, sg = _launch(ref, ref, nv)
    assert (want.stoi >= 1.0 - 1e-9).all() and (want.estoi >= 1.0 - 1e-9).all()
    _within("identical", st, np.ones(3), "stoi")
    _within("identical", es, np.ones(3), "estoi")
    np.testing.assert_array_equal(sg.numpy(), want.segments)


@gpu
@pytest.mark.parametrize("N", [1, 408, 409, 615])
def test_rows_too_short_for_a_segment(N):
    """N = 408 resamples to 255 samples (no frame), 409 to 256 (one frame), 615 to 385 (two); the workspace then holds
    a single frame slot"""
    x = R.harmonic_row(N, 5)[None].astype(np.float32)
    want = R.stoi(x, x, [N])
    st, es, fr, sg = _launch(x, x, np.array([N], np.int32))
    assert want.frames[0] == {1: 0, 408: 0, 409: 1, 615: 2}[N] and int(fr[0]) == want.frames[0]
    assert int(sg[0]) == 0 and float(st[0]) == 0.0 and float(es[0]) == 0.0


@gpu
def test_entry_point_and_binding_refuse():
    """only arguments the library rejects before launching: -EINVAL, and the poisoned outputs untouched"""
    from speech_anonymization_amd import _lib, ops
    lib, E = _lib.load(), -errno.EINVAL
    B, N = 2, 8000
    ref = torch.zeros(B, N, device=DEV)
    nv = torch.full((B,), N, dtype=torch.int32, device=DEV)
    taps = ops.stoi_taps(DEV)
    st = torch.full((B,), float("nan"), device=DEV)
    es = torch.full((B,), float("nan"), device=DEV)
    fr = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    sg = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    ws = ops.stoi_workspace(B, N, DEV).fill_(float("nan"))

    def call(ref=ref, deg=ref, nv=nv, B=B, N=N, taps=taps, st=st, ws=ws):
        return lib.sa_stoi(_f(ref), _f(deg), _f(nv), B, N, _f(taps), _f(st), _f(es), _f(fr), _f(sg), _f(ws),
                           _lib.stream())

    for bad in (dict(ref=None), dict(deg=None), dict(nv=None), dict(taps=None), dict(st=None), dict(ws=None),
                dict(B=0), dict(B=-2), dict(B=65536), dict(N=0), dict(N=-1), dict(N=(1 << 24) + 1)):
        assert call(**bad) == E, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(st).all()) and bool(torch.isnan(es).all()) and bool(torch.isnan(ws).all())
    assert bool((fr == POISON).all()) and bool((sg == POISON).all())
    S = _lib.SaHipError
    with pytest.raises(S, match=r"\[B, N\]"):
        ops.stoi(ref[0], ref[0], nv)
    with pytest.raises(S, match="deg: expected shape"):
        ops.stoi(ref, ref[:, :100].contiguous(), nv)
    with pytest.raises(S, match="n_valid: expected torch.int32"):
        ops.stoi(ref, ref, nv.long())
    with pytest.raises(S, match="deg: expected torch.float32"):
        ops.stoi(ref, ref.double(), nv)
    with pytest.raises(S, match="contiguous"):
        ops.stoi(ref.t().contiguous().t(), ref, nv)
    with pytest.raises(S, match="deg: the STOI kernels take GPU tensors"):
        ops.stoi(ref, ref.cpu(), nv)


@gpu
def test_anonymize_reports_stoi(tmp_path):
    """one fresh child process: --mcadams 1.0 copies every row bit for bit, so every scored
    utterance reports 1 within the bar; the same command without the flag prints none of the new keys"""
    def run(extra):
        return anon_cli.run_child(["--device", DEV, "--synthetic", "4", "--mcadams", "1.0", "--out_dir",
                                   str(tmp_path / ("a" + str(len(extra))))] + extra)

    res = run(["--report_stoi", "true"])
    assert len(res["utterances"]) == 4
    scored = [u for u in res["utterances"] if u["stoi_segments"] > 0]
    assert len(scored) >= 1
    for u in res["utterances"]:
        assert {"stoi", "estoi", "stoi_segments"} <= set(u)
        if u["stoi_segments"] > 0:
            assert abs(u["stoi"] - 1.0) <= R.bar("stoi", 1.0) and abs(u["estoi"] - 1.0) <= R.bar("estoi", 1.0)
        else:
            assert u["stoi"] is None and u["estoi"] is None
    assert abs(res["stoi_mean"] - 1.0) <= R.bar("stoi", 1.0) and abs(res["estoi_mean"] - 1.0) <= R.bar("estoi", 1.0)
    plain = run([])
    assert not {"stoi_mean", "estoi_mean"} & set(plain)
    assert not any({"stoi", "estoi", "stoi_segments"} & set(u) for u in plain["utterances"])
    assert [u["id"] for u in plain["utterances"]] == [u["id"] for u in res["utterances"]]
