"""GPU checks of the LPC formant normalisation (csrc/sa_formant_norm.hip, ops.pole_warp,
ops.formant_centre, formantnorm.FormantNormalizer, --formant_norm) against the fp64 restatement
tests/formantnorm_ref.py, which takes its roots from numpy.roots and its medians from a sort, not by the kernels'
methods.

The per-sample bar of sa_pole_warp is sa_mcadams's (tests/test_mcadams_gpu.py; u = 2^-24; F_a, F_b the two frames'
values at a sample, g the gain, all from the restatement):

    |out - ref| <= g u (|F_a| + |F_b| + 2 |F_a + F_b|) + u |ref| + u |ref| K + C max|ref_row|

  g u |F_a|, g u |F_b|      the two stored frames' roundings to fp32
  2 g u |F_a + F_b|         their fp32 sum's rounding and the fp32 rounding of g y
  u |ref|                   (kept apart, as there)
  u |ref| K                 the gain's own relative error K u, derived by mcadams_ref.gain_bar from the same roundings
                            (Cauchy-Schwarz on the sum of squares); the gain itself is held to K u
  C max|ref_row|            C = 16 x 1.36e-10: tools/formant_norm_delta.py re-runs the restatement on these same cases
                            with its own fp64 Aberth and with the lag sums from the far end and finds 1.35e-10 of the
                            row's peak between equally valid fp64 evaluations (tests/test_formant_norm_cpu.py holds
                            formantnorm_ref.C_MEASURED to the tool's output); the factor 16 covers the kernel's
                            summation orders and its atan2 and cos.  Never measured on the kernel.

Left out: samples touched by a frame the restatement flags as near a decision, at most 1 % (none on these cases:
tests/test_formant_norm_cpu.py checks that).  sa_formant_centre's medians and counts are exact, its q within one fp32
ulp.  The end-to-end bars are twice the restatement's own distances, recorded by the same tool.

Measured on an MI355X: the worst error over bar of sa_pole_warp is 0.50 (0.20 to 0.50 over the cases), the worst gain
error 0.56 u against bars of 3.06 to 3.15 u; sa_formant_centre's q came out 0 ulp off the restatement's at every T; the
open-loop ratios and the closed-loop distances agree with the restatement's to six digits."""
import ctypes
import errno
import math
import os

import numpy as np
import pytest
import torch

from tests import anon_cli
from tests import formantnorm_ref as R
from tests import lpcformant_ref as LF
from tests import mcadams_ref as M

DEV = "cuda:0"
U = R.U
C = R.C_FACTOR * R.C_MEASURED
POISON = -7
gpu = pytest.mark.gpu


def _f(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(*arrays):
    return [torch.as_tensor(np.asarray(v)).to(DEV).contiguous() for v in arrays]


def _warp(wav, q, n_valid, level, want_status=True, want_gain=True):
    """sa_pole_warp through the library itself, into buffers poisoned with NaN and -7 -> (out, status, gain), CPU"""
    from speech_anonymization_amd import _lib, ops
    wd, qd, nd = _dev(wav, q, n_valid)
    B, N = wd.shape
    T = M.n_frames(N)
    out = torch.full_like(wd, float("nan"))
    ws = ops.pole_warp_workspace(B, N, DEV).fill_(float("nan"))
    status = torch.full((B, T), POISON, dtype=torch.int32, device=DEV)
    gain = torch.full((B,), float("nan"), device=DEV)
    rc = _lib.load().sa_pole_warp(_f(wd), _f(qd), _f(nd), B, N, int(level), _f(out), _f(ws),
                                  _f(status if want_status else None), _f(gain if want_gain else None), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu(), status.cpu(), gain.cpu()


def _centre(freq, status, f0, frames, target=R.TARGET_DEFAULT, q_min=0.8, q_max=1.2, m=R.MIN_FRAMES,
            want=(True, True)):
    """sa_formant_centre through the library itself, into poisoned outputs; want: which of med, count get a pointer"""
    from speech_anonymization_amd import _lib
    fd, sd, fr = _dev(freq, status, frames)
    pd = None if f0 is None else _dev(f0)[0]
    B, T, _ = fd.shape
    med = torch.full((B, 3), float("nan"), device=DEV)
    q = torch.full((B,), float("nan"), device=DEV)
    count = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    cf = ctypes.c_float
    rc = _lib.load().sa_formant_centre(_f(fd), _f(sd), _f(pd), _f(fr), B, T, cf(target[0]), cf(target[1]),
                                       cf(target[2]), cf(q_min), cf(q_max), m, _f(med if want[0] else None), _f(q),
                                       _f(count if want[1] else None), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return {"med": med.cpu(), "q": q.cpu(), "count": count.cpu()}


# ---------------------------------------------------------------------------------------------------
# sa_pole_warp
# ---------------------------------------------------------------------------------------------------
CASES = R.gpu_cases()


@pytest.fixture(scope="module", params=[(c, lv) for c in range(len(CASES)) for lv in (True, False)],
                ids=lambda p: "%s_level%d" % (CASES[p[0]][0], p[1]))
def case(request):
    """(wav, q, n_valid, level, restatement, GPU (out, status, gain)): computed once per case, left unchanged"""
    (name, wav, q, nv), level = CASES[request.param[0]], request.param[1]
    return wav, q, nv, level, R.case_ref(name, level), _warp(wav, q, nv, level)


@gpu
def test_status_equals_the_restatement(case):
    wav, q, nv, level, ref, (out, status, gain) = case
    keep = ~ref.near
    assert status.shape == ref.status.shape
    assert not bool((status == POISON).any())                               # every frame's status written
    np.testing.assert_array_equal(status.numpy()[keep], ref.status[keep])


@gpu
def test_output_and_gain_against_fp64(case):
    wav, q, nv, level, ref, (out, status, gain) = case
    assert out.shape == wav.shape and bool(torch.isfinite(out).all())      # every element written over the NaN
    assert bool(torch.isfinite(gain).all())
    got = out.double().numpy()
    assert ref.left_out.mean() <= 0.01
    for b in range(wav.shape[0]):
        if ref.q[b] != 1.0 and (ref.status[b] == R.OK).any():              # both branches of the map were taken
            assert ref.below[b] > 0 and ref.above[b] > 0, (b, ref.below[b], ref.above[b])
        K = R.gain_bar(ref, b, C)
        g = ref.gain[b]
        gerr = abs(float(gain[b]) - g) / g
        print(f"row {b}: q {ref.q[b]:.4f} gain {float(gain[b]):.9g} ref {g:.9g} rel err {gerr / U:.3f} u, bar {K:.3f} u")
        assert gerr <= K * U
        r = ref.out[b]
        bar = (g * U * (np.abs(ref.Fa[b]) + np.abs(ref.Fb[b]) + 2.0 * np.abs(ref.Fa[b] + ref.Fb[b])) + U * np.abs(r)
               + U * np.abs(r) * K + C * np.abs(r).max())
        err = np.abs(got[b] - r)
        keep = ~ref.left_out[b]
        ratio = float((err[keep] / np.where(bar[keep] > 0, bar[keep], 1.0)).max()) if keep.any() else 0.0
        print(f"row {b}: worst error {err[keep].max():.3e}, worst error / bar {ratio:.3f}, peak {np.abs(r).max():.3f}")
        assert (err[keep] <= bar[keep]).all(), (b, ratio)


@gpu
def test_exact_behaviour(case):
    wav, q, nv, level, ref, (out, status, gain) = case
    x = torch.as_tensor(wav)
    for b in range(wav.shape[0]):
        n = int(nv[b])
        assert not bool(out[b, n:].any())                                   # exactly 0 from n_valid on
        if float(q[b]) == 1.0:
            assert torch.equal(_bits(out[b, :n]), _bits(x[b, :n]))          # bit for bit
            assert float(gain[b]) == 1.0 and not bool(status[b].any())
        if n == 0 or not x[b, :n].any():
            assert float(gain[b]) == 1.0 and bool((status[b] == R.SILENT).all()) and not bool(out[b].any())
        if not level:
            assert float(gain[b]) == 1.0


@gpu
def test_two_runs_the_binding_and_null_outputs_give_the_same_bits(case):
    from speech_anonymization_amd import ops
    wav, q, nv, level, _, (out, status, gain) = case
    again = _warp(wav, q, nv, level)
    for a, b in zip((out, status, gain), again):
        assert torch.equal(_bits(a), _bits(b))
    o2, g2, s2 = ops.pole_warp(*_dev(wav, q, nv), level, return_status=True)
    assert o2.is_cuda and g2.is_cuda and s2.is_cuda
    assert torch.equal(_bits(o2.cpu()), _bits(out)) and torch.equal(_bits(g2.cpu()), _bits(gain))
    assert torch.equal(s2.cpu(), status)
    assert len(ops.pole_warp(*_dev(wav, q, nv), level)) == 2
    o3, s3, g3 = _warp(wav, q, nv, level, want_status=False, want_gain=False)               # both may be NULL
    assert torch.equal(_bits(o3), _bits(out)) and bool((s3 == POISON).all()) and bool(torch.isnan(g3).all())


@gpu
def test_a_row_does_not_depend_on_its_batch():
    _, wav, q, nv = CASES[0]
    whole = _warp(wav, q, nv, True)
    for b in (0, 2):
        alone = _warp(wav[b:b + 1], q[b:b + 1], nv[b:b + 1], True)
        for a, w in zip(alone, whole):
            assert torch.equal(_bits(a), _bits(w[b:b + 1])), b


@gpu
def test_ratios_are_bounded_on_the_device():
    """q outside [0.5, 2] is the nearer bound and a NaN is 1, inside the kernel"""
    _, wav, _, nv = CASES[0]
    bad = np.array([0.3, 3.0, float("nan")], np.float32)
    good = np.array([0.5, 2.0, 1.0], np.float32)
    a, b = _warp(wav, bad, nv, True), _warp(wav, good, nv, True)
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v))
    assert bool(torch.isfinite(a[0]).all())
    assert torch.equal(_bits(a[0][2, :int(nv[2])]), _bits(torch.as_tensor(wav)[2, :int(nv[2])]))


@gpu
def test_pole_warp_entry_point_and_binding_refuse():
    """only arguments the library rejects before launching: -EINVAL, and the poisoned outputs untouched"""
    from speech_anonymization_amd import _lib, ops
    lib, E = _lib.load(), -errno.EINVAL
    assert [lib.sa_pole_warp_dim(i) for i in range(9)] == [lib.sa_mcadams_dim(i) for i in range(7)] + [850, E]
    assert ops.PW_KNEE == lib.sa_pole_warp_dim(7) / 1000.0 == R.KNEE
    B, N = 2, 800
    wav = torch.zeros(B, N, device=DEV)
    q = torch.full((B,), 0.9, device=DEV)
    nv = torch.full((B,), N, dtype=torch.int32, device=DEV)
    out = torch.full_like(wav, float("nan"))
    ws = ops.pole_warp_workspace(B, N, DEV).fill_(float("nan"))
    assert ws.numel() == ops.mcadams_workspace(B, N, DEV).numel()
    status = torch.full((B, M.n_frames(N)), POISON, dtype=torch.int32, device=DEV)
    gain = torch.full((B,), float("nan"), device=DEV)

    def call(wav=wav, q=q, nv=nv, B=B, N=N, out=out, ws=ws):
        return lib.sa_pole_warp(_f(wav), _f(q), _f(nv), B, N, 1, _f(out), _f(ws), _f(status), _f(gain), _lib.stream())

    for bad in (dict(wav=None), dict(q=None), dict(nv=None), dict(out=None), dict(ws=None), dict(B=0), dict(B=-2),
                dict(B=65536), dict(N=0), dict(N=-1), dict(N=(1 << 30) + 1)):
        assert call(**bad) == E, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()) and bool(torch.isnan(gain).all())
    assert bool((status == POISON).all())
    S = _lib.SaHipError
    with pytest.raises(S, match=r"\[B, N\]"):
        ops.pole_warp(wav[0], q, nv)
    with pytest.raises(S, match="q: expected shape"):
        ops.pole_warp(wav, q[:1], nv)
    with pytest.raises(S, match="n_valid: expected torch.int32"):
        ops.pole_warp(wav, q, nv.long())
    with pytest.raises(S, match="q: expected torch.float32"):
        ops.pole_warp(wav, q.double(), nv)
    with pytest.raises(S, match="contiguous"):
        ops.pole_warp(wav.t().contiguous().t(), q, nv)
    with pytest.raises(S, match="wav: the formant normalisation kernels take GPU tensors"):
        ops.pole_warp(wav.cpu(), q, nv)


# ---------------------------------------------------------------------------------------------------
# sa_formant_centre, on given tracks
# ---------------------------------------------------------------------------------------------------
CENTRE_T = (1, 7, 8, 9, 300, 5000)
CENTRE_TARGET = (700.0, 1300.0, 2600.0)                     # (near the given tracks: q inside the clamps)


@pytest.fixture(scope="module", params=CENTRE_T, ids=lambda T: f"T{T}")
def given(request):
    c = R.centre_case(request.param)
    return c, R.centre(*c, CENTRE_TARGET), _centre(*c, target=CENTRE_TARGET)


def _ulps(got, ref):
    return abs(float(got) - float(ref)) / LF.ulp32(ref)


@gpu
def test_medians_counts_and_ratio_against_the_restatement(given):
    c, want, got = given
    T = c[0].shape[1]
    print(f"T {T}: count {got['count'].tolist()} q {got['q'].tolist()} (restatement {want.q.tolist()})")
    np.testing.assert_array_equal(got["count"].numpy(), want.count)
    assert torch.equal(_bits(got["med"]), _bits(torch.from_numpy(want.med)))
    assert want.count[3] == 0 and got["q"][3] == 1.0 and not got["med"][3].any()             # fewer than min_frames
    for b in range(4):
        assert _ulps(got["q"][b], want.q[b]) <= 1.0, (b, float(got["q"][b]), float(want.q[b]))
    if T >= 300:
        assert (want.count[:3] >= R.MIN_FRAMES).all() and want.count[1] < want.count[0] == T
        assert all(0.8 < float(v) < 1.2 and float(v) != 1.0 for v in want.q[:3])              # not at a clamp


@gpu
def test_centre_twice_the_binding_null_outputs_and_no_f0(given):
    from speech_anonymization_amd import ops
    c, _, first = given
    again = _centre(*c, target=CENTRE_TARGET)
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(again[k])), k
    freq, status, f0, frames = _dev(*c)
    med, q, count = ops.formant_centre(freq, status, f0, frames, CENTRE_TARGET)
    assert med.is_cuda and q.is_cuda and count.is_cuda
    assert torch.equal(_bits(med.cpu()), _bits(first["med"])) and torch.equal(_bits(q.cpu()), _bits(first["q"]))
    assert torch.equal(count.cpu(), first["count"])
    bare = _centre(*c, target=CENTRE_TARGET, want=(False, False))                             # both may be NULL
    assert torch.equal(_bits(bare["q"]), _bits(first["q"]))
    assert bool(torch.isnan(bare["med"]).all()) and bool((bare["count"] == POISON).all())
    # f0 = NULL: every frame counts as voiced
    want = R.centre(c[0], c[1], None, c[3], CENTRE_TARGET)
    got = _centre(c[0], c[1], None, c[3], target=CENTRE_TARGET)
    np.testing.assert_array_equal(got["count"].numpy(), want.count)
    assert torch.equal(_bits(got["med"]), _bits(torch.from_numpy(want.med)))
    assert all(_ulps(got["q"][b], want.q[b]) <= 1.0 for b in range(4))
    m2, q2, c2 = ops.formant_centre(freq, status, None, frames, CENTRE_TARGET)
    assert torch.equal(_bits(q2.cpu()), _bits(got["q"])) and torch.equal(c2.cpu(), got["count"])


@gpu
def test_target_clamps_and_min_frames_on_the_gpu():
    freq, status, f0, frames = R.centre_case(300)
    want = R.centre(freq, status, f0, frames, CENTRE_TARGET)
    # a row whose medians are the target gives exactly 1
    row0 = tuple(float(v) for v in want.med[0])
    got = _centre(freq, status, f0, frames, target=row0)
    assert float(got["q"][0]) == 1.0 and float(got["q"][1]) != 1.0
    # the clamps, at both ends
    high = _centre(freq, status, f0, frames, target=(1400.0, 2440.0, 5200.0))
    low = _centre(freq, status, f0, frames, target=(350.0, 610.0, 1300.0))
    assert bool((high["q"][:3] == np.float32(1.2)).all()) and bool((low["q"][:3] == np.float32(0.8)).all())
    wide = _centre(freq, status, f0, frames, target=(1400.0, 2440.0, 5200.0), q_min=0.5, q_max=2.0)
    assert all(1.2 < float(v) <= 2.0 for v in wide["q"][:3])
    assert float(high["q"][3]) == 1.0 and float(low["q"][3]) == 1.0                          # not scored: left alone
    # min_frames at a row's count scores the row, one above it does not
    n = int(want.count[1])
    at = _centre(freq, status, f0, frames, target=CENTRE_TARGET, m=n)
    above = _centre(freq, status, f0, frames, target=CENTRE_TARGET, m=n + 1)
    assert at["count"][1] == n and _ulps(at["q"][1], want.q[1]) <= 1.0
    assert above["count"][1] == 0 and float(above["q"][1]) == 1.0 and not above["med"][1].any()
    few = R.centre(freq, status, f0, frames, CENTRE_TARGET, min_frames=1)
    n3 = int(few.count[3])
    assert 1 <= n3 < R.MIN_FRAMES
    got3 = _centre(freq, status, f0, frames, target=CENTRE_TARGET, m=n3)
    assert got3["count"][3] == n3 and torch.equal(_bits(got3["med"][3]), _bits(torch.from_numpy(few.med[3])))
    assert _centre(freq, status, f0, frames, target=CENTRE_TARGET, m=n3 + 1)["count"][3] == 0


@gpu
def test_centre_entry_point_and_binding_refuse():
    from speech_anonymization_amd import _lib, ops
    lib, E = _lib.load(), -errno.EINVAL
    B, T = 2, 20
    F = torch.full((B, T, 3), 500.0, device=DEV)
    st = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    f0 = torch.full((B, T), 120.0, device=DEV)
    fr = torch.full((B,), T, dtype=torch.int32, device=DEV)
    med = torch.full((B, 3), float("nan"), device=DEV)
    q = torch.full((B,), float("nan"), device=DEV)
    count = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    cf = ctypes.c_float

    def call(F=F, st=st, fr=fr, q=q, B=B, T=T, t=(550.0, 1650.0, 2750.0), lo=0.8, hi=1.2, m=8):
        return lib.sa_formant_centre(_f(F), _f(st), _f(f0), _f(fr), B, T, cf(t[0]), cf(t[1]), cf(t[2]), cf(lo), cf(hi), m,
                                     _f(med), _f(q), _f(count), _lib.stream())

    for bad in (dict(F=None), dict(st=None), dict(fr=None), dict(q=None), dict(B=0), dict(B=-2), dict(B=65536), dict(T=0),
                dict(T=-1), dict(T=104859), dict(t=(89.0, 1650.0, 2750.0)), dict(t=(550.0, 550.0, 2750.0)),
                dict(t=(550.0, 2750.0, 1650.0)), dict(t=(550.0, 1650.0, 5501.0)), dict(t=(float("nan"), 1650.0, 2750.0)),
                dict(lo=0.49), dict(lo=1.01), dict(hi=0.99), dict(hi=2.01), dict(lo=float("nan")), dict(m=0), dict(m=-3)):
        assert call(**bad) == E, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(med).all()) and bool(torch.isnan(q).all()) and bool((count == POISON).all())
    S = _lib.SaHipError
    tg = (550.0, 1650.0, 2750.0)
    with pytest.raises(S, match=r"freq: expected \[B, T, 3\]"):
        ops.formant_centre(F[0], st, f0, fr, tg)
    with pytest.raises(S, match="status: expected torch.int32"):
        ops.formant_centre(F, st.long(), f0, fr, tg)
    with pytest.raises(S, match="f0: expected shape"):
        ops.formant_centre(F, st, f0[:, :5].contiguous(), fr, tg)
    with pytest.raises(S, match="f0: expected a contiguous"):
        ops.formant_centre(F, st, f0.t().contiguous().t(), fr, tg)
    with pytest.raises(S, match="frames: the formant normalisation kernels take GPU tensors"):
        ops.formant_centre(F, st, f0, fr.cpu(), tg)
    with pytest.raises(S, match="target_hz"):
        ops.formant_centre(F, st, f0, fr, (550.0, 1650.0))
    with pytest.raises(S, match="target_hz"):
        ops.formant_centre(F, st, f0, fr, (50.0, 1650.0, 2750.0))
    with pytest.raises(S, match="q_min"):
        ops.formant_centre(F, st, f0, fr, tg, q_min=1.1)
    for m in (0, -1, True, 2.5):
        with pytest.raises(S, match="min_frames, a count of frames, 1 or more"):
            ops.formant_centre(F, st, f0, fr, tg, min_frames=m)


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("q", R.E2E_RATIOS)
def test_a_given_ratio_moves_every_formant_by_it(q):
    """FormantNormalizer(ratio=q) read by metrics.formant_shift with every frame voiced at the known fundamental:
    each per-formant ratio within twice the restatement's recorded relative distance from q"""
    from speech_anonymization_amd import formantnorm, metrics
    rows = torch.from_numpy(LF.e2e_rows()).to(DEV)
    B, N = rows.shape
    T = N // 160 + 1
    fn = formantnorm.FormantNormalizer(ratio=q)
    out = fn(rows, torch.ones(B))
    assert out.shape == rows.shape and out.dtype == torch.float32 and all(v.is_cuda for v in fn.last)
    assert torch.equal(fn.last[0].cpu(), torch.full((B,), q))
    counts = fn.last[4].cpu()
    assert counts.sum(1).tolist() == [M.n_frames(N)] * B and not bool(counts[:, 2].any())   # no frame fell back
    f0 = torch.from_numpy(LF.known_f0(T)).to(DEV)
    nv = torch.full((B,), N, dtype=torch.int32, device=DEV)
    cols = [c.cpu() for c in metrics.formant_shift(rows, out.contiguous(), nv, f0, f0,
                                                   torch.full((B,), T, dtype=torch.int32, device=DEV))]
    ratio, common = torch.stack(cols[3:6], 1).double().numpy(), cols[7].tolist()
    rec = R.recorded()["open"][str(q)]
    for b in range(B):
        d = [abs(ratio[b, k] / float(np.float32(q)) - 1.0) for k in range(3)]
        print(f"q {q} row {b}: ratios {ratio[b].tolist()} (restatement {rec['ratio'][b]}) distance {d} bars "
              f"{[2.0 * v for v in rec['worst']]} common {common[b]}")
    assert min(common) >= 8
    for b in range(B):
        for k in range(3):
            assert abs(ratio[b, k] / float(np.float32(q)) - 1.0) <= 2.0 * rec["worst"][k], (b, k)


@gpu
def test_the_closed_loop_brings_the_formants_to_the_target():
    """two rows with their resonances at 0.9 x and 1.12 x, target (600, 1350, 2500): |ln| of the geometric distance of
    the medians from the target is at most twice the restatement's recorded value afterwards, and smaller than before"""
    from speech_anonymization_amd import formantnorm, ops
    rows = torch.from_numpy(R.closed_rows()).to(DEV)
    B, N = rows.shape
    T = N // 160 + 1
    f0 = torch.from_numpy(R.closed_f0(T)).to(DEV)
    nv = torch.full((B,), N, dtype=torch.int32, device=DEV)
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    rec = R.recorded()["closed"]

    def medians(wav):
        freq, status = ops.formant_tracks(wav, nv)
        return ops.formant_centre(freq, status, f0, frames, R.CLOSED_TARGET)

    med0, q, count0 = medians(rows)
    out, gain = ops.pole_warp(rows, q, nv)
    med1, _, count1 = medians(out)
    for b in range(B):
        before = R.geometric_distance(med0[b].tolist(), R.CLOSED_TARGET)
        after = R.geometric_distance(med1[b].tolist(), R.CLOSED_TARGET)
        print(f"row {b}: q {float(q[b]):.6f} (restatement {rec['q'][b]:.6f}) distance before {before:.6f} after "
              f"{after:.6f} (restatement {rec['distance_before'][b]:.6f}, {rec['distance_after'][b]:.6f}) frames "
              f"{int(count0[b])}, {int(count1[b])}")
        assert int(count0[b]) >= 8 and int(count1[b]) >= 8
        assert abs(math.log(after)) <= 2.0 * rec["abs_ln_after"][b]
        assert abs(math.log(after)) < abs(math.log(before))
    # the class on the same rows, with the F0 track given by the known fundamental
    fn = formantnorm.FormantNormalizer(target_hz=R.CLOSED_TARGET)
    real, formantnorm.f0_track = formantnorm.f0_track, lambda wav, *a, **k: f0
    try:
        assert torch.equal(_bits(fn(rows, torch.ones(B))), _bits(out))
    finally:
        formantnorm.f0_track = real
    assert torch.equal(_bits(fn.last[0]), _bits(q)) and torch.equal(fn.last[2], count0)


UTT_KEYS = {"q", "gain", "formant_frames_in", "f1_in_hz", "f2_in_hz", "f3_in_hz", "silent_frames", "fallback_frames",
            "peak", "samples"}


@gpu
def test_anonymize_ratio_one_is_the_identity(tmp_path):
    """--formant_norm_ratio 1.0 in a child process: the documented keys, every output its input bit for bit (as the
    16-bit files hold them), every reported ratio exactly 1"""
    from speech_anonymization_amd import data
    out = tmp_path / "one"
    res = anon_cli.run_child(["--device", DEV, "--synthetic", "4", "--seed", "1986", "--batch_size", "3", "--out_dir",
                              str(out), "--formant_norm_ratio", "1.0", "--report_formants", "true"])
    assert res["formant_norm"] is True and res["formant_norm_ratio"] == 1.0 and res["level"] is True
    assert "mcadams" not in res and "pitch_norm" not in res and "model_type" not in res
    assert sorted(os.listdir(out)) == [f"synthetic_{i:04d}.wav" for i in range(4)] and len(res["utterances"]) == 4
    rows = []
    for batch in data.synthetic_gender_dataset(4, 3, seed=1986):
        wavs, lens = batch.sig
        rows += [wavs[i, :int(round(float(lens[i]) * wavs.shape[1]))] for i in range(wavs.shape[0])]
    for i, u in enumerate(res["utterances"]):
        assert UTT_KEYS <= set(u), u
        assert u["q"] == 1.0 and u["gain"] == 1.0 and u["formant_frames_in"] == 0 and u["f1_in_hz"] is None
        assert u["samples"] == rows[i].shape[0]
        data.write_audio(str(tmp_path / "in.wav"), rows[i].float())
        assert open(tmp_path / "in.wav", "rb").read() == open(out / f"{u['id']}.wav", "rb").read()
        if u["formant_frames"]:
            assert u["f1_shift"] == u["f2_shift"] == u["f3_shift"] == u["formant_shift"] == 1.0


@gpu
def test_anonymize_formants_then_psola(tmp_path):
    """--formant_norm true --pitch_norm true --psola true: both stages run and write their keys"""
    res = anon_cli.run_child(["--device", DEV, "--synthetic", "4", "--out_dir", str(tmp_path / "both"), "--formant_norm",
                              "true", "--pitch_norm", "true", "--psola", "true", "--report_f0", "true"])
    assert res["formant_norm"] is True and res["pitch_norm"] is True and res["psola"] is True
    assert res["pitch_target_hz"] == 170.0 and res["target_hz"] == [550.0, 1650.0, 2750.0]
    assert res["q_min"] == 0.8 and res["q_max"] == 1.2 and res["min_frames"] == 8
    for u in res["utterances"]:
        assert UTT_KEYS | {"ratio", "f0_mean_hz", "voiced_share"} <= set(u), u
        assert float(np.float32(0.8)) <= u["q"] <= float(np.float32(1.2)) and u["gain"] > 0     # (q is an fp32) and 0.5 <= u["ratio"] <= 2.0 and 0 < u["peak"] < 4
        if u["formant_frames_in"]:
            assert u["formant_frames_in"] >= 8 and 90.0 <= u["f1_in_hz"] < u["f2_in_hz"] < u["f3_in_hz"] <= 5500.0
        else:
            assert u["q"] == 1.0 and u["f1_in_hz"] is None and u["f2_in_hz"] is None and u["f3_in_hz"] is None


@gpu
@pytest.mark.parametrize("extra, pitch", [([], False), (["--pitch_norm", "true"], True)], ids=["formants", "and_psola"])
def test_recipe_trains_one_epoch(tmp_path, extra, pitch):
    """a fresh child process, under a time limit; no error bar: one epoch on 16 synthetic utterances"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "gender_classifier_train_formant_norm.py"),
                        os.path.join(root, "speechbrain_configs", "gender_classifier_formant_norm.yaml"), "--device", DEV,
                        "--output_folder", str(tmp_path / "recipe"), "--synthetic", "16", "--number_of_epochs", "1"]
                       + extra, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["formant_norm"] is True and summary["target_hz"] == [550.0, 1650.0, 2750.0]
    assert summary["pitch_norm"] is pitch and summary.get("psola") == (True if pitch else None)
    assert np.isfinite(summary["test_loss"]) and 0.0 <= summary["test_error"] <= 1.0
