"""The source-filter resynthesis on the GPU (include/sa_hip.h carries the definition) against the
integer / fp64 restatement tests/srcfilt_ref.py.

The pulse table (sa_srcfilt_pulses) and the excitation (sa_srcfilt_excite) are compared bit for bit: every decision
behind them is made on integers or on one correctly rounded fp64 operation, and the excitation's fp32 operations are
rounded one by one.  Only the synthesis (sa_srcfilt_synth) has a bar, DESIGN section 17's per sample:

    |out - ref| <= g u (|F_a| + |F_b| + 2 |F_a + F_b|) + u |ref| + u |ref| K + C max|ref_row|

u = 2^-24; K from tests/mcadams_ref.gain_bar, the gain itself held to K u; C = 16 x the worst distance between the
restatement and itself under three perturbations (lag sums and Ee from the far end, the filter's taps in the opposite
order), measured by tools/srcfilt_delta.py on these very cases and read from profiles/srcfilt_delta.json -- never
measured on the kernel.  The statuses are compared exactly; tests/test_srcfilt_cpu.py checks first that no frame of the
inputs lies near a decision, so no sample is left out (the cap would be 1 %).

End to end, SourceFilter on the three 4800-sample voiced rows at their own pitch and at 170 Hz: the voiced-mean F0 by
the restatement's tracker and the envelope peak near 1220 Hz, each allowed twice the distance the delta tool measured
on the restatement (DESIGN section 25's rule)."""
import ctypes
import errno
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from speech_anonymization_amd import sourcefilter  # noqa: F401  (without the feature nothing here can run)
from tests import anon_cli
from tests import mcadams_ref as M
from tests import srcfilt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = R.U
gpu = pytest.mark.gpu
POISON = -7


def _f(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV).contiguous()


def _pulses(f0, rho_q, nv, N):
    """sa_srcfilt_pulses through the library itself, into poisoned tables -> (pos_q, period_q, count) on the device"""
    from speech_anonymization_amd import _lib
    f0, rho_q, nv = _dev(f0, torch.float32), _dev(rho_q, torch.int32), _dev(nv, torch.int32)
    B, T = f0.shape
    K = N // 40 + 2
    pos = torch.full((B, K), POISON, dtype=torch.int64, device=DEV)
    per = torch.full((B, K), POISON, dtype=torch.int32, device=DEV)
    count = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    rc = _lib.load().sa_srcfilt_pulses(_f(f0), _f(rho_q), _f(nv), B, N, T, _f(pos), _f(per), _f(count), _lib.stream())
    assert rc == 0
    return pos, per, count


def _excite(f0, pos, per, count, seed, nv, N, aspiration):
    from speech_anonymization_amd import _lib
    f0, seed, nv = _dev(f0, torch.float32), _dev(seed, torch.int32), _dev(nv, torch.int32)
    B, T = f0.shape
    exc = torch.full((B, N), float("nan"), device=DEV)
    rc = _lib.load().sa_srcfilt_excite(_f(f0), _f(pos), _f(per), _f(count), _f(seed), _f(nv), B, N, T,
                                       ctypes.c_float(aspiration), _f(exc), _lib.stream())
    assert rc == 0
    return exc


def _synth(wav, exc, nv, level, want_status=True, want_gain=True):
    """sa_srcfilt_synth into buffers poisoned with NaN -> (out, status, gain) on the CPU"""
    from speech_anonymization_amd import _lib, ops
    wav, exc, nv = _dev(wav, torch.float32), _dev(exc, torch.float32), _dev(nv, torch.int32)
    B, N = wav.shape
    out = torch.full_like(wav, float("nan"))
    ws = ops.srcfilt_workspace(B, N, DEV).fill_(float("nan"))
    status = torch.full((B, M.n_frames(N)), POISON, dtype=torch.int32, device=DEV)
    gain = torch.full((B,), float("nan"), device=DEV)
    rc = _lib.load().sa_srcfilt_synth(_f(wav), _f(exc), _f(nv), B, N, int(level), _f(out), _f(ws),
                                      _f(status) if want_status else None, _f(gain) if want_gain else None,
                                      _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu(), status.cpu(), gain.cpu()


def _bits(t):
    return t.cpu().contiguous().view(torch.int32).numpy()


def _check_tables(got, want):
    pos, per, count = (v.cpu().numpy() for v in got)
    rpos, rper, rcount = want
    np.testing.assert_array_equal(count, rcount)
    for b in range(len(count)):
        k = int(count[b])
        np.testing.assert_array_equal(pos[b, :k], rpos[b, :k])
        np.testing.assert_array_equal(per[b, :k], rper[b, :k])
        assert (pos[b, k:] == POISON).all() and (per[b, k:] == POISON).all()       # nothing written past the count


# ---------------------------------------------------------------------------------------------------
# pulses and excitation: equal bits
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rho", ["null", "to_170", "clamped"])
@pytest.mark.parametrize("padded", [False, True], ids=["T_floor", "T_ceil"])
@pytest.mark.parametrize("name", list(R.waves()))
def test_pulse_table_and_excitation_equal_the_restatement(name, padded, rho):
    from speech_anonymization_amd import ops
    wav, nv, f0, seed = R.case_inputs(name, padded)
    B, N = wav.shape
    rho_q = R.rho_variants(name, f0.shape[1])[rho]
    want = R.pulses(f0, rho_q, nv, N)
    got = _pulses(f0, rho_q, nv, N)
    _check_tables(got, want)
    bound = ops.srcfilt_pulses(_dev(f0), _dev(rho_q, torch.int32), _dev(nv), N=N)
    _check_tables([torch.where(torch.arange(N // 40 + 2, device=DEV)[None] < bound[2][:, None], t,
                               torch.full_like(t, POISON)) for t in bound[:2]] + [bound[2]], want)
    for asp in (0.0, 0.3):
        ref = R.excite(f0, *want, seed, nv, N, asp)
        exc = _excite(f0, *got, seed, nv, N, asp)
        assert bool(torch.isfinite(exc).all())               # every element written over the NaN
        np.testing.assert_array_equal(_bits(exc), ref.view(np.int32))
        again = ops.srcfilt_excite(_dev(f0), *bound, _dev(seed), _dev(nv), asp, N=N)
        assert torch.equal(_bits_t(again), _bits_t(exc))
        for b in range(B):
            assert not bool(exc[b, max(int(nv[b]), 0):].any())


def _bits_t(t):
    return t.contiguous().view(torch.int32)


@gpu
def test_pulses_restage_their_periods_past_1024_frames():
    """N = 170000 has 1063 frames: the walk stages the periods twice.  A track of voiced stretches at drifting pitch
    with unvoiced gaps, NaNs and a per-frame rho; tables and excitation equal the restatement's bits"""
    N = 170000
    T = R.frames_of_track(N)
    rng = np.random.default_rng(27)
    f0 = (110.0 + 90.0 * rng.random((2, T))).astype(np.float32)
    f0[0, (np.arange(T) // 37) % 3 == 1] = 0.0
    f0[1, rng.random(T) < 0.1] = np.nan
    f0[1, 1000:1030] = 0.0
    rho_q = (R.ONE * (0.6 + 1.2 * rng.random((2, T)))).astype(np.int32)
    nv, seed = np.array([N, 169000], np.int32), np.array([5, 6], np.int32)
    want = R.pulses(f0, rho_q, nv, N)
    assert want[2].min() > 1000 and (want[0][:, 0] == 0).all()
    got = _pulses(f0, rho_q, nv, N)
    _check_tables(got, want)
    exc = _excite(f0, *got, seed, nv, N, 0.3)
    np.testing.assert_array_equal(_bits(exc), R.excite(f0, *want, seed, nv, N, 0.3).view(np.int32))


# ---------------------------------------------------------------------------------------------------
# synthesis: statuses exact, output under the bar
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def C():
    rec = R.load_delta()
    c = R.C_FACTOR * rec["c"]["worst"]
    assert c < U / 4.0
    return c


@pytest.fixture(scope="module", params=list(R.SYNTH_CASES), ids=lambda p: "%s_asp%g" % p)
def case(request):
    """(wav, n_valid, the restatement at level on, the GPU's (out, status, gain) at level on and off): once per case,
    left unchanged.  The excitation handed to the kernel is the restatement's, which the tests above hold the
    excitation kernel to bit for bit."""
    name, asp = request.param
    wav, nv, _, _ = R.case_inputs(name)
    ref = R.case_ref(name, asp)
    return wav, nv, ref, _synth(wav, ref.exc, nv, True), _synth(wav, ref.exc, nv, False)


@gpu
def test_status_equals_the_restatement(case):
    wav, nv, ref, (out, status, gain), (_, status_off, _) = case
    assert not ref.near.any()
    assert status.shape == ref.status.shape and not bool((status == POISON).any())
    np.testing.assert_array_equal(status.numpy(), ref.status)
    assert torch.equal(status, status_off)


@gpu
def test_status_three_frames_are_written_as_zeros():
    """aspiration 0: the frame of row 2 over [960, 1280) is voiced and the chain leaves it without a pulse; row 0's last
    frame holds one term, where the window is 0"""
    wav, nv, _, _ = R.case_inputs("odd")
    ref = R.case_ref("odd", 0.0)
    out, status, gain = _synth(wav, ref.exc, nv, True)
    assert int(status[2, 7]) == R.UNEXCITED and int(status[0, 11]) == R.UNEXCITED
    assert int((status == R.UNEXCITED).sum()) == int((ref.status == R.UNEXCITED).sum()) == 2
    assert not ref.F[2, 7].any() and not ref.F[0, 11].any()
    # [1600, 1687) of row 0 is frame 10's second half alone: the kernel's frame 11 added exactly nothing
    want = ref.gain[0] * ref.F[0, 10, 160:247]
    assert np.abs(out[0, 1600:].double().numpy() - want).max() <= 4.0 * U * np.abs(want).max()


@gpu
@pytest.mark.parametrize("level", [True, False], ids=["level", "no_level"])
def test_output_against_fp64(case, C, level):
    wav, nv, ref, on, off = case
    out, status, gain = on if level else off
    assert out.shape == wav.shape and bool(torch.isfinite(out).all())     # every element written over the NaN
    assert bool(torch.isfinite(gain).all())
    got = out.double().numpy()
    assert ref.left_out.mean() <= 0.01 and not ref.left_out.any()
    for b in range(wav.shape[0]):
        K = M.gain_bar(ref, b, C) if level else 1.0
        g = ref.gain[b] if level else 1.0
        gerr = abs(float(gain[b]) - g) / g
        print(f"row {b}: gain {float(gain[b]):.9g} ref {g:.9g} rel err {gerr / U:.3f} u, bar {K:.3f} u")
        if level:
            assert gerr <= K * U
        else:
            assert float(gain[b]) == 1.0
        r = ref.out[b] if level else ref.y[b]
        bar = (g * U * (np.abs(ref.Fa[b]) + np.abs(ref.Fb[b]) + 2.0 * np.abs(ref.Fa[b] + ref.Fb[b])) + U * np.abs(r)
               + U * np.abs(r) * K + C * np.abs(r).max())
        err = np.abs(got[b] - r)
        ratio = float((err / np.where(bar > 0, bar, 1.0)).max())
        print(f"row {b}: worst error {err.max():.3e}, worst error / bar {ratio:.3f}, peak {np.abs(r).max():.3f}")
        assert (err <= bar).all(), (b, ratio)


@gpu
def test_exact_behaviour(case):
    wav, nv, ref, (out, status, gain), (out_off, _, gain_off) = case
    for b in range(wav.shape[0]):
        n = int(nv[b])
        assert not bool(out[b, n:].any()) and not bool(out_off[b, n:].any())        # exactly 0 from n_valid on
        if n == 0:
            assert float(gain[b]) == 1.0 and bool((status[b] == R.SILENT).all()) and not bool(out[b].any())
        else:
            assert bool(out[b, :n].any())
    assert bool((gain_off == 1.0).all())


@gpu
def test_two_runs_a_row_alone_and_the_binding_give_the_same_bits(case):
    from speech_anonymization_amd import ops
    wav, nv, ref, (out, status, gain), _ = case
    again = _synth(wav, ref.exc, nv, True)
    assert torch.equal(_bits_t(again[0]), _bits_t(out)) and torch.equal(again[1], status)
    assert torch.equal(_bits_t(again[2]), _bits_t(gain))
    o2, g2, s2 = ops.srcfilt_synth(_dev(wav), _dev(ref.exc), _dev(nv), True, return_status=True)
    assert torch.equal(_bits_t(o2.cpu()), _bits_t(out)) and torch.equal(g2.cpu(), gain) and torch.equal(s2.cpu(), status)
    o3, _, _ = _synth(wav, ref.exc, nv, True, want_status=False, want_gain=False)   # both may be NULL
    assert torch.equal(_bits_t(o3), _bits_t(out))
    for b in range(wav.shape[0]):                            # a row alone: the bits it has inside the batch
        o1, s1, g1 = _synth(wav[b:b + 1], ref.exc[b:b + 1], nv[b:b + 1], True)
        assert torch.equal(_bits_t(o1[0]), _bits_t(out[b])) and torch.equal(s1[0], status[b]) and g1[0] == gain[b]


@gpu
def test_the_three_in_a_row_equal_the_steps_and_rows_do_not_depend_on_the_batch():
    from speech_anonymization_amd import ops
    wav, nv, f0, seed = R.case_inputs("odd")
    B, N = wav.shape
    rho_q = R.rho_variants("odd", f0.shape[1])["to_170"]
    ref = R.srcfilt(wav, f0, rho_q, seed, nv, 0.3, True)
    args = (_dev(wav), _dev(f0), _dev(rho_q, torch.int32), _dev(seed), _dev(nv))
    out, gain, count, status = ops.srcfilt(*args, 0.3, True, return_status=True)
    np.testing.assert_array_equal(count.cpu().numpy(), ref.count)
    np.testing.assert_array_equal(status.cpu().numpy(), ref.status)
    o, s, g = _synth(wav, ref.exc, nv, True)
    assert torch.equal(_bits_t(out.cpu()), _bits_t(o)) and torch.equal(gain.cpu(), g)
    out2, gain2, count2 = ops.srcfilt(*args, 0.3, True)
    assert torch.equal(out2, out) and torch.equal(gain2, gain) and torch.equal(count2, count)
    none = ops.srcfilt(args[0], args[1], None, args[3], args[4], 0.3, True)          # rho_q NULL is 2^16 throughout
    ones = ops.srcfilt(args[0], args[1], torch.full_like(args[2], R.ONE), args[3], args[4], 0.3, True)
    assert all(torch.equal(a, b) for a, b in zip(none, ones))
    for b in range(B):
        alone = ops.srcfilt(*(a[b:b + 1].contiguous() for a in args), 0.3, True)
        assert torch.equal(alone[0][0], out[b]) and alone[1][0] == gain[b] and alone[2][0] == count[b]


@gpu
def test_the_three_frame_kernels_agree_on_which_frames_are_silent_or_kept():
    """sa_mcadams, sa_pole_warp and sa_srcfilt_synth frame, sum and fit through one text (csrc/sa_lpc_shared.h): on the
    width-16037 batch (no multiple of the hop; rows cut at 1.0, 0.73 and 0.5 of it, so there are voiced frames and
    frames past n_valid), with no alpha or q equal to 1, they mark the same frames silent, a frame whose fit fails in
    one fails in all, and the two that go on to the roots agree throughout."""
    from speech_anonymization_amd import data, ops
    wav = next(iter(data.synthetic_gender_dataset(3, 3, n_samples=16037, seed=7))).sig[0].to(DEV).contiguous()
    B, N = wav.shape
    nv = torch.round(torch.tensor([1.0, 0.73, 0.5], dtype=torch.float64) * N).to(torch.int32).to(DEV)
    f0 = ops.yin_f0(wav)
    pos_q, period_q, count = ops.srcfilt_pulses(f0, None, nv, N=N)
    exc = ops.srcfilt_excite(f0, pos_q, period_q, count, _dev([11, 12, 13], torch.int32), nv, N=N)
    mc = ops.mcadams(wav, _dev([0.8, 0.9, 1.1], torch.float32), nv, return_status=True)[2]
    pw = ops.pole_warp(wav, _dev([0.9, 1.1, 1.2], torch.float32), nv, return_status=True)[2]
    sf = ops.srcfilt_synth(wav, exc, nv, return_status=True)[2]
    assert bool((sf == R.SILENT).any()) and bool((sf == 0).any()) and bool((f0 > 0).any())
    assert torch.equal(mc == R.SILENT, sf == R.SILENT) and torch.equal(pw == R.SILENT, sf == R.SILENT)
    assert bool((mc[sf == 2] == 2).all()) and bool((pw[sf == 2] == 2).all())
    assert torch.equal(mc, pw)


@gpu
def test_entry_points_and_bindings_refuse():
    """only arguments the library rejects before launching: -EINVAL, and the poisoned outputs untouched"""
    from speech_anonymization_amd import _lib, ops
    lib, E = _lib.load(), -errno.EINVAL
    B, N, T = 2, 800, 6
    K = N // 40 + 2
    f0 = torch.full((B, T), 150.0, device=DEV)
    rho = torch.full((B, T), R.ONE, dtype=torch.int32, device=DEV)
    nv = torch.full((B,), N, dtype=torch.int32, device=DEV)
    seed = torch.zeros(B, dtype=torch.int32, device=DEV)
    wav = torch.zeros(B, N, device=DEV)
    pos = torch.full((B, K), POISON, dtype=torch.int64, device=DEV)
    per = torch.full((B, K), POISON, dtype=torch.int32, device=DEV)
    count = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    exc = torch.full((B, N), float("nan"), device=DEV)
    out = torch.full((B, N), float("nan"), device=DEV)
    ws = ops.srcfilt_workspace(B, N, DEV).fill_(float("nan"))
    status = torch.full((B, M.n_frames(N)), POISON, dtype=torch.int32, device=DEV)
    gain = torch.full((B,), float("nan"), device=DEV)
    st = _lib.stream()

    def pulses(f0=f0, nv=nv, B=B, N=N, T=T, pos=pos, per=per, count=count):
        return lib.sa_srcfilt_pulses(_f(f0), _f(rho), _f(nv), B, N, T, _f(pos), _f(per), _f(count), st)

    def excite(f0=f0, tab=pos, per=per, cnt=count, seed=seed, nv=nv, B=B, N=N, T=T, asp=0.3, exc=exc):
        return lib.sa_srcfilt_excite(_f(f0), _f(tab), _f(per), _f(cnt), _f(seed), _f(nv), B, N, T, ctypes.c_float(asp),
                                     _f(exc), st)

    def synth(wav=wav, e=wav, nv=nv, B=B, N=N, out=out, ws=ws):
        return lib.sa_srcfilt_synth(_f(wav), _f(e), _f(nv), B, N, 1, _f(out), _f(ws), _f(status), _f(gain), st)

    for bad in (dict(f0=None), dict(nv=None), dict(pos=None), dict(per=None), dict(count=None), dict(B=0), dict(B=65536),
                dict(N=0), dict(N=(1 << 24) + 1), dict(T=5), dict(T=7), dict(T=0)):
        assert pulses(**bad) == E, bad
    for bad in (dict(f0=None), dict(tab=None), dict(per=None), dict(cnt=None), dict(seed=None), dict(nv=None),
                dict(exc=None), dict(B=0), dict(B=65536), dict(N=0), dict(N=(1 << 24) + 1), dict(T=5), dict(T=7),
                dict(asp=-0.01), dict(asp=1.01), dict(asp=float("nan"))):
        assert excite(**bad) == E, bad
    for bad in (dict(wav=None), dict(e=None), dict(nv=None), dict(out=None), dict(ws=None), dict(B=0), dict(B=-2),
                dict(B=65536), dict(N=0), dict(N=-1), dict(N=(1 << 24) + 1)):
        assert synth(**bad) == E, bad
    torch.cuda.synchronize()
    assert bool((pos == POISON).all()) and bool((per == POISON).all()) and bool((count == POISON).all())
    assert bool(torch.isnan(exc).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())
    assert bool(torch.isnan(gain).all()) and bool((status == POISON).all())
    S = _lib.SaHipError
    with pytest.raises(S, match=r"f0: expected \[B, T\]"):
        ops.srcfilt_pulses(f0[0], rho, nv, N=N)
    with pytest.raises(S, match="f0 has 6 frames"):
        ops.srcfilt_pulses(f0, rho, nv, N=N + 160)
    with pytest.raises(S, match="rho_q: expected torch.int32"):
        ops.srcfilt_pulses(f0, rho.long(), nv, N=N)
    with pytest.raises(S, match="n_valid: expected shape"):
        ops.srcfilt_pulses(f0, rho, nv[:1], N=N)
    with pytest.raises(S, match="contiguous"):
        ops.srcfilt_pulses(f0.t().contiguous().t(), rho, nv, N=N)
    good = ops.srcfilt_pulses(f0, rho, nv, N=N)
    with pytest.raises(S, match="pos_q: expected torch.int64"):
        ops.srcfilt_excite(f0, good[0].int(), good[1], good[2], seed, nv, N=N)
    with pytest.raises(S, match="period_q: expected shape"):
        ops.srcfilt_excite(f0, good[0], good[1][:, :5].contiguous(), good[2], seed, nv, N=N)
    with pytest.raises(S, match="seed: expected torch.int32"):
        ops.srcfilt_excite(f0, *good, seed.long(), nv, N=N)
    with pytest.raises(S, match="aspiration 1.5 in 0..1"):
        ops.srcfilt_excite(f0, *good, seed, nv, 1.5, N=N)
    with pytest.raises(S, match="aspiration nan in 0..1"):
        ops.srcfilt(wav, f0, rho, seed, nv, float("nan"))
    with pytest.raises(S, match=r"\[B, N\]"):
        ops.srcfilt_synth(wav[0], wav[0], nv)
    with pytest.raises(S, match="exc: expected shape"):
        ops.srcfilt_synth(wav, wav[:, :10].contiguous(), nv)
    with pytest.raises(S, match="wav: expected torch.float32"):
        ops.srcfilt_synth(wav.double(), wav, nv)
    with pytest.raises(S, match="GPU tensors"):
        ops.srcfilt_synth(wav.cpu(), wav, nv)


# ---------------------------------------------------------------------------------------------------
# the class, end to end
# ---------------------------------------------------------------------------------------------------
@gpu
def test_sourcefilter_runs_without_a_host_copy_and_draws_its_seeds():
    from speech_anonymization_amd import ops, sourcefilter
    wav = torch.as_tensor(R.e2e_rows()).to(DEV)
    B, N = wav.shape
    lens = torch.tensor([1.0, 0.75, 1.0], device=DEV)
    sf = sourcefilter.SourceFilter(R.TARGET_HZ, seed=3)
    first = sf(wav, lens)                                    # (warm-up: the library loads)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                  # a device-to-host copy raises from here on
    try:
        second = sf(wav, lens)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert first.shape == second.shape == wav.shape and second.dtype == torch.float32
    assert not torch.equal(first, second)                    # the second batch has seeds of its own
    assert all(v.is_cuda for v in sf.last) and sf.calls == 2 and sf.drawn == 2 * B
    f0, rho_q, count, gain, counts = sf.last
    assert torch.equal(f0, ops.yin_f0(wav))
    ratio = ops.pitch_ratio(f0, lens, N, R.TARGET_HZ)[0]
    assert torch.equal(rho_q, torch.round(ratio.double() * R.ONE).to(torch.int32)[:, None].expand_as(rho_q))
    assert counts.shape == (B, 4) and counts.sum(1).tolist() == [M.n_frames(N)] * B
    assert counts[:, 2].tolist() == [0] * B and int(counts[1, 1]) >= 6              # the cut row's tail is silent
    assert not bool(second[1, 3600:].any()) and bool(second[1, :3600].any())
    # the same object again from the start, and the seeds the restatement names
    other = sourcefilter.SourceFilter(R.TARGET_HZ, seed=3)
    assert torch.equal(other(wav, lens), first) and torch.equal(other(wav, lens), second)
    nv = torch.tensor([N, 3600, N], dtype=torch.int32, device=DEV)
    direct = ops.srcfilt(wav, f0, rho_q, _dev(R.draw_seeds(3, B, B)), nv, 0.3, True)
    assert torch.equal(direct[0], second) and torch.equal(direct[1], gain) and torch.equal(direct[2], count)


@gpu
@pytest.mark.parametrize("target", [None, R.TARGET_HZ], ids=["own_pitch", "170"])
def test_pitch_lands_on_the_target_and_the_envelope_stays(target):
    from speech_anonymization_amd import sourcefilter
    rec = R.load_delta()["e2e"]["own" if target is None else "170"]
    wav = R.e2e_rows()
    B, N = wav.shape
    sf = sourcefilter.SourceFilter(target, seed=R.E2E_SEED)
    out = sf(torch.as_tensor(wav).to(DEV), torch.ones(B, device=DEV)).cpu()
    assert out.shape == wav.shape and bool(torch.isfinite(out).all())
    f0, rho_q, count, gain, counts = (v.cpu() for v in sf.last)
    assert counts[:, 0].tolist() == [M.n_frames(N)] * B and bool((count > 30).all())
    if target is None:
        assert bool((rho_q == R.ONE).all())
    f_rel, peak_hz, f_out, p_in, p_out = R.e2e_measure(wav, out.numpy(), target)
    for b in range(B):
        print(f"row {b}: f0 {f_out[b]:.3f} Hz, rel distance {f_rel[b]:.3e} (recorded worst {rec['f0_rel_worst']:.3e}); "
              f"peak {p_in[b]:.1f} -> {p_out[b]:.1f} Hz (recorded worst {rec['peak_hz_worst']:.1f})")
    assert (f_rel <= 2.0 * rec["f0_rel_worst"]).all()
    assert (peak_hz <= 2.0 * rec["peak_hz_worst"]).all()
    # the level: the RMS over the valid region is the input's (the gain's fp32 rounding and one per output sample)
    rms_in = np.sqrt((wav.astype(np.float64) ** 2).sum(1))
    rms_out = np.sqrt((out.double().numpy() ** 2).sum(1))
    assert (np.abs(rms_out / rms_in - 1.0) <= 1e-6).all()


@gpu
def test_anonymize_resynth_mode_in_a_child(tmp_path):
    out = tmp_path / "resynth"
    res = anon_cli.run_child(["--device", DEV, "--synthetic", "4", "--out_dir", str(out), "--resynth", "true",
                              "--report_f0", "true"])
    assert res["resynth"] is True and res["aspiration"] == 0.3 and res["pitch_target_hz"] is None
    assert "pitch_norm" not in res and "model_type" not in res and "recon_ckpt" not in res and "mcadams" not in res
    assert sorted(os.listdir(out)) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    assert len(res["utterances"]) == 4
    for u in res["utterances"]:
        assert {"id", "samples", "peak", "pulses", "ratio", "gain", "silent_frames", "fallback_frames",
                "unexcited_frames", "f0_mean_hz", "voiced_share"} <= set(u)
        assert u["ratio"] == 1.0 and u["gain"] > 0 and u["fallback_frames"] == 0 and u["pulses"] > 10
        assert 0 < u["peak"] < 4


@gpu
def test_anonymize_resynth_to_a_target(tmp_path, capsys):
    res = anon_cli.run(capsys, ["--device", DEV, "--synthetic", "3", "--batch_size", "3", "--out_dir", str(tmp_path),
                                "--resynth", "true", "--resynth_pitch_hz", "170", "--aspiration", "0.1", "--seed", "5",
                                "--f0_method", "viterbi", "--report_f0", "true", "--report_stoi", "true",
                                "--report_prosody", "true", "--report_mcd", "true", "--report_formants", "true"])
    assert res["resynth"] is True and res["pitch_target_hz"] == 170.0 and res["aspiration"] == 0.1
    assert res["seed"] == 5 and res["f0_method"] == "viterbi"
    for u in res["utterances"]:
        assert 0.5 <= u["ratio"] <= 2.0 and u["ratio"] != 1.0 and u["pulses"] > 10
        assert {"stoi", "f0_corr", "mcd_db", "formant_shift"} <= set(u)


@gpu
def test_recipe_trains_one_epoch(tmp_path):
    """a fresh child process, under a time limit; no error bar: one epoch on 16 synthetic utterances"""
    out = tmp_path / "resynth_recipe"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gender_classifier_train_resynth.py"),
                        os.path.join(ROOT, "speechbrain_configs", "gender_classifier_resynth.yaml"), "--device", DEV,
                        "--output_folder", str(out), "--synthetic", "16", "--number_of_epochs", "1",
                        "--resynth_pitch_hz", "170"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["resynth"] is True and summary["pitch_target_hz"] == 170.0 and summary["aspiration"] == 0.3
    assert 0.0 <= summary["test_error"] <= 1.0
