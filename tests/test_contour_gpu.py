"""GPU checks of the F0-contour pitch modification (csrc/sa_contour.hip and the variants in
sa_phasevoc.hip and sa_envelope.hip; ops.pitch_contour, pv_synth_map, env_warp_frames, pitch_resample_map) against the
restatement tests/contour_ref.py, then PitchNormalizer and the command line with ``contour_scale``.

The tables are integers, so rho_q, Q, T'_b and every index derived from them are compared for EQUALITY: the rows fed
to the contour kernel are ones whose decisions tests/test_contour_cpu.py shows to have a margin.  The synthesis takes
the GPU's own R and magnitudes and keeps section 19's bars ((Tout + 8) 2^-50 turns for phi', 4 u S' for C), the warp
keeps section 16's, the resampling section 15's ((taps + 4) u mass).  u = 2^-24."""
import ctypes
import os

import pytest
import torch

from tests import anon_cli
from tests import contour_ref as Cr
from tests import formant_ref as F
from tests import phasevoc_ref as V
from tests import pitch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = P.U
gpu = pytest.mark.gpu
EINVAL = -22

# tools/contour_delta.py: the fp64 restatement on the glide and the vibrato row (N = 24 000, target 170 Hz), per row.
# The GPU path differs from it by the fp32 rounding of STFT, ISTFT and the resampler's weights and by the fp32
# tracker; as in section 19 the bar is 4 x the restatement's figure.
REF_FIGURES = {("std_in", 0.0): (22.3012, 17.6799),
               ("std_out", 0.0): (0.1393, 1.2787), ("mean_err", 0.0): (0.0622, 0.0079), ("worst", 0.0): (0.4609, 3.5220),
               ("worst", 0.5): (0.4850, 2.1844), ("worst", 1.0): (0.6840, 3.9775)}
MARGIN = 4.0
STEADY_BAR_HZ = 4.0 * 0.0210              # section 19's PV_BAR_HZ
# tools/contour_delta.py --preserve_formants (tests/test_contour_cpu.py recomputes both): the glide row at gamma 0 with
# beta = 1 keeps this F0 standard deviation and displaces its cepstral-envelope peak by this much, in Hz
REF_PRESERVE_STD, REF_PRESERVE_MOVE = 0.159, 37.35


def _f(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lib():
    from speech_anonymization_amd import _lib as L
    return L.load(), L


def _tables(rho_q):
    """rho_q int64 [B, T] on the host -> (rho_q int32, Q int64) on the device, and the host's (rho_q, Q, Tq)"""
    rho_q = torch.as_tensor(rho_q, dtype=torch.int64)
    Q, Tq = Cr.time_map(rho_q)
    return rho_q.to(torch.int32).to(DEV), Q.to(DEV), (rho_q, Q, Tq)


def _const_rho(ratios, T):
    return torch.tensor([[int(round(r * Cr.RHO_ONE))] * T for r in ratios], dtype=torch.int64)


@gpu
def test_dims():
    lib, _ = _lib()
    W, smax, hop, rb, qb, tile, span = (lib.sa_contour_dim(i) for i in range(7))
    assert W >= 64 and W % 64 == 0 and (smax, hop, rb, qb) == (8, 160, 16, 17)
    assert tile >= 64 and span >= 2 * tile + 64
    assert lib.sa_contour_dim(7) == EINVAL and lib.sa_contour_dim(-1) == EINVAL


# ---------------------------------------------------------------------------------------------------
# sa_pitch_contour
# ---------------------------------------------------------------------------------------------------
def _contour_case(shape):
    if shape == "T2":
        return Cr.contour_rows_T2() + (1,)
    return Cr.contour_rows(_lib()[0].sa_contour_dim(0)) + (5,)


@gpu
@pytest.mark.parametrize("shape", ["passes", "T2"])
@pytest.mark.parametrize("call", range(len(Cr.CONTOUR_CALLS)))
def test_contour_against_the_restatement(shape, call):
    from speech_anonymization_amd import ops
    f0, lens, N, min_voiced = _contour_case(shape)
    gamma, s, r_min, r_max = Cr.CONTOUR_CALLS[call]
    ref = Cr.contour(f0, lens, N, 170.0, gamma, s, r_min, r_max, min_voiced)
    rho_q, Q, Tq, mean, voiced = ops.pitch_contour(f0.to(DEV), lens.to(DEV), N, 170.0, gamma, s, r_min, r_max,
                                                   min_voiced)
    assert rho_q.dtype == torch.int32 and Q.dtype == torch.int64 and Tq.dtype == torch.int32
    assert rho_q.shape == Q.shape == f0.shape
    rho_q, Q, Tq = rho_q.cpu().long(), Q.cpu(), Tq.cpu().long()
    wrong = (rho_q != ref.rho_q)
    print(f"{shape} gamma {gamma:g} smooth {s}: {int(wrong.sum())} of {wrong.numel()} rho_q differ; T' {Tq.tolist()}; "
          f"rho_q in [{int(rho_q.min())}, {int(rho_q.max())}]")
    assert torch.equal(voiced.cpu().long(), ref.voiced)
    assert torch.equal(rho_q, ref.rho_q)
    own_Q, own_Tq = Cr.time_map(rho_q)
    assert torch.equal(Q, own_Q) and torch.equal(Tq, own_Tq) and torch.equal(Tq, ref.Tq)
    m = mean.cpu().double()
    assert bool(((m - ref.mean).abs() <= 2 * U * ref.mean).all())            # sa_pitch_ratio's bar
    _, r_mean, r_voiced = ops.pitch_ratio(f0.to(DEV), lens.to(DEV), N, 170.0, min_voiced=min_voiced)
    assert torch.equal(r_mean, mean) and torch.equal(r_voiced, voiced)       # one text: sa_pitch_ratio's bits
    assert bool((rho_q[~ref.moved] == Cr.RHO_ONE).all())
    if shape == "passes":
        assert ref.moved.tolist() == [True, True, False, False, True, True, True, True]
        assert int(ref.voiced[4]) < int((f0[4] > 0).sum()) and int(ref.voiced[3]) == 0 and int(ref.voiced[2]) == 3


# ---------------------------------------------------------------------------------------------------
# sa_pv_synth_map
# ---------------------------------------------------------------------------------------------------
def _signal_rows(N):
    """fp32 [4, N]: a glide, a vibrato, a steady 170 Hz row, a 230 Hz row whose middle third is zero"""
    g = torch.Generator().manual_seed(2009)
    rows = [Cr.glide_row(lambda t: Cr.glide_f0(t, N), N, g), Cr.glide_row(Cr.vibrato_f0, N, g),
            P.harmonic_row(170.0, N, g), P.harmonic_row(230.0, N, g)]
    rows[3][N // 3:2 * N // 3] = 0.0
    return torch.stack(rows).float()


def _map_rows(T):
    """rho_q int64 [4, T]: a glide contour's ratios (170 / (110 .. 190)), a vibrato's, a constant 1.37, ones"""
    t = torch.arange(T, dtype=torch.float64)
    glide = 170.0 / (110.0 + 80.0 * t / max(T - 1, 1))
    vib = 170.0 / (150.0 + 25.0 * torch.sin(2 * torch.pi * t / 33.0 + 0.4))
    rows = [glide, vib, torch.full((T,), 1.37, dtype=torch.float64), torch.ones(T, dtype=torch.float64)]
    return torch.stack([torch.round(r * Cr.RHO_ONE).long() for r in rows])


@pytest.fixture(scope="module", params=["chunks", "T5"])
def synth(request):
    """(R, |R| as the kernels form it, device tables, host tables, Tout, restatement, GPU (C, phi')): computed once per
    shape and left unchanged.  "chunks": T_p = Tc + 17; "T5": N = 500, a single partial chunk"""
    from speech_anonymization_amd import ops, vocoder
    Tc = _lib()[0].sa_pv_dim(3)
    N = (Tc + 16) * 160 if request.param == "chunks" else 500
    wav = _signal_rows(N)
    Np = 160 * -(-N // 160)
    R = vocoder.stft(torch.nn.functional.pad(wav, (0, Np - N)).to(DEV).contiguous())
    T = R.shape[1]
    assert T == (Tc + 17 if request.param == "chunks" else 5)
    rq, Q, host = _tables(_map_rows(T))
    Tout = int(host[2].max())
    mag = ops.pitch_stretch_mag(R, torch.ones(4, device=DEV), T)            # |R|, bit for bit what the kernels form
    C, phi = ops.pv_synth_map(R, rq, Q, Tout, return_phase=True)
    torch.cuda.synchronize()
    ref = Cr.pv_synth_map(R.cpu(), host[0], host[1], mag.cpu(), fp32=True)
    return R, mag, (rq, Q), host, Tout, ref, (C.cpu(), phi.cpu())


@gpu
def test_map_phase_and_spectrum_against_fp64(synth):
    R, _, _, host, Tout, (C_ref, phi_ref, Sp, Tb), (C, phi) = synth
    assert Tb == host[2].tolist() and C.shape == C_ref.shape == (4, Tout, 201) and phi.dtype == torch.float64
    if R.shape[1] > 5:
        assert bool((R.cpu()[3, R.shape[1] // 2] == 0).all())              # the zeroed middle: R exactly 0
    bar = (Tout + 8) * 2.0 ** -50
    d = V.circular(phi, phi_ref)
    er, ei = (C.real.double() - C_ref.real).abs(), (C.imag.double() - C_ref.imag).abs()
    pos = Sp > 0
    print(f"T'_b {Tb}: max circular |phi' - ref| = {float(d.max()):.3e} turns, bar {bar:.3e}; max |C - ref| / (u S') = "
          f"{float((torch.maximum(er, ei)[pos] / (U * Sp[pos])).max()):.3f} (bar 4)")
    assert bool((phi >= 0).all()) and bool((phi <= 1).all()) and bool((d <= bar).all())
    assert bool((er <= 4 * U * Sp).all()) and bool((ei <= 4 * U * Sp).all())
    for b in range(4):
        assert bool((C[b, Tb[b]:] == 0).all()) and bool((phi[b, Tb[b]:] == 0).all())
    assert len(set(Tb)) > 1 and bool((C[0].abs() > 0).any())


@gpu
def test_map_at_constant_ratios_is_pv_synth_bit_for_bit(synth):
    from speech_anonymization_amd import ops
    R = synth[0]
    T = R.shape[1]
    ratios = (0.5, 1.0, 1.25, 2.0)
    rq, Q, host = _tables(_const_rho(ratios, T))
    Tout = int(host[2].max())
    assert host[2].tolist() == [P.stretched_frames(T, r) for r in ratios]
    C, phi = ops.pv_synth_map(R, rq, Q, Tout, return_phase=True)
    C0, phi0 = ops.pv_synth(R, torch.tensor(ratios, dtype=torch.float32, device=DEV), Tout, return_phase=True)
    assert torch.equal(C, C0) and torch.equal(phi, phi0)


@gpu
def test_map_with_magnitudes_keeps_the_phase(synth):
    from speech_anonymization_amd import ops
    R, mag, (rq, Q), host, Tout, _, (C, phi) = synth
    M = ops.env_warp_frames(mag, (rq.float() / (Cr.RHO_ONE * 1.15)).contiguous())
    Cm, phim = ops.pv_synth_map(R, rq, Q, Tout, M=M, return_phase=True)
    assert torch.equal(phim.cpu(), phi) and not torch.equal(Cm.cpu(), C)
    want = Cr.pv_synth_map(R.cpu(), host[0], host[1], M.cpu(), fp32=True)
    bar = 4 * U * want[2]
    Cm = Cm.cpu()
    assert bool(((Cm.real.double() - want[0].real).abs() <= bar).all())
    assert bool(((Cm.imag.double() - want[0].imag).abs() <= bar).all())
    assert bool(((Cm.abs().double() - want[2]).abs() <= bar).all())        # and the magnitude is M's
    Cn = ops.pv_synth_map(R, rq, Q, Tout, M=mag)                           # M = |R| given: the bits of M = NULL
    assert torch.equal(Cn.cpu(), C)
    short = ops.pv_synth_map(R, rq, Q, Tout - 1)                           # a smaller Tout truncates
    assert torch.equal(short.cpu(), C[:, :Tout - 1])


# ---------------------------------------------------------------------------------------------------
# sa_env_warp_frames
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", range(len(F.GPU_CASES)))
def test_frames_warp_at_a_constant_factor_is_env_warp_bit_for_bit(c):
    from speech_anonymization_amd import ops
    B, T, q, zero_row = F.GPU_CASES[c]
    S, q = F.kernel_case(B, T, zero_row).to(DEV), torch.tensor(q, dtype=torch.float32, device=DEV)
    for n_c in (1, 30, 64):
        want = ops.env_warp(S, q, n_c, return_env=True)
        got = ops.env_warp_frames(S, q[:, None].expand(B, T).contiguous(), n_c, return_env=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@gpu
def test_frames_warp_against_fp64():
    """T = 8 + 3 frames, so that the second tile is partial; a factor per frame from {0.25 .. 4}, 1 among them"""
    from speech_anonymization_amd import ops
    B, T = 2, 11
    S = F.kernel_case(B, T)
    pool = torch.tensor([0.25, 0.5, 0.8, 1.0, 1.37, 2.0, 4.0])
    q = pool[torch.randint(0, 7, (B, T), generator=torch.Generator().manual_seed(5))]
    q[0, 3], q[1, 9] = 1.0, 1.0
    ref = Cr.env_warp_frames(S, q)
    out, env = ops.env_warp_frames(S.to(DEV), q.to(DEV), return_env=True)
    out, env = out.cpu().reshape(B * T, 1, 201), env.cpu().reshape(B * T, 1, 201)
    assert bool(torch.isfinite(out).all())
    assert bool(((env.double() - ref.env).abs() <= ref.env_bar).all())
    keep = ~ref.unstable
    assert int(ref.unstable.sum()) <= 0.01 * keep.numel()
    err, bar = (out.double() - ref.out).abs(), ref.out_bar * ref.out
    pos = keep & (ref.out > 0)
    print(f"worst err / bar {float((err[pos] / bar[pos]).max()):.4f}, {int(ref.unstable.sum())} left out")
    assert bool((err[keep] <= bar[keep]).all())
    S2 = S.reshape(B * T, 1, 201)
    assert bool((out[S2 == 0] == 0).all())
    assert torch.equal(out[3], S2[3]) and torch.equal(out[T + 9], S2[T + 9])          # q = 1: copied bit for bit
    assert not torch.equal(out[4], S2[4])


# ---------------------------------------------------------------------------------------------------
# sa_pitch_resample_map
# ---------------------------------------------------------------------------------------------------
def _resample_case():
    """test_resample_against_fp64's shapes: N_in = 7 * 160, N_out = 560 (T = 5), 3 workgroups.  Rows 0..3 constant
    ratios 0.5, 1, 1.37, 2 as in that test, row 4 a glide of the ratio from 0.6 to 1.9, row 5 from 2 to 0.5"""
    g = torch.Generator().manual_seed(13)
    Nin, Nout, T = 7 * 160, 560, 5
    y = torch.randn(6, Nin, generator=g)
    t = torch.arange(T, dtype=torch.float64)
    rho = torch.cat([_const_rho((0.5, 1.0, 1.37, 2.0), T),
                     torch.round((0.6 + 1.3 * t / (T - 1)) * Cr.RHO_ONE).long()[None],
                     torch.round((2.0 - 1.5 * t / (T - 1)) * Cr.RHO_ONE).long()[None]])
    nv = torch.tensor([560, 560, 400, 560, 560, 333], dtype=torch.int32)
    return y, rho, nv, Nin, Nout


@gpu
def test_resample_map_against_fp64():
    from speech_anonymization_amd import ops
    y, rho, nv, Nin, Nout = _resample_case()
    rq, Q, host = _tables(rho)
    ref, mass, taps = Cr.resample_map(y.double(), host[0], host[1], nv.tolist(), Nout)
    assert [(int(t) - 1) * 160 for t in host[2][:4]] == [320, 640, 960, 1280]            # rows 0..2 end inside N_in
    assert 60 <= int(taps.max()) <= 64 and int(taps[0].max()) == 32 and int(taps[3, 0]) == 32
    assert int(taps[0, 0]) < 32 and int(taps[3, -1]) < 64                                 # taps that leave the input
    out = ops.pitch_resample_map(y.to(DEV), rq, Q, nv.to(DEV), Nout).cpu().double()
    assert out.shape == (6, Nout)
    bound = (taps + 4).double() * U * mass
    print(f"max |out - ref| / bound = {float(((out - ref).abs() / bound.clamp(min=1e-300)).max()):.3f}; "
          f"max |out - ref| = {float((out - ref).abs().max()):.3e}")
    assert bool(((out - ref).abs() <= bound).all())
    assert bool((out[2, 400:] == 0).all()) and bool(out[2, 399] != 0)
    assert bool((out[5, 333:] == 0).all()) and bool(out[5, 332] != 0)
    assert float((out[1] - y[1, :Nout].double()).abs().max()) <= 4 * U * float(y.abs().max())   # ratio 1 copies
    # at ratios that are multiples of 2^-16 the map's positions are n r exactly: sa_pitch_resample meets the same
    # reference inside the same bound
    r32 = torch.tensor([0.5, 1.0, 1.25, 2.0], dtype=torch.float32)
    rq2, Q2, host2 = _tables(_const_rho(r32.tolist(), 5))
    y4, nv4 = y[:4].contiguous(), nv[:4].contiguous()
    ref2, mass2, taps2 = Cr.resample_map(y4.double(), host2[0], host2[1], nv4.tolist(), Nout)
    bound2 = (taps2 + 4).double() * U * mass2
    old = ops.pitch_resample(y4.to(DEV), r32.to(DEV), nv4.to(DEV), Nout).cpu().double()
    new = ops.pitch_resample_map(y4.to(DEV), rq2, Q2, nv4.to(DEV), Nout).cpu().double()
    assert bool(((new - ref2).abs() <= bound2).all()) and bool(((old - ref2).abs() <= bound2).all())
    # ... and the same bits: n r, the taps and the input's end are exact and equal in both, so every weight is formed
    # from the same fp64 values and added in the same order
    assert torch.equal(old, new)


# ---------------------------------------------------------------------------------------------------
# the raw ABI: poisoned outputs, refusals by arguments only, two runs
# ---------------------------------------------------------------------------------------------------
NAN = float("nan")


def _poison(shape, dtype):
    if dtype.is_complex:
        return torch.view_as_complex(torch.full(tuple(shape) + (2,), NAN, dtype=torch.float32, device=DEV))
    if dtype.is_floating_point:
        return torch.full(shape, NAN, dtype=dtype, device=DEV)
    return torch.full(shape, -7, dtype=dtype, device=DEV)


def _untouched(*ts):
    return all(bool(torch.isnan(torch.view_as_real(t) if t.is_complex() else t).all()) if
               (t.dtype.is_floating_point or t.dtype.is_complex) else bool((t == -7).all()) for t in ts)


@gpu
def test_contour_entry_point_poison_and_refusals():
    lib, L = _lib()
    W = lib.sa_contour_dim(0)
    f0, lens, N = Cr.contour_rows(W)
    B, T = f0.shape
    f0d, ld = f0.to(DEV), lens.to(DEV)
    ref = Cr.contour(f0, lens, N, 170.0, 0.5, 2)
    fl = ctypes.c_float

    def run(f0_=f0d, lens_=ld, B_=B, T_=T, N_=N, target=170.0, gamma=0.5, s=2, r_min=0.5, r_max=2.0, drop=None):
        outs = [_poison((B, T), torch.int32), _poison((B, T), torch.int64), _poison((B,), torch.int32),
                _poison((B,), torch.float32), _poison((B,), torch.int32)]
        ptrs = [None if drop == i else _f(o) for i, o in enumerate(outs)]
        rc = lib.sa_pitch_contour(_f(f0_), _f(lens_), B_, T_, N_, fl(target), fl(gamma), s, fl(r_min), fl(r_max), 5,
                                  *ptrs, L.stream())
        torch.cuda.synchronize()
        return rc, outs

    rc, a = run()
    assert rc == 0 and torch.equal(a[0].cpu().long(), ref.rho_q) and torch.equal(a[1].cpu(), ref.Q)
    assert torch.equal(a[2].cpu().long(), ref.Tq) and torch.equal(a[4].cpu().long(), ref.voiced)
    assert bool(torch.isfinite(a[3]).all())
    rc, b = run()
    assert rc == 0 and all(torch.equal(x, y) for x, y in zip(a, b))        # two runs, the same bits
    bad = [dict(f0_=None), dict(lens_=None), dict(B_=0), dict(B_=65536), dict(T_=1), dict(T_=(1 << 23) + 1),
           dict(N_=0), dict(N_=(1 << 30) + 1), dict(target=0.0), dict(gamma=-0.01), dict(gamma=2.01), dict(gamma=NAN),
           dict(s=-1), dict(s=9), dict(r_min=0.49), dict(r_max=2.01), dict(r_min=1.5, r_max=1.2)]
    bad += [dict(drop=i) for i in range(5)]
    for kw in bad:
        rc, outs = run(**kw)
        assert rc == EINVAL, kw
        assert _untouched(*outs), kw


@gpu
def test_synth_map_entry_point_poison_and_refusals(synth):
    lib, L = _lib()
    R, mag, (rq, Q), _, Tout, _, (C, phi) = synth
    B, T = R.shape[:2]

    def run(R_=R, M_=None, rq_=rq, Q_=Q, B_=B, T_=T, Tout_=Tout, ws_ok=True, c_ok=True, want_phase=True):
        Cx, ph = _poison((B, Tout, 201), torch.complex64), _poison((B, Tout, 201), torch.float64)
        ws = _poison((lib.sa_pv_workspace_bytes(B, Tout) // 8,), torch.float64)
        rc = lib.sa_pv_synth_map(_f(R_), _f(M_), _f(rq_), _f(Q_), B_, T_, Tout_, _f(Cx if c_ok else None),
                                 _f(ph if want_phase else None), _f(ws if ws_ok else None), L.stream())
        torch.cuda.synchronize()
        return rc, Cx, ph

    rc, C1, ph1 = run()
    assert rc == 0 and torch.equal(C1.cpu(), C) and torch.equal(ph1.cpu(), phi)   # (a NaN left anywhere is unequal)
    rc, C2, ph2 = run()
    assert rc == 0 and torch.equal(C2, C1) and torch.equal(ph2, ph1)
    rc, C3, ph3 = run(M_=mag, want_phase=False)
    assert rc == 0 and torch.equal(C3, C1) and _untouched(ph3)
    for kw in (dict(R_=None), dict(rq_=None), dict(Q_=None), dict(B_=0), dict(B_=65536), dict(T_=1),
               dict(T_=(1 << 23) + 1), dict(Tout_=0), dict(Tout_=(1 << 23) + 1), dict(ws_ok=False), dict(c_ok=False)):
        rc, Cx, ph = run(**kw)
        assert rc == EINVAL, kw
        assert _untouched(Cx, ph), kw


@gpu
def test_frames_warp_entry_point_poison_and_refusals():
    lib, L = _lib()
    from speech_anonymization_amd import ops
    B, T = 2, 11
    S = F.kernel_case(B, T).to(DEV)
    q = torch.linspace(0.5, 2.0, B * T).reshape(B, T).contiguous().to(DEV)
    fl = ctypes.c_float

    def run(S_=S, q_=q, B_=B, T_=T, n_c=30, floor_rel=1e-4, lim=4.6, out_ok=True, env_ok=True):
        out, env = _poison((B, T, 201), torch.float32), _poison((B, T, 201), torch.float32)
        rc = lib.sa_env_warp_frames(_f(S_), _f(q_), B_, T_, n_c, fl(floor_rel), fl(lim), _f(out if out_ok else None),
                                    _f(env if env_ok else None), L.stream())
        torch.cuda.synchronize()
        return rc, out, env

    rc, o1, e1 = run(lim=F.gain_limit(40.0))
    want = ops.env_warp_frames(S, q, return_env=True)
    assert rc == 0 and torch.equal(o1, want[0]) and torch.equal(e1, want[1])
    rc, o2, e2 = run(lim=F.gain_limit(40.0), env_ok=False)
    assert rc == 0 and torch.equal(o2, o1) and _untouched(e2)
    odd = q.clone()
    odd[0, 0], odd[0, 1], odd[1, 2] = 9.0, 0.1, NAN                          # read as 4, 0.25, 1
    fix = q.clone()
    fix[0, 0], fix[0, 1], fix[1, 2] = 4.0, 0.25, 1.0
    assert torch.equal(run(q_=odd)[1], run(q_=fix)[1])
    for kw in (dict(S_=None), dict(q_=None), dict(out_ok=False), dict(B_=0), dict(B_=65536), dict(T_=0),
               dict(T_=(1 << 23) + 1), dict(n_c=0), dict(n_c=65), dict(floor_rel=0.0), dict(floor_rel=1.0),
               dict(lim=0.0)):
        rc, out, env = run(**kw)
        assert rc == EINVAL, kw
        assert _untouched(out, env), kw


@gpu
def test_resample_map_entry_point_poison_and_refusals():
    lib, L = _lib()
    from speech_anonymization_amd import ops
    y, rho, nv, Nin, Nout = _resample_case()
    rq, Q, _ = _tables(rho)
    yd, nvd = y.to(DEV), nv.to(DEV)
    B, T = rho.shape

    def run(y_=yd, rq_=rq, Q_=Q, nv_=nvd, B_=B, Nin_=Nin, Nout_=Nout, T_=T, out_ok=True):
        out = _poison((B, Nout), torch.float32)
        rc = lib.sa_pitch_resample_map(_f(y_), _f(rq_), _f(Q_), _f(nv_), B_, Nin_, Nout_, T_,
                                       _f(out if out_ok else None), L.stream())
        torch.cuda.synchronize()
        return rc, out

    rc, o1 = run()
    assert rc == 0 and torch.equal(o1, ops.pitch_resample_map(yd, rq, Q, nvd, Nout))
    rc, o2 = run()
    assert rc == 0 and torch.equal(o2, o1)
    for kw in (dict(y_=None), dict(rq_=None), dict(Q_=None), dict(nv_=None), dict(out_ok=False), dict(B_=0),
               dict(B_=65536), dict(Nin_=0), dict(Nin_=(1 << 30) + 1), dict(Nout_=0), dict(Nout_=(1 << 29) + 1),
               dict(T_=1), dict(T_=(1 << 23) + 1)):
        rc, out = run(**kw)
        assert rc == EINVAL, kw
        assert _untouched(out), kw


@gpu
def test_bindings_refuse_before_the_library_is_loaded(synth, monkeypatch):
    from speech_anonymization_amd import _lib as L, ops
    R, mag, (rq, Q), _, Tout, _, _ = synth
    B, T = R.shape[:2]
    f0 = torch.full((B, T), 150.0, device=DEV)
    lens = torch.ones(B, device=DEV)
    y = torch.zeros(B, (Tout - 1) * 160, device=DEV)
    nv = torch.full((B,), 100, dtype=torch.int32, device=DEV)
    qf = torch.ones(B, T, device=DEV)

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(L, "load", no_load)
    calls = [lambda: ops.pitch_contour(f0.cpu(), lens, 160 * (T - 1)), lambda: ops.pitch_contour(f0.double(), lens, 1600),
             lambda: ops.pitch_contour(f0.t(), lens, 1600), lambda: ops.pitch_contour(f0, lens[:1], 1600),
             lambda: ops.pitch_contour(f0[:, :1].contiguous(), lens, 1600), lambda: ops.pitch_contour(f0, lens, 0),
             lambda: ops.pitch_contour(f0, lens, 1600, gamma=2.5), lambda: ops.pitch_contour(f0, lens, 1600, gamma=-1),
             lambda: ops.pitch_contour(f0, lens, 1600, smooth=9), lambda: ops.pitch_contour(f0, lens, 1600, r_min=0.4),
             lambda: ops.pitch_contour(f0, lens, 1600, r_max=2.5), lambda: ops.pitch_contour(f0, lens, 1600, target_hz=0),
             lambda: ops.pv_synth_map(R.cpu(), rq, Q, Tout), lambda: ops.pv_synth_map(R, rq.long(), Q, Tout),
             lambda: ops.pv_synth_map(R, rq, Q.int(), Tout), lambda: ops.pv_synth_map(R, rq[:, :-1].contiguous(), Q, Tout),
             lambda: ops.pv_synth_map(R, rq, Q.cpu(), Tout), lambda: ops.pv_synth_map(R, rq, Q, 0),
             lambda: ops.pv_synth_map(R, rq, Q, Tout, M=mag.double()), lambda: ops.pv_synth_map(R, rq, Q, Tout, M=mag[:, :-1]),
             lambda: ops.pv_synth_map(R[:, :, :200].contiguous(), rq, Q, Tout),
             lambda: ops.pv_synth_map(R.transpose(0, 1), rq, Q, Tout),
             lambda: ops.env_warp_frames(mag.cpu(), qf), lambda: ops.env_warp_frames(mag, qf[:, 0].contiguous()),
             lambda: ops.env_warp_frames(mag, qf.double()), lambda: ops.env_warp_frames(mag, qf.t()),
             lambda: ops.env_warp_frames(mag, qf, n_c=65), lambda: ops.env_warp_frames(mag[:, :, :200], qf),
             lambda: ops.pitch_resample_map(y.cpu(), rq, Q, nv, 100), lambda: ops.pitch_resample_map(y, rq, Q, nv.long(), 100),
             lambda: ops.pitch_resample_map(y, rq, Q, nv, 0), lambda: ops.pitch_resample_map(y, rq.t(), Q, nv, 100),
             lambda: ops.pitch_resample_map(y, rq[:, :1].contiguous(), Q[:, :1].contiguous(), nv, 100),
             lambda: ops.pitch_resample_map(y.double(), rq, Q, nv, 100)]
    for i, call in enumerate(calls):
        with pytest.raises(L.SaHipError):
            call()
            raise AssertionError(f"call {i} was accepted")


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def _gpu_tracker(w):
    from speech_anonymization_amd import ops
    return ops.yin_f0(w.float().to(DEV).contiguous()).cpu().double()


@pytest.fixture(scope="module")
def figures():
    """contour_ref.delta_cases with PitchNormalizer as the path and ops.yin_f0 as the tracker, gamma 0 and 1 -> (the
    figures, the outputs per gamma)"""
    from speech_anonymization_amd import pitchnorm
    outs = {}

    def path(wav, lens, gamma):
        norm = pitchnorm.PitchNormalizer(170.0, phase="vocoder", contour_scale=gamma)
        outs[gamma] = (norm(wav.to(DEV), lens).cpu(), tuple(t.cpu() for t in norm.last))
        return outs[gamma][0]

    res = Cr.delta_cases(170.0, gammas=(0.0, 1.0), path=path, tracker=_gpu_tracker, report=print)
    return res, outs


@gpu
def test_gamma_zero_flattens_the_contour(figures):
    res, outs = figures
    out, (ratio, mean, voiced) = outs[0.0]
    assert out.shape == (2, Cr.N_CASE) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert bool((voiced >= 140).all()) and bool((mean > 140.0).all()) and bool((mean < 160.0).all())
    assert bool((ratio > 170.0 / 190.0).all()) and bool((ratio < 170.0 / 110.0).all())   # a mean of ratios in that range
    for b in range(2):
        std_in, std_out, err = res[0.0]["std_in"][b], res[0.0]["std_out"][b], res[0.0]["mean_err"][b]
        print(f"row {b}: std {std_in:.3f} -> {std_out:.4f} Hz (restatement {REF_FIGURES[('std_out', 0.0)][b]}), "
              f"|mean - 170| {err:.4f} Hz (restatement {REF_FIGURES[('mean_err', 0.0)][b]})")
        assert std_out <= 0.25 * std_in
        assert std_out <= MARGIN * REF_FIGURES[("std_out", 0.0)][b]
        assert err <= MARGIN * REF_FIGURES[("mean_err", 0.0)][b]
        assert res[0.0]["frames"][b] >= 130


@gpu
def test_gamma_one_is_the_additive_shift(figures):
    res, outs = figures
    for b in range(2):
        worst = res[1.0]["worst"][b]
        print(f"row {b}: worst per-frame |f0_out - (170 + f0_in - mean)| = {worst:.4f} Hz (restatement "
              f"{REF_FIGURES[('worst', 1.0)][b]}), std {res[1.0]['std_in'][b]:.3f} -> {res[1.0]['std_out'][b]:.3f} Hz")
        assert worst <= MARGIN * REF_FIGURES[("worst", 1.0)][b]
        assert res[1.0]["frames"][b] >= 130


@gpu
def test_steady_row_lands_where_the_constant_ratio_path_does():
    from speech_anonymization_amd import ops, pitchnorm
    wav, lens = Cr.steady_row().to(DEV), torch.ones(1)
    N = wav.shape[1]
    a = pitchnorm.PitchNormalizer(170.0, phase="vocoder", contour_scale=1.0)(wav, lens)
    b = pitchnorm.PitchNormalizer(170.0, phase="vocoder")(wav, lens)
    ma, mb = (float(P.voiced_mean(ops.yin_f0(x).cpu().double(), lens, N)[0]) for x in (a, b))
    print(f"steady row: contour path {ma:.4f} Hz, constant-ratio path {mb:.4f} Hz, bar {STEADY_BAR_HZ:.4f} Hz")
    assert abs(ma - mb) <= STEADY_BAR_HZ and abs(ma - 170.0) <= STEADY_BAR_HZ


@gpu
def test_any_seed_gives_the_same_bits(monkeypatch):
    from speech_anonymization_amd import ops, pitchnorm, vocoder
    wav, lens = Cr.case_rows(8000).to(DEV), torch.tensor([1.0, 0.8])

    def never(*a, **k):
        raise AssertionError("the contour path drew phases or took the constant-ratio kernels")

    monkeypatch.setattr(vocoder.GriffinLim, "draw_phase", never)
    for name in ("pitch_ratio", "pv_synth", "pitch_resample", "env_warp"):
        monkeypatch.setattr(ops, name, never)
    a = pitchnorm.PitchNormalizer(170.0, phase="vocoder", contour_scale=0.5, seed=1)(wav, lens)
    b = pitchnorm.PitchNormalizer(170.0, phase="vocoder", contour_scale=0.5, seed=5)(wav, lens)
    assert torch.equal(a, b) and bool((a[1, 6400:] == 0).all()) and bool(a[1, 6399] != 0)
    c = pitchnorm.PitchNormalizer(170.0, phase="vocoder", contour_scale=0.5, formant_ratio=1.1)(wav, lens)
    assert bool(torch.isfinite(c).all()) and not torch.equal(c, a)


@gpu
def test_preserve_formants_with_a_flat_contour():
    """tools/contour_delta.py --preserve_formants: the restatement flattens the glide to a standard deviation of
    0.159 Hz and displaces its envelope peak by 37.35 Hz, inside section 16's bar, so the peak condition is asserted"""
    from speech_anonymization_amd import pitchnorm
    from tests.test_formant_gpu import PRESERVE_PEAK_BAR
    REF_STD, REF_MOVE = REF_PRESERVE_STD, REF_PRESERVE_MOVE
    assert REF_MOVE <= PRESERVE_PEAK_BAR
    wav, lens = Cr.case_rows()[:1], torch.ones(1)
    out = pitchnorm.PitchNormalizer(170.0, phase="vocoder", contour_scale=0.0, preserve_formants=True)(
        wav.to(DEV), lens).cpu()
    _, std_in, _ = Cr.f0_stats(_gpu_tracker(wav), lens, wav.shape[1])
    _, std, _ = Cr.f0_stats(_gpu_tracker(out), lens, wav.shape[1])
    move = float((F.envelope_peak(out) - F.envelope_peak(wav)).abs()[0])
    print(f"preserve_formants, gamma 0: std {float(std_in[0]):.3f} -> {float(std[0]):.4f} Hz (restatement {REF_STD}), "
          f"envelope peak displaced by {move:.2f} Hz (restatement {REF_MOVE}, bar {PRESERVE_PEAK_BAR:.1f})")
    assert float(std[0]) <= 0.25 * float(std_in[0]) and float(std[0]) <= MARGIN * REF_STD
    assert move <= PRESERVE_PEAK_BAR


def _anonymize_child(tmp_path, name, extra):
    out = tmp_path / name
    return out, anon_cli.run_child(["--device", DEV, "--out_dir", str(out), "--pitch_norm", "true", "--phase", "vocoder",
                                    "--synthetic", "4", "--report_f0", "true"] + extra)


@gpu
def test_anonymize_command_line_with_the_contour(tmp_path):
    out, res = _anonymize_child(tmp_path, "flat", ["--contour_scale", "0"])
    print({k: v for k, v in res.items() if k != "utterances"}, res["utterances"][0])
    assert res["contour_scale"] == 0.0 and res["contour_smooth"] == 2 and res["phase"] == "vocoder"
    assert sorted(os.listdir(out)) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    for u in res["utterances"]:
        assert set(u) >= {"id", "samples", "peak", "ratio", "f0_mean_hz", "voiced_share", "f0_std_hz"}
        assert abs(u["f0_mean_hz"] - 170.0) <= 0.5 and 0.0 <= u["f0_std_hz"] < float("inf"), u
        assert u["voiced_share"] >= 0.9 and 0.5 <= u["ratio"] <= 2.0, u
    _, plain = _anonymize_child(tmp_path, "plain", [])
    assert "contour_scale" not in plain and "contour_smooth" not in plain
    assert all("f0_std_hz" not in u for u in plain["utterances"])
