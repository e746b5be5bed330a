"""sa_env_warp (csrc/sa_envelope.hip) against the fp64 restatement of tests/formant_ref.py, then
the two paths that use it and the recipes.  u = 2^-24 is fp32's unit roundoff.

The bars are derived on the restatement's own absolute terms (formant_ref.warp states them in full):

    env:  |E_gpu(w_k) - E(w_k)| <= dE(w_k),
          dE(x) = dc_0 + 2 sum_n dc_n |cos n x| + (n_c + 3) u (|c_0| + 2 sum_n |c_n| |cos n x|) + 64^2 2^-52 2 sum_n |c_n|,
          dc_n = (1 / 400) sum_k w_k (2 LOG_ULP u |L_k| + u) |cos| + (199 + 5) u (1 / 400) sum_k w_k |L_k| |cos|
          -- the two chained dot products, with logf within LOG_ULP = 1 ulp;
    out:  |out_gpu - out| <= (expm1(dg) + (2 EXP_ULP + 2) u) out,  dg = dE(theta_k) + dE(w_k) + u |g|
          -- the image of the gain's bound through exp, with expf within EXP_ULP = 1 ulp.

An element is left out only when its unclamped gain lies within dg of +-limit (there the clamp decision is a coin
toss); the inputs are chosen so that the restatement leaves out none (tests/test_formant_cpu.py checks that first).

End to end the bars are measured on the restatement, never on the code under test: tools/formant_delta.py runs it
over the three resonance rows x 3 phase seeds on the CPU; two Griffin-Lim trajectories that differ by rounding part
ways, so the tests ask twice its figures."""
import ctypes
import errno
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import anon_cli
from tests import formant_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = F.U
gpu = pytest.mark.gpu

# tools/formant_delta.py (fp64, 32 iterations, phase seeds 0..2, target 170 Hz), worst over rows and seeds:
PRESERVE_F0_WORST_HZ = 0.166             # |voiced-mean F0 - 170| with preserve_formants
PRESERVE_PEAK_WORST_HZ = 33.45           # |envelope peak - the input's| with preserve_formants
SHIFT_F0_WORST_HZ = 0.155                # |voiced-mean F0 - the input's|, formant_ratio 0.85 and 1.2
SHIFT_PEAK_WORST_HZ = 153.29             # |envelope peak - beta x the input's|, formant_ratio 0.85 and 1.2
PRESERVE_F0_BAR, PRESERVE_PEAK_BAR = 2.0 * PRESERVE_F0_WORST_HZ, 2.0 * PRESERVE_PEAK_WORST_HZ
SHIFT_F0_BAR, SHIFT_PEAK_BAR = 2.0 * SHIFT_F0_WORST_HZ, 2.0 * SHIFT_PEAK_WORST_HZ


def _f(t):
    return ctypes.c_void_p(t.data_ptr())


def _launch(S, q, n_c, floor_rel=1e-4, max_gain_db=40.0):
    """sa_env_warp through the library itself, into buffers poisoned with NaN -> (out, env) on the CPU in fp64"""
    from speech_anonymization_amd import _lib
    B, T, _ = S.shape
    Sd, qd = S.to(DEV).contiguous(), q.to(DEV).contiguous()
    out = torch.full_like(Sd, float("nan"))
    env = torch.full_like(Sd, float("nan"))
    rc = _lib.load().sa_env_warp(_f(Sd), _f(qd), B, T, n_c, ctypes.c_float(floor_rel),
                                 ctypes.c_float(F.gain_limit(max_gain_db)), _f(out), _f(env), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu(), env.cpu()


# ---------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(c, n_c) for c in range(len(F.GPU_CASES)) for n_c in (1, 30, 64)],
                ids=lambda p: "B%dT%d_nc%d" % (F.GPU_CASES[p[0]][0], F.GPU_CASES[p[0]][1], p[1]))
def case(request):
    """(S, q, n_c, restatement, GPU (out, env)): computed once per case and left unchanged"""
    (B, T, q, zero_row), n_c = F.GPU_CASES[request.param[0]], request.param[1]
    S, q = F.kernel_case(B, T, zero_row), torch.tensor(q, dtype=torch.float32)
    return S, q, n_c, F.warp(S, q, n_c=n_c), _launch(S, q, n_c)


@gpu
def test_envelope_against_fp64(case):
    S, q, n_c, ref, (_, env) = case
    assert env.shape == S.shape and bool(torch.isfinite(env).all())        # every element written over the NaN
    err = (env.double() - ref.env).abs()
    print(f"{tuple(S.shape[:2])} n_c={n_c}: max |env - ref| {float(err.max()):.3e}, smallest bar "
          f"{float(ref.env_bar.min()):.3e}, worst err / bar {float((err / ref.env_bar).max()):.4f}")
    assert bool((err <= ref.env_bar).all())


@gpu
def test_warped_magnitudes_against_fp64(case):
    S, q, n_c, ref, (out, _) = case
    assert out.shape == S.shape and bool(torch.isfinite(out).all())
    keep = ~ref.unstable
    left_out = int(ref.unstable.sum())
    assert left_out <= 0.01 * keep.numel()
    err, bar = (out.double() - ref.out).abs(), ref.out_bar * ref.out
    pos = keep & (ref.out > 0)
    worst = float((err[pos] / bar[pos]).max()) if pos.any() else 0.0
    print(f"{tuple(S.shape[:2])} n_c={n_c}: {left_out} left out, {int((ref.g_raw.abs() > ref.limit).sum())} clamped, "
          f"worst relative err {float((err[pos] / ref.out[pos]).max()) if pos.any() else 0.0:.3e}, worst err / bar {worst:.4f}")
    assert bool((err[keep] <= bar[keep]).all())
    assert bool((out[S == 0] == 0).all())                                  # zeros stay zeros, whatever the gain
    zero_frames = ~S.bool().any(-1)
    assert bool((out[zero_frames] == 0).all())


@gpu
def test_rows_at_q_one_are_copied_bit_for_bit(case):
    S, q, n_c, _, (out, _) = case
    for b in range(S.shape[0]):
        if float(q[b]) == 1.0:
            assert torch.equal(out[b], S[b])
    one = torch.ones(S.shape[0])
    assert torch.equal(_launch(S, one, n_c)[0], S)


@gpu
def test_two_runs_and_the_binding_give_the_same_bits(case):
    from speech_anonymization_amd import ops
    S, q, n_c, _, (out, env) = case
    again = _launch(S, q, n_c)
    assert torch.equal(again[0], out) and torch.equal(again[1], env)
    o, e = ops.env_warp(S.to(DEV), q.to(DEV), n_c, return_env=True)
    assert torch.equal(o.cpu(), out) and torch.equal(e.cpu(), env)
    assert torch.equal(ops.env_warp(S.to(DEV), q.to(DEV), n_c).cpu(), out)  # env NULL: the same out


@gpu
def test_warp_factors_are_bounded_on_the_device():
    """q outside [0.25, 4] is the nearer bound and a NaN is 1, inside the kernel"""
    S = F.kernel_case(3, 9)
    bad = torch.tensor([9.0, 0.1, float("nan")])
    good = torch.tensor([4.0, 0.25, 1.0])
    a, b = _launch(S, bad, 30), _launch(S, good, 30)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0][2], S[2])


@gpu
def test_entry_point_and_binding_refuse():
    from speech_anonymization_amd import _lib, ops
    lib, E = _lib.load(), -errno.EINVAL
    S = torch.ones(2, 9, 201, device=DEV)
    q = torch.ones(2, device=DEV)
    out = torch.empty_like(S)
    f = ctypes.c_float

    def warp(S_=S, q_=q, B=2, T=9, n_c=30, floor_rel=1e-4, lim=4.6, out_=out):
        return lib.sa_env_warp(None if S_ is None else _f(S_), None if q_ is None else _f(q_), B, T, n_c, f(floor_rel),
                               f(lim), None if out_ is None else _f(out_), None, _lib.stream())

    assert warp() == 0
    for bad in (dict(S_=None), dict(q_=None), dict(out_=None), dict(B=0), dict(B=65536), dict(T=0),
                dict(T=(1 << 23) + 1), dict(n_c=0), dict(n_c=65), dict(floor_rel=0.0), dict(floor_rel=1.0),
                dict(lim=0.0), dict(lim=-1.0)):
        assert warp(**bad) == E, bad
    torch.cuda.synchronize()
    for args, kw in (((S.cpu(), q), {}), ((S, q.cpu()), {}), ((S.double(), q), {}), ((S, q.double()), {}),
                     ((S[:, :, :200], q), {}), ((S.transpose(0, 1), q), {}), ((S[:, ::2], q), {}),
                     ((S, torch.ones(3, device=DEV)), {}), ((S, q), dict(n_c=0)), ((S, q), dict(n_c=65)),
                     ((S, q), dict(floor_rel=0.0)), ((S, q), dict(floor_rel=1.0)), ((S, q), dict(max_gain_db=0.0))):
        with pytest.raises(_lib.SaHipError):
            ops.env_warp(*args, **kw)


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    """(wav fp32 [3, 8000], lens, the input's voiced-mean F0 and envelope peak by the restatement)"""
    wav = F.resonance_rows()
    f0, share = F.voiced_f0(wav)
    assert float(share.min()) >= 0.9
    return wav, torch.ones(3), f0, F.envelope_peak(wav)


@gpu
def test_preserve_formants_moves_the_pitch_and_keeps_the_envelope(rows):
    from speech_anonymization_amd import pitchnorm
    wav, lens, f0_in, peak_in = rows
    out = pitchnorm.PitchNormalizer(170.0, preserve_formants=True)(wav.to(DEV), lens)
    assert out.shape == wav.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    f0, share = F.voiced_f0(out.cpu())
    peak = F.envelope_peak(out.cpu())
    plain = pitchnorm.PitchNormalizer(170.0)(wav.to(DEV), lens)
    f0_plain, peak_plain = F.voiced_f0(plain.cpu())[0], F.envelope_peak(plain.cpu())
    print("in    f0", f0_in.tolist(), "peak", peak_in.tolist())
    print("keep  f0", f0.tolist(), "peak", peak.tolist(), "voiced share", share.tolist(),
          f"bars {PRESERVE_F0_BAR:.3f} Hz, {PRESERVE_PEAK_BAR:.1f} Hz")
    print("plain f0", f0_plain.tolist(), "peak", peak_plain.tolist())
    assert bool(((f0 - 170.0).abs() <= PRESERVE_F0_BAR).all())
    assert bool(((peak - peak_in).abs() <= PRESERVE_PEAK_BAR).all())
    assert float(share.min()) >= 0.5
    assert bool(((peak_plain - peak_in).abs() > PRESERVE_PEAK_BAR).all())   # the plain path moves it: the test can tell


@gpu
@pytest.mark.parametrize("beta", [1.2, 0.85])
def test_formant_shifter_moves_the_envelope_and_keeps_the_pitch(rows, beta):
    from speech_anonymization_amd import pitchnorm
    wav, _, f0_in, peak_in = rows
    lens = torch.tensor([1.0, 0.8, 1.0])
    out = pitchnorm.FormantShifter(beta)(wav.to(DEV), lens)
    assert out.shape == wav.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert bool((out[1, 6400:] == 0).all()) and bool(out[1, 6399] != 0) and bool(out[0, -1] != 0)   # the zero tail
    full = pitchnorm.FormantShifter(beta)(wav.to(DEV), torch.ones(3)).cpu()
    assert torch.equal(full[1, :6400], out[1, :6400].cpu())
    f0, share = F.voiced_f0(full)
    peak = F.envelope_peak(full)
    print(f"beta {beta}: f0", f0.tolist(), "in", f0_in.tolist(), "peak", peak.tolist(), "expected",
          (beta * peak_in).tolist(), "voiced share", share.tolist(), f"bars {SHIFT_F0_BAR:.3f} Hz, {SHIFT_PEAK_BAR:.1f} Hz")
    assert bool(((f0 - f0_in).abs() <= SHIFT_F0_BAR).all())
    assert bool(((peak - beta * peak_in).abs() <= SHIFT_PEAK_BAR).all())
    assert float(share.min()) >= 0.5


@gpu
def test_default_normalizer_is_the_plain_composition_bit_for_bit(rows, monkeypatch):
    """PitchNormalizer(170) with the defaults launches no warp and returns the bits of stft -> stretch ->
    Griffin-Lim (same seed) -> resample"""
    from speech_anonymization_amd import ops, pitchnorm, vocoder
    wav, lens, _, _ = rows
    x = wav.to(DEV)
    real = ops.env_warp

    def no_warp(*a, **k):
        raise AssertionError("sa_env_warp was launched")

    monkeypatch.setattr(ops, "env_warp", no_warp)
    norm = pitchnorm.PitchNormalizer(170.0)
    out = norm(x, lens)
    monkeypatch.setattr(ops, "env_warp", real)
    ratio = norm.last[0]
    N = x.shape[1]
    R = vocoder.stft(x)
    Tout = max(pitchnorm.stretched_frames(R.shape[1], r) for r in ratio.cpu().tolist())
    y = vocoder.GriffinLim(n_iter=32, momentum=0.99, seed=1)(ops.pitch_stretch_mag(R, ratio, Tout))
    n_valid = torch.round(lens.to(DEV).double() * N).clamp(0, N).to(torch.int32)
    assert torch.equal(out, ops.pitch_resample(y, ratio, n_valid, N))
    # and with the formants scaled by the pitch ratio itself -- q == 1 on every row -- the warp copies
    one_row = x[:1].contiguous()
    r0 = float(ratio[0])
    same = pitchnorm.PitchNormalizer(170.0, formant_ratio=r0).shift(one_row, lens[:1], ratio[:1].contiguous())
    assert torch.equal(same, pitchnorm.PitchNormalizer(170.0).shift(one_row, lens[:1], ratio[:1].contiguous()))


@gpu
def test_recipe_trains_one_epoch_with_preserved_formants(tmp_path):
    """a fresh child process, under a time limit; no error bar: the synthetic classes differ by pitch only"""
    from speech_anonymization_amd import gender
    out = tmp_path / "pitch_norm_formants"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gender_classifier_train_pitch_norm.py"),
                        os.path.join(ROOT, "speechbrain_configs", "gender_classifier_pitch_norm.yaml"), "--device", DEV,
                        "--output_folder", str(out), "--synthetic", "32", "--number_of_epochs", "1",
                        "--preserve_formants", "true"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["preserve_formants"] is True and res["pitch_target_hz"] == 170.0 and "formant_ratio" not in res
    assert 0.0 <= res["test_error"] <= 1.0
    ck = res["best_checkpoint"]
    assert ck and os.path.isdir(ck)
    clf = gender.load_external_classifier(ck)
    assert not clf.training


def _anonymize(capsys, argv):
    return anon_cli.run(capsys, ["--device", DEV, "--synthetic", "4", "--seed", "3"] + argv)


@gpu
def test_anonymize_formant_modes(tmp_path, capsys):
    from speech_anonymization_amd import data
    out = tmp_path / "shift"
    res = _anonymize(capsys, ["--out_dir", str(out), "--formant_ratio", "1.15", "--report_f0", "true"])
    assert res["formant_shift"] is True and res["formant_ratio"] == 1.15 and res["n_iter"] == 32
    assert "pitch_norm" not in res and "preserve_formants" not in res
    lens = torch.cat([b.sig[1] for b in data.synthetic_gender_dataset(4, 3, seed=3)])
    assert sorted(os.listdir(out)) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    for i, u in enumerate(res["utterances"]):
        sig = data.read_audio(os.path.join(out, u["id"] + ".wav"))
        assert u["id"] == f"synthetic_{i:04d}" and sig.numel() == u["samples"] == int(round(float(lens[i]) * 16000))
        assert u["peak"] > 0.0 and 60.0 <= u["f0_mean_hz"] <= 400.0 and 0.0 < u["voiced_share"] <= 1.0, u
    keep = tmp_path / "keep"
    res = _anonymize(capsys, ["--out_dir", str(keep), "--pitch_norm", "true", "--preserve_formants", "true",
                              "--report_f0", "true"])
    assert res["pitch_norm"] is True and res["preserve_formants"] is True and res["pitch_target_hz"] == 170.0
    assert sorted(os.listdir(keep)) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    for u in res["utterances"]:
        assert set(u) >= {"id", "samples", "peak", "ratio", "f0_mean_hz", "voiced_share"} and 0.5 <= u["ratio"] <= 2.0
