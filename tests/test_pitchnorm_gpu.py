"""The pitch-normalisation kernels (csrc/sa_pitch.hip) against the fp64 restatement of
tests/pitch_ref.py, then the whole path and the recipe.  u = 2^-24 is fp32's unit roundoff.

sa_yin_f0's decisions are comparisons of rounded numbers, so they are compared where the reference's own decision
is not a coin toss: pitch_ref.stable marks the frames on which no scaling of the d' by factors within 1 +- eps --
eps = (W + tau_max + 8) u, the bound on d' itself -- changes the verdict on any lag up to the pick, and whose
interpolation denominator is at least 64 eps (a + 2 c + e).  At most 5 % of the frames may be left out that way."""
import importlib.util
import json
import math
import os

import pytest
import torch

from tests import anon_cli
from tests import pitch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = P.U
gpu = pytest.mark.gpu

# tools/pitch_norm_delta.py: the fp64 restatement over 16 utterances of synthetic_gender_dataset x 3 phase seeds, 32
# iterations, target 170 Hz, ends at most 5.323 Hz from the target (voiced share at least 0.697).  Two Griffin-Lim
# trajectories that differ by rounding part ways (tools/vocoder_delta.py), so the bar is twice that.
DELTA_WORST_HZ = 5.323
BAR_HZ = 2.0 * DELTA_WORST_HZ
RATIOS = (0.5, 1.0, 1.37, 2.0)


def _ratios():
    r32 = torch.tensor(RATIOS, dtype=torch.float32)
    return r32, r32.double().tolist()


# ---------------------------------------------------------------------------------------------------
# sa_yin_f0
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[160 * 19 + 37, 500], ids=["T20", "T4_all_padding"])
def yin_case(request):
    """(N, reference (f0, d', p), GPU (f0, d')): computed once per shape and left unchanged"""
    from speech_anonymization_amd import ops
    N = request.param
    x = P.yin_case(N)
    ref = P.yin(x)
    f0, dp = ops.yin_f0(x.to(DEV), 0.15, return_dprime=True)
    torch.cuda.synchronize()
    return N, ref, (f0.cpu().double(), dp.cpu().double())


@gpu
def test_yin_dprime_against_fp64(yin_case):
    N, (_, dp, _), (f0g, dpg) = yin_case
    T = N // 160 + 1
    assert f0g.shape == (5, T) and dpg.shape == (5, T, 267)
    rel = ((dpg - dp).abs() / dp.clamp(min=1e-300)).max()
    print(f"N={N}: max relative |d' - ref| = {float(rel):.3e}, bound {P.EPS_DPRIME:.3e}")
    assert bool(((dpg - dp).abs() <= P.EPS_DPRIME * dp).all())
    assert bool((dpg[..., 0] == 1.0).all())


@gpu
def test_yin_decisions_and_f0_on_stable_frames(yin_case):
    N, (f0, dp, p), (f0g, dpg) = yin_case
    st = P.stable(dp, p)
    left_out = int((~st).sum())
    voiced = p > 0
    print(f"N={N}: {left_out} of {st.numel()} frames left out as unstable; {int(voiced.sum())} voiced")
    assert left_out <= 0.05 * st.numel()
    assert bool((((f0g > 0) == voiced) | ~st).all())
    assert bool(((P.yin_pick(dpg) == p) | ~st).all())                      # the lag its own d' leads to
    sv = st & voiced
    err, bound = (f0g - f0).abs(), 2.0 * P.f0_bound(dp, p)
    if sv.any():
        print(f"N={N}: max |f0 - ref| on stable voiced frames {float(err[sv].max()):.3e} Hz; smallest bound "
              f"{float(bound[sv].min()):.3e}, worst err / bound {float((err[sv] / bound[sv]).max()):.3e}")
    assert bool((err[sv] <= bound[sv]).all())
    if N > 3000:
        assert int(voiced[0].sum()) >= 10 and int(voiced[1].sum()) >= 10 and int(voiced[2].sum()) >= 8
        assert abs(float(f0g[0][voiced[0]].median()) - 62.0) < 0.5
        assert abs(float(f0g[1][voiced[1]].median()) - 395.0) < 0.5
        assert not f0g[2, 14:].any()                                       # the zeroed tail from 0.6 N
    assert not voiced[3].any() and not voiced[4].any()                     # noise and silence


@gpu
def test_yin_silence_is_exactly_unvoiced(yin_case):
    _, _, (f0g, dpg) = yin_case
    assert bool((f0g[4] == 0).all()) and bool((dpg[4] == 1.0).all())


@gpu
def test_yin_without_dprime_gives_the_same_bits(yin_case):
    from speech_anonymization_amd import ops, pitchnorm
    N, _, (f0g, _) = yin_case
    x = P.yin_case(N).to(DEV)
    a, b = ops.yin_f0(x), pitchnorm.f0_track(x)
    assert torch.equal(a, b) and torch.equal(a.cpu().double(), f0g)


# ---------------------------------------------------------------------------------------------------
# sa_pitch_ratio, sa_pitch_stretch_mag, sa_pitch_resample
# ---------------------------------------------------------------------------------------------------
@gpu
def test_ratio_against_fp64():
    """B = 4, T = 20: the two clamps, a row under min_voiced, lens that cut frames off (what lies past the cut would
    change the mean), and one more call whose ratios fall inside the bounds"""
    from speech_anonymization_amd import ops
    N = 160 * 19 + 37
    g = torch.Generator().manual_seed(7)
    f0 = torch.zeros(4, 20)
    f0[0, 2:14] = 60.0 + torch.rand(12, generator=g)                       # -> r_max
    f0[1, :] = 390.0 + torch.rand(20, generator=g)                         # -> r_min
    f0[2, 5:9] = 150.0                                                     # 4 voiced < 5 -> 1
    f0[3, :] = 120.0 + 80.0 * torch.rand(20, generator=g)
    f0[3, 4] = 0.0
    f0[3, 12:] = 300.0                                                     # past the cut: 11 frames count
    lens = torch.tensor([1.0, 1.0, 1.0, 0.53])
    for kw in ({}, {"target_hz": 200.0, "r_min": 0.6, "r_max": 1.9, "min_voiced": 3}):
        ref_r, ref_m, ref_v = P.ratio(f0, lens, N, **kw)
        r, m, v = ops.pitch_ratio(f0.to(DEV), lens.to(DEV), N, **kw)
        r, m, v = r.cpu().double(), m.cpu().double(), v.cpu().long()
        print("ratio", r.tolist(), "ref", ref_r.tolist(), "voiced", v.tolist())
        assert torch.equal(v, ref_v) and v.tolist() == [12, 20, 4, 10]
        assert bool(((r - ref_r).abs() <= 2 * U * ref_r).all())
        assert bool(((m - ref_m).abs() <= 2 * U * ref_m).all())
    assert ref_r.tolist()[:2] == [1.9, 0.6] and 0.6 < float(ref_r[3]) < 1.9 and float(ref_r[2]) == 200.0 / 150.0
    r = ops.pitch_ratio(f0.to(DEV), lens.to(DEV), N)[0].cpu().tolist()
    assert r[:3] == [2.0, 0.5, 1.0]


@gpu
def test_stretch_mag_against_fp64():
    from speech_anonymization_amd import ops
    g = torch.Generator().manual_seed(11)
    R = torch.complex(torch.randn(4, 11, 201, generator=g), torch.randn(4, 11, 201, generator=g))
    r32, r = _ratios()
    ref, nb, Tb = P.stretch(R.to(torch.complex128).abs(), r)
    assert Tb == [6, 11, 15, 21]
    S = ops.pitch_stretch_mag(R.to(DEV), r32.to(DEV), max(Tb)).cpu().double()
    assert S.shape == ref.shape == (4, 21, 201)
    print(f"max |S - ref| / (8 u (|R_i| + |R_i+1|)) = {float(((S - ref).abs() / (8 * U * nb).clamp(min=1e-300)).max()):.3f}")
    assert bool(((S - ref).abs() <= 8 * U * nb).all())
    for b in range(4):
        assert bool((S[b, Tb[b]:] == 0).all()) and bool((S[b, :Tb[b]] > 0).all())
    short = ops.pitch_stretch_mag(R.to(DEV), r32.to(DEV), 9).cpu().double()      # a smaller Tout truncates
    assert torch.equal(short, S[:, :9])


@gpu
def test_resample_against_fp64():
    """N_in = 7 * 160, N_out = 560: outputs 0..63 and the last 64 have taps that leave the input, rows 0..2 have an
    input shorter than N_in (the stretched length of their ratio), row 2 ends at n_b = 400 < N_out; 3 workgroups"""
    from speech_anonymization_amd import ops
    g = torch.Generator().manual_seed(13)
    Nin, Nout = 7 * 160, 560
    y = torch.randn(4, Nin, generator=g)
    r32, r = _ratios()
    nv = torch.tensor([560, 560, 400, 560], dtype=torch.int32)
    ref, mass, taps = P.resample(y.double(), r, nv.tolist(), Nout)
    assert [P.input_end(Nin, Nout, x) for x in r] == [320, 640, 960, 1120]
    assert 60 <= int(taps.max()) <= 64 and int(taps[0].max()) == 32 and int(taps[3, 0]) == 32
    out = ops.pitch_resample(y.to(DEV), r32.to(DEV), nv.to(DEV), Nout).cpu().double()
    assert out.shape == (4, Nout)
    bound = (taps + 4).double() * U * mass
    print(f"max |out - ref| / bound = {float(((out - ref).abs() / bound.clamp(min=1e-300)).max()):.3f}; "
          f"max |out - ref| = {float((out - ref).abs().max()):.3e}")
    assert bool(((out - ref).abs() <= bound).all())
    assert bool((out[2, 400:] == 0).all()) and bool(out[2, 399] != 0)
    assert float((out[1] - y[1, :Nout].double()).abs().max()) <= 4 * U * float(y.abs().max())   # ratio 1 copies


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
@gpu
def test_normalizer_moves_the_mean_f0_to_the_target():
    from speech_anonymization_amd import data, pitchnorm
    wav, lens = next(iter(data.synthetic_gender_dataset(4, 4))).sig
    N = wav.shape[1]
    norm = pitchnorm.PitchNormalizer(target_hz=170.0)
    out = norm(wav.to(DEV), lens)
    assert out.shape == wav.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    ratio, mean_in, voiced_in = (t.cpu() for t in norm.last)
    nb = P.n_valid(lens, N)
    for b in range(4):
        assert bool((out[b, int(nb[b]):] == 0).all())
    mean, voiced, frames = P.voiced_mean(pitchnorm.f0_track(out).cpu().double(), lens, N)
    print("in", mean_in.tolist(), "ratio", ratio.tolist(), "out", mean.tolist(), "voiced", voiced.tolist(), "of",
          frames.tolist(), f"bar {BAR_HZ:.3f} Hz")
    assert bool((voiced_in >= norm.min_voiced).all()) and bool((voiced >= norm.min_voiced).all())
    assert bool(((ratio.double() - 170.0 / mean_in.double()).abs() <= 1e-5).all())
    assert bool(((mean - 170.0).abs() <= BAR_HZ).all())
    again = pitchnorm.PitchNormalizer(target_hz=170.0).shift(wav.to(DEV), lens, norm.last[0])
    assert torch.equal(again, out)                                          # same seed, same bits


@gpu
def test_recipe_main_trains_one_epoch(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("gender_classifier_train_pitch_norm",
                                                  os.path.join(ROOT, "gender_classifier_train_pitch_norm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "pitch_norm"
    mod.main([os.path.join(ROOT, "speechbrain_configs", "gender_classifier_pitch_norm.yaml"), "--device", DEV,
              "--output_folder", str(out), "--synthetic", "16", "--batch_size", "8", "--number_of_epochs", "1",
              "--pitch_target_hz", "180"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(res)
    assert math.isfinite(res["test_loss"]) and 0.0 <= res["test_error"] <= 1.0 and res["pitch_target_hz"] == 180.0
    ck = res["best_checkpoint"]
    assert ck and os.path.isdir(ck) and os.path.dirname(ck) == str(out / "save")
    for name in ("embedding_model.ckpt", "classifier.ckpt", "normalizer.ckpt"):
        assert os.path.isfile(os.path.join(ck, name))


def _anonymize(capsys, argv):
    return anon_cli.run(capsys, ["--device", DEV, "--synthetic", "4", "--seed", "3"] + argv)


@gpu
def test_anonymize_pitch_norm_and_report_f0(tmp_path, capsys):
    """--pitch_norm true writes the normalised waveforms without a model or a checkpoint; --report_f0 true adds the
    mean F0 and the voiced share, here and in passthrough mode (where the vocoder leaves the pitch where it was)"""
    from speech_anonymization_amd import data
    out = tmp_path / "pn"
    res = _anonymize(capsys, ["--out_dir", str(out), "--pitch_norm", "true", "--report_f0", "true"])
    assert res["pitch_norm"] is True and res["pitch_target_hz"] == 170.0 and res["n_iter"] == 32
    lens = torch.cat([b.sig[1] for b in data.synthetic_gender_dataset(4, 3, seed=3)])    # convae.yaml: batch_size 3
    assert sorted(os.listdir(out)) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    for i, u in enumerate(res["utterances"]):
        sig = data.read_audio(os.path.join(out, u["id"] + ".wav"))
        assert u["id"] == f"synthetic_{i:04d}" and sig.numel() == u["samples"] == int(round(float(lens[i]) * 16000))
        assert 0.5 <= u["ratio"] <= 2.0 and u["peak"] > 0.0
        assert abs(u["f0_mean_hz"] - 170.0) <= BAR_HZ and 0.5 < u["voiced_share"] <= 1.0, u
    ref = tmp_path / "ref"
    res = _anonymize(capsys, ["--out_dir", str(ref), "--passthrough", "true", "--n_iter", "8", "--report_f0", "true",
                              "--model_type", "fcae"])
    assert res["passthrough"] and all(set(u) >= {"f0_mean_hz", "voiced_share", "spectral_convergence"}
                                      for u in res["utterances"])
    assert all(u["f0_mean_hz"] == 0.0 or 60.0 <= u["f0_mean_hz"] <= 400.0 for u in res["utterances"])
