"""Host side of the pitch normalisation (speech_anonymization_amd.pitchnorm): the fp64
restatement's tracker on the synthetic set, the ratio logic, the refusals of the recipe and of anonymize.py, the
entry points' -EINVAL answers and the ops' refusal of CPU tensors.  No GPU."""
import ctypes
import errno
import os
import types

import pytest
import torch

from tests import pitch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_yin_finds_the_generators_fundamentals():
    """data.synthetic_gender_dataset(8, 8) draws its labels, then its fundamentals, first from its generator: the
    same two draws give the true values.  The restatement's voiced mean is within 0.5 Hz of each (measured: 0.03)
    and no frame of the set is an unstable one at the GPU test's epsilon."""
    from speech_anonymization_amd import data
    g = torch.Generator().manual_seed(1986)
    label = torch.randint(0, 2, (8,), generator=g)
    lo = torch.where(label == 0, 100.0, 190.0).double()
    hi = torch.where(label == 0, 140.0, 250.0).double()
    true = lo + (hi - lo) * torch.rand(8, generator=g, dtype=torch.float64)
    batch = next(iter(data.synthetic_gender_dataset(8, 8)))
    assert torch.equal(batch.gender, label)
    wav, lens = batch.sig
    f0, dp, p = P.yin(wav)
    assert f0.shape == (8, 16000 // 160 + 1) and dp.shape == (8, 101, 267)
    mean, voiced, frames = P.voiced_mean(f0, lens, wav.shape[1])
    print("true", true.tolist(), "\nfound", mean.tolist(), "\nvoiced", voiced.tolist(), "of", frames.tolist())
    assert float((mean - true).abs().max()) <= 0.5
    assert bool((voiced >= 0.9 * frames).all())
    tail = P.n_valid(lens, wav.shape[1]) // 160 + 4                       # frames that read only the zeroed tail
    for b in range(8):
        assert not f0[b, int(tail[b]):].any()
    assert int((~P.stable(dp, p)).sum()) == 0


def test_reference_ratio_clamps_and_min_voiced():
    N = 160 * 19 + 37
    f0 = torch.zeros(5, 20, dtype=torch.float64)
    f0[0, 2:12] = 60.0                       # 170 / 60 = 2.83 -> r_max
    f0[1, :] = 390.0                         # 170 / 390 = 0.436 -> r_min
    f0[2, 3:7] = 150.0                       # 4 voiced frames < 5 -> 1
    f0[3, :8] = 100.0                        # lens cuts the row to 1600 // 160 + 1 = 11 frames: 300 Hz is not seen
    f0[3, 11:] = 300.0
    f0[4, :] = 170.0 / 2.0                   # exactly the upper edge
    lens = torch.tensor([1.0, 1.0, 1.0, 1600.4 / N, 1.0])
    r, m, v = P.ratio(f0, lens, N)
    assert r.tolist() == [2.0, 0.5, 1.0, 1.7, 2.0]
    assert v.tolist() == [10, 20, 4, 8, 20] and m.tolist() == [60.0, 390.0, 150.0, 100.0, 85.0]
    r, _, _ = P.ratio(f0, lens, N, target_hz=120.0, r_min=0.8, r_max=1.25, min_voiced=4)
    assert r.tolist() == [1.25, 0.8, 0.8, 1.2, 1.25]
    r, _, v = P.ratio(torch.zeros(1, 20), torch.ones(1), N)                # no voiced frame at all
    assert r.tolist() == [1.0] and v.tolist() == [0]


def test_reference_stretch_and_resample_are_the_identity_at_ratio_one():
    g = torch.Generator().manual_seed(3)
    mag = torch.rand(2, 7, 5, generator=g, dtype=torch.float64)
    S, _, Tb = P.stretch(mag, [1.0, 1.0])
    assert Tb == [7, 7] and torch.equal(S, mag)
    S, _, Tb = P.stretch(mag, [0.5, 2.0])
    assert Tb == [4, 13] and S.shape == (2, 13, 5) and not S[0, 4:].any()
    assert torch.equal(S[1, ::2], mag[1]) and torch.allclose(S[1, 1], 0.5 * (mag[1, 0] + mag[1, 1]))
    y = torch.randn(1, 6 * 160, generator=g, dtype=torch.float64)
    out, _, taps = P.resample(y, [1.0], [900], 6 * 160)
    assert float((out[0, :900] - y[0, :900]).abs().max()) <= 1e-15 and not out[0, 900:].any()
    assert int(taps.max()) == 31 and P.input_end(7 * 160, 560, 2.0) == 1120 and P.input_end(7 * 160, 560, 0.5) == 320


GOOD = {"pitch_norm": {"target_hz": 170.0, "r_min": 0.5, "r_max": 2.0}}


@pytest.mark.parametrize("change,run_opts,environ,word", [
    ({"pitch_target_hz": 500.0}, {}, {}, "--pitch_target_hz"),
    ({"pitch_target_hz": 59.0}, {}, {}, "--pitch_target_hz"),
    ({"pitch_norm": {"target_hz": 401.0}}, {}, {}, "--pitch_target_hz"),
    ({"pitch_norm": {"r_min": 0.4}}, {}, {}, "r_min"),
    ({"pitch_norm": {"r_max": 2.5}}, {}, {}, "r_max"),
    ({"pitch_norm": {"r_min": 1.5, "r_max": 1.2}}, {}, {}, "above"),
    ({}, {"distributed_launch": True}, {}, "data parallelism"),
    ({}, {}, {"WORLD_SIZE": "2"}, "data parallelism"),
    ({"hip_graph": True}, {}, {}, "hip_graph"),
    ({}, {"hip_graph": True}, {}, "hip_graph"),
])
def test_check_pitch_options_refuses_in_one_line(change, run_opts, environ, word):
    from speech_anonymization_amd import pitchnorm
    with pytest.raises(SystemExit) as e:
        pitchnorm.check_pitch_options(dict(GOOD, **change), run_opts, environ)
    msg = str(e.value)
    assert word in msg and "\n" not in msg


def test_check_pitch_options_accepts_and_the_yaml_loads(tmp_path):
    from speech_anonymization_amd import pitchnorm
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml, parse_arguments
    assert pitchnorm.check_pitch_options({}, {}, {})["target_hz"] == 170.0
    fn = os.path.join(ROOT, "speechbrain_configs", "gender_classifier_pitch_norm.yaml")
    _, run_opts, overrides = parse_arguments([fn, "--device", "cuda:0", "--pitch_target_hz", "200",
                                              "--output_folder", str(tmp_path)])
    with open(fn) as f:
        st = load_hyperpyyaml(f, overrides)
    pn = pitchnorm.check_pitch_options(st, run_opts, {})
    assert pn == {"target_hz": 200.0, "n_iter": 32, "momentum": 0.99, "seed": 1, "r_min": 0.5, "r_max": 2.0,
                  "min_voiced": 5, "threshold": 0.15}
    norm = pitchnorm.PitchNormalizer(**pn)
    assert norm.target_hz == 200.0 and norm.gl.n_iter == 32 and norm.gl.seed == 1 and norm.last is None
    with open(os.path.join(ROOT, "speechbrain_configs", "gender_classifier.yaml")) as f:
        plain = load_hyperpyyaml(f, {"output_folder": str(tmp_path)})
    st.pop("pitch_norm"), st.pop("pitch_target_hz")
    assert st == plain                                                    # a copy of the plain recipe's settings
    for bad in ({"target_hz": 30.0}, {"r_min": 0.3}, {"r_max": 3.0}, {"r_min": 1.5, "r_max": 1.0}):
        with pytest.raises(ValueError):
            pitchnorm.PitchNormalizer(**bad)


ANON = {"model_type": "fcae", "out_dir": "/tmp/out", "synthetic": 4, "pitch_norm": True}


@pytest.mark.parametrize("change,word", [
    ({"passthrough": True}, "--passthrough"),
    ({"recon_ckpt": "/some/CKPT+x"}, "--recon_ckpt"),
    ({"pitch_target_hz": 500}, "--pitch_target_hz"),
    ({"out_dir": None}, "--out_dir"),
    ({"hip_graph": True}, "hip_graph"),
])
def test_check_anonymize_options_pitch_norm_branches(change, word):
    from speech_anonymization_amd import vocoder
    with pytest.raises(SystemExit) as e:
        vocoder.check_anonymize_options(dict(ANON, **change), {}, {})
    msg = str(e.value)
    assert word in msg and "\n" not in msg


def test_check_anonymize_options_lets_pitch_norm_through():
    from speech_anonymization_amd import vocoder
    vocoder.check_anonymize_options(dict(ANON), {"device": "cuda:0"}, {})
    vocoder.check_anonymize_options(dict(ANON, model_type=None, pitch_target_hz=200, report_f0=True), {}, {})
    vocoder.check_anonymize_options({"model_type": "fcae", "recon_ckpt": "/x", "out_dir": "/o", "synthetic": 2,
                                     "report_f0": True}, {}, {})
    with pytest.raises(SystemExit, match="--recon_ckpt DIR is required without --passthrough true"):
        vocoder.check_anonymize_options(dict(ANON, pitch_norm=False), {}, {})


def test_yin_dim_exports_the_constants():
    from speech_anonymization_amd import _lib, pitchnorm
    lib = _lib.load()
    assert [lib.sa_yin_dim(i) for i in range(8)] == [16000, 160, 400, 40, 266, 666, 8, 256]
    assert lib.sa_yin_dim(8) == -errno.EINVAL and lib.sa_yin_dim(-1) == -errno.EINVAL
    assert (pitchnorm.SAMPLE_RATE, pitchnorm.W, pitchnorm.TAU_MIN, pitchnorm.TAU_MAX) == (16000, 400, 40, 266)
    assert (P.SR, P.HOP, P.W, P.TAU_MIN, P.TAU_MAX, P.L) == (16000, 160, 400, 40, 266, 666)


def test_entry_points_refuse_bad_arguments():
    """-EINVAL before any launch: NULL pointers, B < 1, B > 65535, N < 1, sizes past the documented bounds, ratio
    bounds outside [0.5, 2] or crossed.  The pointers are host buffers nothing dereferences."""
    from speech_anonymization_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p, f, E = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_float, -errno.EINVAL
    big = (1 << 30) + 1

    def yin(wav=p, B=2, N=500, f0=p):
        return lib.sa_yin_f0(wav, B, N, f(0.15), f0, None, None)

    for bad in (dict(wav=None), dict(f0=None), dict(B=0), dict(B=-1), dict(B=65536), dict(N=0), dict(N=-5), dict(N=big)):
        assert yin(**bad) == E, bad

    def ratio(f0=p, lens=p, B=2, T=20, N=3077, target=170.0, r_min=0.5, r_max=2.0, ratio=p, mean=p, voiced=p):
        return lib.sa_pitch_ratio(f0, lens, B, T, N, f(target), f(r_min), f(r_max), 5, ratio, mean, voiced, None)

    for bad in (dict(f0=None), dict(lens=None), dict(ratio=None), dict(mean=None), dict(voiced=None), dict(B=0),
                dict(B=65536), dict(T=0), dict(T=(1 << 23) + 1), dict(N=0), dict(N=big), dict(target=0.0),
                dict(target=float("nan")), dict(r_min=0.49), dict(r_max=2.01), dict(r_min=1.5, r_max=1.2),
                dict(r_min=float("nan"))):
        assert ratio(**bad) == E, bad

    def stretch(R=p, ratio=p, B=2, T=11, Tout=21, S=p):
        return lib.sa_pitch_stretch_mag(R, ratio, B, T, Tout, S, None)

    for bad in (dict(R=None), dict(ratio=None), dict(S=None), dict(B=0), dict(B=65536), dict(T=1), dict(T=(1 << 23) + 1),
                dict(Tout=0), dict(Tout=(1 << 23) + 1)):
        assert stretch(**bad) == E, bad

    def resample(y=p, ratio=p, nv=p, B=2, Nin=1120, Nout=560, out=p):
        return lib.sa_pitch_resample(y, ratio, nv, B, Nin, Nout, out, None)

    for bad in (dict(y=None), dict(ratio=None), dict(nv=None), dict(out=None), dict(B=0), dict(B=65536), dict(Nin=0),
                dict(Nin=big), dict(Nout=0), dict(Nout=(1 << 29) + 1)):
        assert resample(**bad) == E, bad


def test_ops_refuse_cpu_tensors_before_loading_anything(monkeypatch):
    from speech_anonymization_amd import _lib, ops, pitchnorm
    from speech_anonymization_amd._lib import SaHipError

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(SaHipError, match="GPU"):
        ops.yin_f0(torch.zeros(1, 500))
    with pytest.raises(SaHipError, match="GPU"):
        ops.pitch_ratio(torch.zeros(1, 4), torch.ones(1), 500)
    with pytest.raises(SaHipError, match="GPU"):
        ops.pitch_stretch_mag(torch.zeros(1, 4, 201, dtype=torch.complex64), torch.ones(1), 4)
    with pytest.raises(SaHipError, match="GPU"):
        ops.pitch_resample(torch.zeros(1, 480), torch.ones(1), torch.ones(1, dtype=torch.int32), 480)
    with pytest.raises(SaHipError, match="GPU"):
        pitchnorm.f0_track(torch.zeros(1, 500))
    with pytest.raises(SaHipError, match="GPU"):
        pitchnorm.PitchNormalizer()(torch.zeros(1, 500), torch.ones(1))
    with pytest.raises(SaHipError, match="GPU"):
        pitchnorm.PitchNormalizer().shift(torch.zeros(1, 500), torch.ones(1), torch.ones(1))


def test_pitch_norm_brain_normalises_at_every_stage_before_the_features(monkeypatch):
    """the pitch_norm recipe's brain (GenderBrain with the normaliser as its one waveform transform): the normaliser
    sees the raw waveforms at TRAIN, VALID and TEST, and the augmentation and the front end see what it returned"""
    from speech_anonymization_amd import gender, pitchnorm
    from speech_anonymization_amd.brain import Batch, Stage

    class Modules(dict):
        __getattr__ = dict.__getitem__

    seen = []

    def normalizer(wavs, lens):
        seen.append(("norm", wavs))
        return wavs + 1.0

    def fbank(wavs):
        seen.append(("fbank", wavs))
        return wavs[:, :, None]

    row = gender.RECIPES["gender_classifier_train_pitch_norm"]
    assert row.brain is gender.GenderBrain
    made = row.transforms(row.check({}, {}, {}))
    assert len(made) == 1 and isinstance(made[0], pitchnorm.PitchNormalizer)
    monkeypatch.setattr(gender.xvector, "train_log_probs", lambda emb, cl, feats, lens: feats)
    b = object.__new__(gender.GenderBrain)
    b.device = torch.device("cpu")
    b.modules = Modules(compute_features=fbank, mean_var_norm=lambda feats, lens: feats, embedding_model=None,
                        classifier=None)
    b.hparams = types.SimpleNamespace(waveform_transforms=[normalizer])
    wav, lens = torch.zeros(2, 8), torch.ones(2)
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        del seen[:]
        out = b.compute_forward(Batch(wav, lens, torch.zeros(2, dtype=torch.long)), stage)
        assert [k for k, _ in seen] == ["norm", "fbank"] and seen[0][1] is wav
        assert torch.equal(seen[1][1], wav + 1.0) and out.shape == (2, 8, 1)
