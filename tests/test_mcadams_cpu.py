"""CPU checks of the McAdams transform: the fp64 restatement's own identities, the conditioning of
the inputs the GPU test compares on, the one-line refusals, the recipe's settings, the symbol list and the
entry point's -EINVAL -- nothing here needs a GPU."""
import ctypes
import errno
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import mcadams_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_MEASURED, C_FACTOR = M.C_MEASURED, M.C_FACTOR         # 1.43e-10 (tools/mcadams_delta.py) and 16


def test_restatement_reproduces_its_input_at_alpha_one():
    """phi^1 = phi, a' = a, IIR(1 / a) FIR(a) = identity, and w^2 sums to 1 at hop 160: measured 3e-11"""
    wav = np.stack([M.voiced_row(130.0, M.FORMANTS, 1687, 7), M.voiced_row(220.0, M.FORMANTS, 1687, 8)])
    nv = np.array([1687, 1200])
    out = M.mcadams(wav, np.ones(2, np.float32), nv, level=False, copy_unity=False)
    assert (out.status[0] == M.OK).all()
    live = np.arange(1687)[None, :] < nv[:, None]
    x = np.asarray(wav, np.float32).astype(np.float64)
    err = np.abs(out.out - np.where(live, x, 0.0)).max()
    print("identity error", err)
    assert err <= 1e-9
    np.testing.assert_array_equal(out.out[1, 1200:], 0.0)
    sq = M.WINDOW ** 2
    np.testing.assert_allclose(sq[:M.H] + sq[M.H:], 1.0, rtol=0, atol=8 * 2.0 ** -53)    # 0.5 -+ 0.5 cos, the root, the square, the sum


def test_window_framing_and_frame_count():
    assert [M.n_frames(n) for n in (1, 50, 160, 161, 1600, 1687)] == [2, 2, 2, 3, 11, 12]
    fr = M.frames_of(np.ones(50), 30)
    assert fr.shape == (2, 320)
    np.testing.assert_array_equal(fr[0, :160], 0.0)                        # samples before 0
    np.testing.assert_array_equal(fr[0, 160:190], M.WINDOW[160:190])
    np.testing.assert_array_equal(fr[0, 190:], 0.0)                        # from n_valid on
    np.testing.assert_array_equal(fr[1, :30], M.WINDOW[:30])


def test_a_known_pole_pair_moves_to_phi_to_the_alpha():
    """one resonance at angle phi: the rebuilt polynomial has its pair at phi^alpha with the same modulus"""
    phi, mod, alpha = 0.6, 0.95, 0.7
    z = np.concatenate([[mod * np.exp(1j * phi), mod * np.exp(-1j * phi)], 0.3 * np.exp(2j * np.pi * (np.arange(18) + 0.5) / 18)])
    a = np.real(np.poly(z))
    a2, ok, _ = M.rebuild(np.roots(a), alpha)
    assert ok
    got = np.roots(a2)
    top = got[np.argmax(np.abs(got) * (got.imag > 0))]
    assert abs(abs(top) - mod) < 1e-9 and abs(np.angle(top) - phi ** alpha) < 1e-9


def test_aberth_agrees_with_numpy_roots():
    f = M.frames_of(M.voiced_row(150.0, M.FORMANTS, 800, 9), 800)[2]
    r = M.autocorr(f)
    r[0] *= 1.0 + M.R0_LIFT
    a, _, ok = M.levinson(r)
    assert ok
    z, it, conv = M.aberth(a)
    assert conv and it <= 20
    want = np.roots(a)
    assert max(np.abs(want - v).min() for v in z) < 1e-10


def test_alpha_is_sanitised_as_the_kernel_does():
    got = M.sanitize_alpha(np.array([9.0, 0.1, np.nan, 0.8, 1.0], np.float32))
    np.testing.assert_array_equal(got, np.array([2.0, 0.25, 1.0, np.float32(0.8), 1.0], np.float64))


@pytest.mark.parametrize("level", [True, False])
def test_gpu_cases_are_well_conditioned(level):
    """checked before any GPU comparison: on every case the restatement leaves out no sample, flags no fallback, and
    the recorded C leaves the bar under a quarter of an fp32 rounding"""
    assert C_FACTOR * C_MEASURED <= M.U / 4
    names = [c[0] for c in M.gpu_cases()]
    assert names == ["odd", "two_frames", "empty_row", "synthetic"]
    for name, wav, alpha, nv in M.gpu_cases():
        ref = M.case_ref(name, level)
        assert not ref.left_out.any() and not ref.near.any(), name
        assert not (ref.status == M.FALLBACK).any(), name
        assert ref.status.shape == (wav.shape[0], M.n_frames(wav.shape[1]))
    odd = M.case_ref("odd", level)
    assert (odd.status[0] == M.OK).all() and (odd.status[1] == 0).all()
    assert (odd.status[2, 8:] == M.SILENT).all() and (odd.status[2, :6] == M.OK).all()
    np.testing.assert_array_equal(odd.out[1], odd.x[1])                    # alpha = 1: copied
    empty = M.case_ref("empty_row", level)
    assert (empty.status[0] == M.SILENT).all() and not empty.out[0].any() and empty.gain[0] == 1.0
    if level:
        for b in (0, 2):
            n = int(odd.n_valid[b])
            np.testing.assert_allclose(np.sum(odd.out[b, :n] ** 2), np.sum(odd.x[b, :n] ** 2), rtol=1e-12)
    else:
        assert (odd.gain == 1.0).all()


def test_recorded_c_matches_the_restatement():
    """the figure the GPU bar uses is the one tools/mcadams_delta.py measures (on one case here, to stay quick)"""
    name, wav, alpha, nv = M.gpu_cases()[0]
    ref = M.case_ref(name, True)
    ab = M.mcadams(wav, alpha, nv, True, roots=M.aberth)
    rv = M.mcadams(wav, alpha, nv, True, reverse_acf=True)
    assert (ab.status == ref.status).all() and ab.iters <= 20
    peak = np.abs(ref.out).max(1, keepdims=True)
    c = max((np.abs(ab.out - ref.out) / peak).max(), (np.abs(rv.out - ref.out) / peak).max())
    print("C on the first case", c)
    assert c <= 4.0 * C_MEASURED


# ---- refusals, before any device is touched ------------------------------------------------------------
@pytest.mark.parametrize("settings, word", [
    ({"mcadams": 0.3}, "--mcadams 0.3: a McAdams coefficient between 0.5 and 1.2"),
    ({"mcadams": 1.5}, "--mcadams 1.5: a McAdams coefficient"),
    ({"mcadams": "x"}, "--mcadams x: a McAdams coefficient"),
    ({"mcadams": True}, "--mcadams True: a McAdams coefficient"),
    ({"mcadams_min": 0.6}, "--mcadams_min LO and --mcadams_max HI go together"),
    ({"mcadams_max": 0.9}, "--mcadams_min LO and --mcadams_max HI go together"),
    ({"mcadams_min": 0.9, "mcadams_max": 0.6}, "--mcadams_min 0.9 is above --mcadams_max 0.6"),
    ({"mcadams_min": 0.4, "mcadams_max": 0.6}, "--mcadams_min 0.4: a McAdams coefficient"),
    ({"mcadams_min": 0.6, "mcadams_max": 1.3}, "--mcadams_max 1.3: a McAdams coefficient"),
    ({"mcadams": 0.8, "mcadams_min": 0.6, "mcadams_max": 0.9}, "exclude each other"),
])
def test_check_mcadams_options_refuses_in_one_line(settings, word):
    from speech_anonymization_amd import mcadams
    with pytest.raises(SystemExit) as e:
        mcadams.check_mcadams_options(settings)
    assert word in str(e.value) and "\n" not in str(e.value)


def test_check_mcadams_options_returns_the_constructor_arguments():
    from speech_anonymization_amd import mcadams
    assert mcadams.check_mcadams_options({"mcadams": 0.7}) == {"alpha": 0.7, "seed": 1, "level": True}
    assert mcadams.check_mcadams_options({}) == {"alpha": 0.8, "seed": 1, "level": True}
    got = mcadams.check_mcadams_options({"mcadams_min": 0.5, "mcadams_max": 0.9,
                                         "mcadams_options": {"alpha": 0.8, "seed": 5, "level": False}})
    assert got == {"alpha_range": (0.5, 0.9), "seed": 5, "level": False}
    block = {"mcadams_options": {"alpha_min": 0.6, "alpha_max": 0.7}}
    assert mcadams.check_mcadams_options(block)["alpha_range"] == (0.6, 0.7)
    assert mcadams.check_mcadams_options(dict(block, mcadams=0.9))["alpha"] == 0.9
    for kw in (dict(alpha=0.4), dict(alpha=1.3), dict(alpha_range=(0.9, 0.6)), dict(alpha_range=(0.4, 0.6)),
               dict(alpha_range=(0.6,))):
        with pytest.raises(ValueError, match="McAdams"):
            mcadams.McAdams(**kw)


BASE = {"model_type": "convae", "out_dir": "o", "synthetic": 4, "mcadams": 0.8}


@pytest.mark.parametrize("change, word", [
    ({"pitch_norm": True}, "--mcadams and --pitch_norm true exclude each other"),
    ({"formant_ratio": 1.1}, "--mcadams and --formant_ratio exclude each other"),
    ({"preserve_formants": True}, "--mcadams and --preserve_formants true exclude each other"),
    ({"recon_ckpt": "d"}, "--mcadams and --recon_ckpt exclude each other"),
    ({"passthrough": True}, "--mcadams and --passthrough true exclude each other"),
    ({"mcadams": 2.0}, "--mcadams 2.0: a McAdams coefficient"),
    ({"out_dir": None}, "--out_dir OUT is required"),
    ({"hip_graph": True}, "anonymize does not support --hip_graph"),
])
def test_check_anonymize_options_mcadams_branches(change, word):
    from speech_anonymization_amd import vocoder
    with pytest.raises(SystemExit) as e:
        vocoder.check_anonymize_options(dict(BASE, **change), {}, {})
    assert word in str(e.value) and "\n" not in str(e.value)


def test_check_anonymize_options_lets_mcadams_through_and_keeps_the_other_modes():
    from speech_anonymization_amd import vocoder
    vocoder.check_anonymize_options(dict(BASE), {"device": "cuda:0"}, {})
    vocoder.check_anonymize_options(dict(BASE, model_type=None, report_f0=True), {}, {})       # no model runs
    vocoder.check_anonymize_options({"out_dir": "o", "synthetic": 2, "mcadams_min": 0.5, "mcadams_max": 0.9}, {}, {})
    with pytest.raises(SystemExit, match="--recon_ckpt DIR is required without --passthrough true"):
        vocoder.check_anonymize_options(dict(BASE, mcadams=None), {}, {})
    with pytest.raises(SystemExit, match="unknown model_type None"):
        vocoder.check_anonymize_options(dict(BASE, mcadams=None, model_type=None), {}, {})
    with pytest.raises(SystemExit, match="anonymize runs on one GPU"):
        vocoder.check_anonymize_options(dict(BASE), {}, {"WORLD_SIZE": "2"})


def test_anonymize_refuses_before_it_touches_a_device(monkeypatch, tmp_path):
    def no_device(*a, **k):
        raise AssertionError("a device was touched")

    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    spec = importlib.util.spec_from_file_location("anonymize", os.path.join(ROOT, "anonymize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = os.path.join(ROOT, "speechbrain_configs", "convae.yaml")
    for extra, word in ((["--mcadams", "0.8", "--passthrough", "true"], "--mcadams and --passthrough true"),
                        (["--mcadams", "1.4"], "--mcadams 1.4"),
                        (["--mcadams_min", "0.6"], "go together"),
                        (["--mcadams", "0.8", "--pitch_norm", "true"], "--mcadams and --pitch_norm true")):
        with pytest.raises(SystemExit) as e:
            mod.main([cfg, "--synthetic", "2", "--out_dir", str(tmp_path / "never")] + extra)
        assert word in str(e.value) and "\n" not in str(e.value)
    assert not (tmp_path / "never").exists()


# ---- the recipe ---------------------------------------------------------------------------------------------
def test_recipe_config_loads_and_refuses():
    from speech_anonymization_amd import mcadams
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    path = os.path.join(ROOT, "speechbrain_configs", "gender_classifier_mcadams.yaml")
    with open(path) as fin:
        settings = load_hyperpyyaml(fin, {})
    assert settings["mcadams_options"] == {"alpha": 0.8, "seed": 1, "level": True}
    assert "pitch_norm" not in settings and settings["output_folder"].endswith("gender_classifier_mcadams")
    assert mcadams.check_recipe_options(settings, {}, {}) == {"alpha": 0.8, "seed": 1, "level": True}
    with open(path) as fin:
        ranged = load_hyperpyyaml(fin, {"mcadams_min": 0.5, "mcadams_max": 0.9})
    assert mcadams.check_recipe_options(ranged, {}, {})["alpha_range"] == (0.5, 0.9)
    with pytest.raises(SystemExit, match="gender_classifier_train_mcadams does not support --hip_graph"):
        mcadams.check_recipe_options(dict(settings, hip_graph=True), {}, {})
    with pytest.raises(SystemExit, match="gender_classifier_train_mcadams runs on one GPU"):
        mcadams.check_recipe_options(settings, {"distributed_launch": True}, {})
    with pytest.raises(SystemExit, match="gender_classifier_train_mcadams runs on one GPU"):
        mcadams.check_recipe_options(settings, {}, {"WORLD_SIZE": "4"})
    with pytest.raises(SystemExit, match="--mcadams 0.2"):
        mcadams.check_recipe_options(dict(settings, mcadams=0.2), {}, {})
    assert os.path.exists(os.path.join(ROOT, "gender_classifier_train_mcadams.py"))


def test_alpha_draw_is_deterministic_in_seed_and_call_count():
    from speech_anonymization_amd import mcadams
    dev = torch.device("cpu")                                # the draw itself runs wherever its generator lives
    a, b = mcadams.McAdams(alpha_range=(0.5, 0.9), seed=3), mcadams.McAdams(alpha_range=(0.5, 0.9), seed=3)
    first, second = a.draw(4, dev), a.draw(4, dev)
    assert torch.equal(first, b.draw(4, dev)) and torch.equal(second, b.draw(4, dev))
    assert not torch.equal(first, second)
    assert not torch.equal(first, mcadams.McAdams(alpha_range=(0.5, 0.9), seed=4).draw(4, dev))
    assert float(first.min()) >= 0.5 and float(first.max()) <= 0.9 and first.dtype == torch.float32
    assert torch.equal(mcadams.McAdams(0.7).draw(3, dev), torch.full((3,), 0.7))


# ---- the library boundary -------------------------------------------------------------------------------
def test_symbols_and_dimensions():
    from speech_anonymization_amd import _lib, ops
    assert "sa_mcadams" in _lib.SYMBOLS and "sa_mcadams_dim" in _lib.SYMBOLS
    lib = _lib.load()
    assert [lib.sa_mcadams_dim(i) for i in range(7)] == [320, 160, 20, 1, 64, 64, 4096]
    assert lib.sa_mcadams_dim(7) == -errno.EINVAL and lib.sa_mcadams_dim(-1) == -errno.EINVAL
    assert (M.W, M.H, M.P, M.ABERTH_MAX) == (320, 160, 20, 64)
    assert (ops.MC_W, ops.MC_H, ops.MC_CHUNK) == (320, 160, 4096)
    assert [ops.mcadams_frames(n) for n in (1, 160, 161, 1687)] == [M.n_frames(n) for n in (1, 160, 161, 1687)]


def test_entry_point_refuses_bad_arguments():
    """-EINVAL before any launch.  The pointers are host buffers nothing dereferences."""
    from speech_anonymization_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p, E = ctypes.cast(buf, ctypes.c_void_p), -errno.EINVAL

    def call(wav=p, alpha=p, n_valid=p, B=2, N=1600, level=1, out=p, ws=p, status=None, gain=None):
        return lib.sa_mcadams(wav, alpha, n_valid, B, N, level, out, ws, status, gain, None)

    for bad in (dict(wav=None), dict(alpha=None), dict(n_valid=None), dict(out=None), dict(ws=None), dict(B=0),
                dict(B=-1), dict(B=65536), dict(N=0), dict(N=-5), dict(N=(1 << 30) + 1)):
        assert call(**bad) == E, bad


def test_ops_and_class_refuse_cpu_tensors_before_loading_anything(monkeypatch):
    from speech_anonymization_amd import _lib, mcadams, ops
    from speech_anonymization_amd._lib import SaHipError

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(SaHipError, match="GPU"):
        ops.mcadams(torch.zeros(1, 500), torch.ones(1), torch.full((1,), 500, dtype=torch.int32))
    with pytest.raises(SaHipError, match="GPU"):
        mcadams.McAdams(0.8)(torch.zeros(1, 500), torch.ones(1))
