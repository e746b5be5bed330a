"""The source-filter resynthesis without a GPU: properties of the integer / fp64 restatement
(tests/srcfilt_ref.py) -- the pulse chain, its clamps and both frame counts, the noise, the statuses of the GPU test's
own inputs, which must leave no frame near a decision before that test relies on it -- the constant C of the GPU
test's bar recomputed against profiles/srcfilt_delta.json, the option checkers' one-line refusals, and the ABI header
against the binding."""
import os
import re

import numpy as np
import pytest

from speech_anonymization_amd import sourcefilter  # noqa: F401  (without the feature nothing here can run)
from tests import mcadams_ref as M
from tests import srcfilt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- pulses ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.waves()))
@pytest.mark.parametrize("padded", [False, True])
def test_chain_spacing_and_capacity(name, padded):
    wav, nv, f0, _ = R.case_inputs(name, padded)
    B, N = wav.shape
    assert f0.shape[1] == R.frames_of_track(N, padded)
    for label, rho in R.rho_variants(name, f0.shape[1]).items():
        pos, per, count = R.pulses(f0, rho, nv, N)
        assert pos.shape == per.shape == (B, N // 40 + 2)
        for b in range(B):
            k = int(count[b])
            assert k <= N // 40 + 1
            p, d = pos[b, :k], per[b, :k]
            assert (np.diff(p) >= 40 << 16).all() and (p >> 16 < max(int(nv[b]), 0)).all() and (p >= 0).all()
            assert ((d >= 40 << 16) & (d <= 266 << 16)).all()
            voiced = R.voiced(f0[b])
            for s, q in zip(p, d):                           # a pulse sits in a voiced frame and carries its period
                t = R.frame(int(s) >> 16, f0.shape[1])
                assert voiced[t] and q == R.periods(f0[b], None if rho is None else rho[b])[t]
            if int(nv[b]) == 0 or not voiced.any():
                assert k == 0


def test_both_frame_counts_differ_only_where_they_must():
    """N = 1687: 11 frames of the waveform, 12 of the padded one; the last frame's pulses move when frame 11 exists"""
    f11, f12 = np.full((1, 11), 100.0, np.float32), np.full((1, 12), 100.0, np.float32)
    f12[0, 11] = 0.0
    a = R.pulses(f11, None, [1687], 1687)
    b = R.pulses(f12, None, [1687], 1687)
    assert a[2][0] == 11                                     # 0, 160, ..., 1600: frame 10 absorbs the tail
    assert b[2][0] == 11 and (a[0] == b[0]).all()            # 1600 + 80 = 1680 is where frame 11 starts: 1600 is the last
    f12[0, 10] = 0.0                                         # frame 10 unvoiced, frame 11 unvoiced and last: stop
    c = R.pulses(f12, None, [1687], 1687)
    assert c[2][0] == 10
    assert R.frames_of_track(1600) == R.frames_of_track(1600, True) == 11


def test_period_clamps_and_voicing():
    f0 = np.array([900.0, 30.0, np.nan, -1.0, np.inf, 0.0, 160.0, 1e-30, 3e38], np.float32)
    p = R.periods(f0)
    assert p[0] == 40 << 16 and p[1] == 266 << 16            # 17.8 and 533 samples, clamped
    assert p[2] == p[3] == p[4] == p[5] == 0                 # NaN, negative, +inf, 0: unvoiced
    assert p[6] == 100 << 16 and p[7] == 266 << 16 and p[8] == 40 << 16
    assert R.voiced(f0).tolist() == [True, True, False, False, False, False, True, True, True]
    # rint, half to even, on one rounding of the quotient: 16000 2^32 / (f 2^16) for f = 2^k is exact
    assert R.periods(np.array([128.0], np.float32))[0] == 125 << 16
    # rho divides the period, and is clamped to [2^15, 2^17]
    f = np.full(4, 100.0, np.float32)
    p = R.periods(f, np.array([1 << 16, 1, 1 << 30, 3 << 15]))
    assert p.tolist() == [160 << 16, 266 << 16, 80 << 16, (160 << 17) // 3 + 1]    # 320 clamped; 106.67 rounded up
    assert R.periods(f, np.array([1, 1, 1, 1])).tolist() == R.periods(f, np.full(4, 1 << 15)).tolist()


def test_walk_jumps_over_unvoiced_frames_and_stops_in_the_last():
    f0 = np.array([100.0, 0.0, 0.0, 100.0, 0.0], np.float32)       # T = 5 of N = 640
    pos, per = R.pulses_row(f0, None, 640, 640)
    # 160 is frame 1: jump to 240 (frame 2), to 400 (frame 3: a pulse); 560 is frame 4, unvoiced and the last: stop
    assert [s >> 16 for s in pos] == [0, 400]
    assert R.pulses_row(f0, None, 401, 640)[0] == pos
    assert R.pulses_row(f0, None, 400, 640)[0] == pos[:1]
    assert R.pulses_row(np.zeros(5, np.float32), None, 640, 640) == ([], [])
    # fractional positions: 16000 / 110 = 145.45 samples
    pos, per = R.pulses_row(np.full(5, 110.0, np.float32), None, 640, 640)
    assert len(pos) == 5 and all(b - a == per[0] for a, b in zip(pos, pos[1:])) and pos[1] & 0xffff


# ---- noise and excitation --------------------------------------------------------------------------------
def test_noise_is_exact_uniform_and_seeded():
    u = R.noise(11, 1 << 16)
    assert u.dtype == np.float32 and u.min() >= -1.0 and u.max() < 1.0
    k = u.astype(np.float64) * 2.0 ** 23
    assert (k == np.rint(k)).all()                           # multiples of 2^-23: exact in fp32
    assert abs(float(u.mean())) < 0.01 and abs(float((u.astype(np.float64) ** 2).mean()) - 1.0 / 3.0) < 0.01
    assert not np.array_equal(u, R.noise(12, 1 << 16))
    assert np.array_equal(R.noise(-5, 64), R.noise((1 << 32) - 5, 64))      # the seed is read as uint32
    # the mix itself: 0 is its fixed point, and it is a bijection of uint32 (no two of 2^16 inputs collide)
    assert int(R.mix(np.uint64(0))) == 0
    assert len(set(R.mix(np.arange(1 << 16, dtype=np.uint64)).tolist())) == 1 << 16
    s = R.draw_seeds(1, 0, 6)
    assert s.dtype == np.int32 and (s >= 0).all() and len(set(s.tolist())) == 6
    assert np.array_equal(R.draw_seeds(1, 3, 3), s[3:]) and not np.array_equal(R.draw_seeds(2, 0, 6), s)


def test_sourcefilter_draws_the_restatements_seeds():
    """the class's counter-based draw, run on the CPU here: the same integers as the restatement"""
    from speech_anonymization_amd import sourcefilter
    sf = sourcefilter.SourceFilter(seed=1)
    a, b = sf.draw(4, "cpu"), sf.draw(2, "cpu")
    assert np.array_equal(np.concatenate([a.numpy(), b.numpy()]), R.draw_seeds(1, 0, 6))
    other = sourcefilter.SourceFilter(seed=77)
    assert np.array_equal(other.draw(5, "cpu").numpy(), R.draw_seeds(77, 0, 5))


def test_excitation_terms():
    N = 640
    f0 = np.full((1, 5), 110.0, np.float32)
    pos, per, count = R.pulses(f0, None, [N], N)
    e0 = R.excite(f0, pos, per, count, [3], [N], N, 0.0)[0]
    A = np.float32(np.sqrt(per[0, 0] * 2.0 ** -16))
    assert e0[0] == A and e0[1] == 0.0                       # phi = 0: one term
    n1, frac = int(pos[0, 1]) >> 16, int(pos[0, 1]) & 0xffff
    phi = np.float32(frac * 2.0 ** -16)
    assert e0[n1] == np.float32(A * np.float32(np.float32(1) - phi)) and e0[n1 + 1] == np.float32(A * phi)
    assert np.count_nonzero(e0) == 1 + 2 * (int(count[0]) - 1)
    # unit mean power of the pulse train, over whole periods
    span = int(pos[0, 4]) >> 16
    assert abs(float((e0[:span].astype(np.float64) ** 2).sum()) / span - 1.0) < 0.5
    # aspiration scales the noise of a voiced frame; an unvoiced frame has it at 1
    e3 = R.excite(f0, pos, per, count, [3], [N], N, 0.3)[0]
    quiet = np.ones(N, bool)
    for s in pos[0, :count[0]]:
        quiet[int(s) >> 16] = quiet[min((int(s) >> 16) + 1, N - 1)] = False
    assert np.array_equal(e3[quiet], (np.float32(0.3) * R.noise(3, N))[quiet])
    un = R.excite(np.zeros((1, 5), np.float32), *R.pulses(np.zeros((1, 5), np.float32), None, [N], N), [3], [500], N,
                  0.3)[0]
    assert np.array_equal(un[:500], R.noise(3, N)[:500]) and not un[500:].any()


# ---- the GPU test's inputs ------------------------------------------------------------------------------
def test_gpu_inputs_leave_no_frame_near_a_decision():
    """checked before tests/test_srcfilt_gpu.py relies on it: no frame near a decision, no sample left out, no
    fallback; the status-3 frames are where the test expects them; 16 C stays under a quarter of an fp32 rounding"""
    for name, asp in R.SYNTH_CASES:
        ref = R.case_ref(name, asp)
        wav, nv, _ = R.waves()[name]
        assert ref.status.shape == (wav.shape[0], M.n_frames(wav.shape[1]))
        assert not ref.near.any() and not ref.left_out.any(), (name, asp)
        assert not (ref.status == R.FALLBACK).any(), (name, asp)
        assert np.isfinite(ref.out).all()
    odd0, odd3 = R.case_ref("odd", 0.0), R.case_ref("odd", 0.3)
    assert (odd0.status[2, 7] == R.UNEXCITED) and (odd3.status[2, 7] == R.OK)      # [960, 1280): no pulse, no noise
    assert int(odd0.pos_q[2, odd0.count[2] - 1]) >> 16 == 906
    assert (odd0.status[2, 8:] == R.SILENT).all() and (odd0.status[0, :11] == R.OK).all()
    assert (odd0.status[1] == R.OK).all()                    # (its gap is unvoiced: noise at full level)
    # row 0's last frame, [1600, 1920): the only excitation in it is the second term of the pulse at 1599.99994, on
    # sample 1600, where the window is exactly 0 -- Ee = 0, another frame without excitation
    assert odd0.status[0, 11] == R.UNEXCITED and int(odd0.pos_q[0, 12]) >> 16 == 1599 and odd0.count[0] == 13
    assert (odd3.status != R.UNEXCITED).all()
    empty = R.case_ref("empty_row", 0.3)
    assert (empty.status[0] == R.SILENT).all() and not empty.out[0].any() and empty.gain[0] == 1.0
    assert empty.count.tolist() == [0, 0] and (empty.status[1] == R.OK).all()      # an all-unvoiced row: noise alone
    for b in (0, 1):
        n = int(odd3.n_valid[b])
        np.testing.assert_allclose(np.sum(odd3.out[b, :n] ** 2), np.sum(odd3.x[b, :n] ** 2), rtol=1e-12)
    long = R.case_ref("long", 0.3)
    assert R.voiced(R.track("long", 31)).sum() >= 25 and long.count[0] >= 40


def test_recorded_figures_match_the_restatement():
    """profiles/srcfilt_delta.json is what tools/srcfilt_delta.py measures; C is recomputed here"""
    rec = R.load_delta()
    c = R.measure_c()
    print("C recomputed", c, "recorded", rec["c"])
    assert rec["c_factor"] == R.C_FACTOR
    assert set(c) | {"worst"} == set(rec["c"])
    assert rec["c"]["worst"] == max(rec["c"][k] for k in c)
    assert max(c.values()) == pytest.approx(rec["c"]["worst"], rel=0.5)
    assert R.C_FACTOR * rec["c"]["worst"] < R.U / 4.0
    assert set(rec["near"]) == {f"{n}_{a:g}" for n, a in R.SYNTH_CASES}
    assert all(v["near_frames"] == 0 and v["left_out_share"] == 0.0 and v["status"][2] == 0
               for v in rec["near"].values())
    assert rec["near"]["odd_0"]["status"][3] >= 1
    for label in ("own", "170"):
        e = rec["e2e"][label]
        assert len(e["f0_rel"]) == len(e["peak_hz"]) == 3
        assert e["f0_rel_worst"] == max(e["f0_rel"]) and e["peak_hz_worst"] == max(e["peak_hz"])
        assert e["f0_rel_worst"] < 0.05 and e["peak_hz_worst"] < 100.0
    assert all(abs(f - R.TARGET_HZ) < 0.1 for f in rec["e2e"]["170"]["f0_out_hz"])


# ---- refusals, before any device is touched ------------------------------------------------------------
@pytest.mark.parametrize("settings, word", [
    ({"resynth": 3}, "--resynth 3: true or false"),
    ({"resynth": True, "aspiration": 1.5}, "--aspiration 1.5: the level between 0 and 1"),
    ({"resynth": True, "aspiration": -0.1}, "--aspiration -0.1: the level between 0 and 1"),
    ({"resynth": True, "aspiration": "x"}, "--aspiration x: the level"),
    ({"resynth": True, "aspiration": True}, "--aspiration True: the level"),
    ({"resynth": True, "aspiration": float("nan")}, "--aspiration nan: the level"),
    ({"resynth": True, "resynth_pitch_hz": 500.0}, "--resynth_pitch_hz 500: a target between 60 and 400 Hz"),
    ({"resynth": True, "resynth_pitch_hz": 20}, "--resynth_pitch_hz 20: a target between 60 and 400 Hz"),
    ({"resynth": True, "resynth_pitch_hz": "x"}, "--resynth_pitch_hz nan: a target"),
    ({"resynth": True, "resynth_pitch_hz": True}, "--resynth_pitch_hz True: a target"),
    ({"resynth": True, "f0_method": "pyin"}, "--f0_method pyin"),
    ({"resynth_options": {"seed": -1}}, "seed -1: a whole number"),
    ({"resynth_options": {"seed": 1.5}}, "seed 1.5: a whole number"),
    ({"resynth_options": {"r_min": 0.4}}, "r_min 0.4"),
    ({"resynth_options": {"min_voiced": 0}}, "min_voiced 0: a count of frames"),
])
def test_check_resynth_options_refuses_in_one_line(settings, word):
    from speech_anonymization_amd import sourcefilter
    with pytest.raises(SystemExit) as e:
        sourcefilter.check_resynth_options(settings)
    assert word in str(e.value) and "\n" not in str(e.value)


def test_check_resynth_options_returns_the_constructor_arguments():
    from speech_anonymization_amd import sourcefilter
    default = {"pitch_target_hz": None, "aspiration": 0.3, "seed": 1, "f0_method": "yin", "level": True, "r_min": 0.5,
               "r_max": 2.0, "min_voiced": 5}
    assert sourcefilter.check_resynth_options({"resynth": True}) == default
    got = sourcefilter.check_resynth_options({"resynth": True, "resynth_pitch_hz": 170, "aspiration": 0,
                                              "f0_method": "viterbi"})
    assert got == dict(default, pitch_target_hz=170.0, aspiration=0.0, f0_method="viterbi")
    block = {"pitch_target_hz": 150.0, "aspiration": 0.1, "seed": 9, "level": False, "r_min": 0.6, "min_voiced": 3}
    got = sourcefilter.check_resynth_options({"resynth_options": block, "aspiration": 0.2})
    assert got == dict(default, pitch_target_hz=150.0, aspiration=0.2, seed=9, level=False, r_min=0.6, min_voiced=3)
    sf = sourcefilter.SourceFilter(**got)                     # and the class takes them
    assert sf.pitch_target_hz == 150.0 and sf.aspiration == 0.2 and sf.last is None
    for bad in (dict(aspiration=2), dict(pitch_target_hz=1000), dict(seed=-1), dict(f0_method="x"), dict(r_min=0.1),
                dict(min_voiced=0)):
        with pytest.raises(ValueError):
            sourcefilter.SourceFilter(**bad)


BASE = {"out_dir": "o", "synthetic": 2}


@pytest.mark.parametrize("settings, word", [
    ({"resynth": True, "mcadams": 0.8}, "--resynth true and --mcadams exclude each other"),
    ({"resynth": True, "formant_norm": True}, "--resynth true and --formant_norm exclude each other"),
    ({"resynth": True, "formant_norm_ratio": 0.9}, "--resynth true and --formant_norm exclude each other"),
    ({"resynth": True, "recon_ckpt": "d"}, "--resynth true and --recon_ckpt exclude each other"),
    ({"resynth": True, "passthrough": True}, "--resynth true and --passthrough true exclude each other"),
    ({"resynth": True, "formant_ratio": 1.1}, "--resynth true and --formant_ratio exclude each other"),
    ({"resynth": True, "preserve_formants": True}, "--resynth true and --preserve_formants true exclude"),
    ({"resynth": True, "pitch_norm": True}, "--resynth true and --pitch_norm true exclude each other"),
    ({"resynth": True, "pitch_target_hz": 150.0}, "--resynth true takes no --pitch_target_hz"),
    ({"resynth": True, "phase": "vocoder"}, "--resynth true and --phase exclude each other"),
    ({"resynth": True, "psola": True}, "--resynth true takes no --psola"),
    ({"resynth": True, "contour_scale": 0.5}, "--resynth true takes no --contour_scale"),
    ({"resynth": True, "lifter": 30}, "--resynth true takes no --lifter"),
    ({"resynth": True, "formant_target": "600,1350,2500"}, "--resynth true takes no --formant_target"),
    ({"resynth": True, "aspiration": 7}, "--aspiration 7"),
    ({"resynth": True, "hip_graph": True}, "anonymize does not support --hip_graph"),
    ({"resynth": "yes"}, "--resynth yes: true or false"),
    ({"aspiration": 0.3}, "--aspiration goes with --resynth true"),
    ({"resynth_pitch_hz": 170}, "--resynth_pitch_hz goes with --resynth true"),
    ({"resynth": False, "aspiration": 0.3}, "--aspiration goes with --resynth true"),
    ({"mcadams": 0.8, "resynth_pitch_hz": 170}, "--resynth_pitch_hz goes with --resynth true"),
])
def test_anonymize_refuses_in_one_line(settings, word):
    from speech_anonymization_amd import vocoder
    with pytest.raises(SystemExit) as e:
        vocoder.check_anonymize_options(dict(BASE, **settings), {}, {})
    assert word in str(e.value) and "\n" not in str(e.value)


def test_anonymize_accepts_the_mode_and_leaves_the_others_alone():
    from speech_anonymization_amd import vocoder
    for extra in ({}, {"resynth_pitch_hz": 170}, {"aspiration": 0.0}, {"f0_method": "viterbi"}, {"seed": 5},
                  {"report_f0": True, "report_stoi": True, "report_prosody": True, "report_mcd": True,
                   "report_formants": True}, {"n_iter": 2}):
        s = dict(BASE, resynth=True, **extra)
        vocoder.check_anonymize_options(s, {}, {})
        assert vocoder.anonymize_mode(s) == "resynth"
    assert vocoder.anonymize_mode(dict(BASE, mcadams=0.8)) == "mcadams"
    assert vocoder.anonymize_mode(dict(BASE, resynth=False, passthrough=True)) == "passthrough"


@pytest.mark.parametrize("run_opts, settings, environ, word", [
    ({"distributed_launch": True}, {}, {}, "gender_classifier_train_resynth runs on one GPU"),
    ({}, {}, {"WORLD_SIZE": "2"}, "gender_classifier_train_resynth runs on one GPU"),
    ({}, {"hip_graph": True}, {}, "gender_classifier_train_resynth does not support --hip_graph"),
    ({"hip_graph": True}, {}, {}, "gender_classifier_train_resynth does not support --hip_graph"),
    ({}, {"aspiration": 3}, {}, "--aspiration 3"),
])
def test_recipe_refuses_in_one_line(run_opts, settings, environ, word):
    from speech_anonymization_amd import sourcefilter
    with pytest.raises(SystemExit) as e:
        sourcefilter.check_recipe_options(settings, run_opts, environ)
    assert word in str(e.value) and "\n" not in str(e.value)


def test_recipe_settings_file_gives_the_defaults():
    from speech_anonymization_amd import sourcefilter
    from speech_anonymization_amd.yaml_loader import load_plain
    with open(os.path.join(ROOT, "speechbrain_configs", "gender_classifier_resynth.yaml")) as f:
        settings = load_plain(f, {})
    assert sourcefilter.check_recipe_options(settings, {}, {}) == sourcefilter.check_resynth_options({})
    with open(os.path.join(ROOT, "speechbrain_configs", "gender_classifier_resynth.yaml")) as f:
        settings = load_plain(f, {"resynth_pitch_hz": 170, "f0_method": "viterbi"})
    got = sourcefilter.check_recipe_options(settings, {}, {})
    assert got["pitch_target_hz"] == 170.0 and got["f0_method"] == "viterbi"


def test_ops_refuse_before_the_library_is_loaded(monkeypatch):
    """CPU tensors, wrong dtypes, strides and shapes: one line each, and load() is never reached"""
    import torch
    from speech_anonymization_amd import _lib, ops
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    f0 = torch.zeros(2, 11)
    nv = torch.zeros(2, dtype=torch.int32)
    S = _lib.SaHipError
    for call in (lambda: ops.srcfilt_pulses(f0, None, nv, N=1600),
                 lambda: ops.srcfilt_excite(f0, f0, f0, nv, nv, nv, N=1600),
                 lambda: ops.srcfilt_synth(torch.zeros(2, 1600), torch.zeros(2, 1600), nv),
                 lambda: ops.srcfilt(torch.zeros(2, 1600), f0, None, nv, nv)):
        with pytest.raises(S, match="GPU tensors") as e:
            call()
        assert "\n" not in str(e.value)


# ---- the ABI ----------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_names():
    from speech_anonymization_amd import _lib
    src = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = ["sa_srcfilt_dim", "sa_srcfilt_pulses", "sa_srcfilt_excite", "sa_srcfilt_synth"]
    for name in names:
        assert re.search(r"^\s*int\s+%s\s*\(" % name, plain, flags=re.M), name
        assert name in _lib.SYMBOLS
    assert re.search(r"^\s*long long\s+sa_srcfilt_workspace_bytes\s*\(int B, int N\)", plain, flags=re.M)
    assert re.search(r"int sa_srcfilt_pulses\(const float\* f0, const int\* rho_q, const int\* n_valid, int B, int N, "
                     r"int T,\s+long long\* pos_q,\s+int\* period_q, int\* count, void\* stream\);", plain)
    for word in ("0x7feb352d", "0x846ca68b", "Kcap = N / 40 + 2", "266 2^16", "Ee < 1e-20", "section 27"):
        assert word in src, word
    mk = open(os.path.join(ROOT, "speech-anonymization_amd", "csrc", "Makefile")).read()
    assert "sa_srcfilt.hip" in mk


def test_library_exports_the_entry_points_and_their_constants():
    """the built library, no GPU: the constants the restatement and ops assume, the workspace size, the refusals
    that come before any launch"""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from speech_anonymization_amd import _lib, ops
    lib = _lib.load()
    assert [lib.sa_srcfilt_dim(i) for i in range(10)] == [R.W, R.H, R.P, 64, 4096, R.TMIN, R.TMAX, R.KDIV, 256, 8]
    assert lib.sa_srcfilt_dim(10) == -22 and lib.sa_srcfilt_dim(-1) == -22
    assert ops.SRCFILT_KDIV == R.KDIV and ops.SRCFILT_RHO_ONE == R.ONE and ops.SRCFILT_MAX_N == 1 << 24
    for B, N in ((1, 1), (3, 1687), (32, 160000)):
        T = M.n_frames(N)
        assert lib.sa_srcfilt_workspace_bytes(B, N) == 4 * B * T * 320 + 8 * (2 * B * (-(-N // 4096)) + B)
    for B, N in ((0, 10), (65536, 10), (1, 0), (1, (1 << 24) + 1)):
        assert lib.sa_srcfilt_workspace_bytes(B, N) == -22
    one = ctypes.c_void_p(8)                                 # never dereferenced: every call is refused first
    bad_T = 9
    assert lib.sa_srcfilt_pulses(one, None, one, 1, 1600, bad_T, one, one, one, None) == -22
    assert lib.sa_srcfilt_pulses(None, None, one, 1, 1600, 11, one, one, one, None) == -22
    assert lib.sa_srcfilt_pulses(one, None, one, 0, 1600, 11, one, one, one, None) == -22
    assert lib.sa_srcfilt_pulses(one, None, one, 1, (1 << 24) + 1, 104859, one, one, one, None) == -22
    for asp in (-0.1, 1.5, float("nan")):
        assert lib.sa_srcfilt_excite(one, one, one, one, one, one, 1, 1600, 11, ctypes.c_float(asp), one, None) == -22
    assert lib.sa_srcfilt_excite(one, one, one, one, None, one, 1, 1600, 11, ctypes.c_float(0.3), one, None) == -22
    assert lib.sa_srcfilt_synth(one, None, one, 1, 1600, 1, one, one, None, None, None) == -22
    assert lib.sa_srcfilt_synth(one, one, one, 65536, 1600, 1, one, one, None, None, None) == -22
