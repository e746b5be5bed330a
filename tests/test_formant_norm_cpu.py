"""CPU checks of the LPC formant normalisation: the fp64 restatement's own identities, the
properties of the angle map, the conditioning of the inputs the GPU test compares on, the recorded figures held to
the restatement, the one-line refusals, the symbol list and the entry points' -EINVAL -- nothing here needs a GPU."""
import ctypes
import errno
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import formantnorm_ref as R
from tests import lpcformant_ref as LF
from tests import mcadams_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ----------------------------------------------------------------------------------------
def test_restatement_reproduces_its_input_at_ratio_one():
    """q phi = phi, a' = a, IIR(1 / a) FIR(a) = identity, and w^2 sums to 1 at hop 160 (the window identity)"""
    wav = np.stack([M.voiced_row(130.0, M.FORMANTS, 1687, 7), M.voiced_row(220.0, M.FORMANTS, 1687, 8)])
    nv = np.array([1687, 1200])
    out = R.pole_warp(wav, np.ones(2, np.float32), nv, level=False, copy_unity=False)
    assert (out.status[0] == R.OK).all() and out.below[0] > 0 and out.above[0] > 0           # both branches, both the identity
    live = np.arange(1687)[None, :] < nv[:, None]
    x = np.asarray(wav, np.float32).astype(np.float64)
    err = np.abs(out.out - np.where(live, x, 0.0)).max()
    print("identity error", err)
    assert err <= 1e-9
    np.testing.assert_array_equal(out.out[1, 1200:], 0.0)
    copied = R.pole_warp(wav, np.ones(2, np.float32), nv)
    np.testing.assert_array_equal(copied.out, np.where(live, x, 0.0))      # q = 1: copied, not transformed
    assert (copied.gain == 1.0).all() and not copied.status.any()


@pytest.mark.parametrize("q", [0.5, 0.8, 0.85, 1.0, 1.15, 1.2, 1.3, 2.0])
def test_the_map_is_monotone_continuous_and_onto(q):
    phi0 = R.knee(q)
    assert phi0 == 0.85 * math.pi * min(1.0, 1.0 / q) and 0.0 < phi0 < math.pi
    assert R.warp_angle(0.0, q) == 0.0 and R.warp_angle(math.pi, q) == pytest.approx(math.pi, abs=4e-16)
    grid = np.unique(np.concatenate([np.linspace(0.0, math.pi, 4001), [phi0]]))
    v = np.array([R.warp_angle(p, q) for p in grid])
    assert (np.diff(v) > 0).all() and v[0] == 0.0 and v[-1] <= math.pi + 4e-16               # strictly increasing
    before, after = (R.warp_angle(np.nextafter(phi0, to), q) for to in (0.0, 4.0))           # continuous at the knee:
    assert before <= R.warp_angle(phi0, q) <= after and after - before <= 4e-15               # one ulp moves it by ulps
    assert R.warp_angle(phi0, q) == q * phi0 and q * phi0 < math.pi
    below = grid[grid <= phi0]
    np.testing.assert_array_equal(v[:below.shape[0]], q * below)            # exactly q phi up to the knee
    if q <= 1.2:                                                            # every resonance up to 5667 Hz scaled by q
        assert phi0 * R.SR / (2.0 * math.pi) >= 5666.0 > LF.F_HIGH


def test_a_known_pole_pair_moves_to_q_phi():
    """one resonance below the knee and one above it: the rebuilt polynomial has them at the mapped angles, moduli
    kept, and counts them on either side"""
    q, lo, hi = 1.15, (0.6, 0.95), (2.9, 0.9)
    z = np.concatenate([[m * np.exp(s * 1j * p) for p, m in (lo, hi) for s in (1, -1)],
                        0.3 * np.exp(2j * np.pi * (np.arange(16) + 0.5) / 16)])
    a2, ok, _, below, above = R.rebuild(np.roots(np.real(np.poly(z))), q)
    assert ok and below + above == 10 and above >= 1
    got = np.roots(a2)
    for (p, m), want in ((lo, q * 0.6), (hi, R.warp_angle(2.9, q))):
        near = got[np.argmin(np.abs(got - m * np.exp(1j * want)))]
        assert abs(abs(near) - m) < 1e-9 and abs(np.angle(near) - want) < 1e-9
    assert R.warp_angle(2.9, q) > 2.9 and R.warp_angle(2.9, 0.85) < 2.9 and R.warp_angle(2.9, 0.85) > 0.85 * 2.9


def test_q_is_sanitised_as_the_kernel_does():
    got = R.sanitize_q(np.array([0.3, 3.0, np.nan, 0.85, 1.0], np.float32))
    np.testing.assert_array_equal(got, np.array([0.5, 2.0, 1.0, np.float32(0.85), 1.0], np.float64))


def test_centre_on_a_small_case():
    freq = np.array([[[500.0, 1500.0, 2500.0], [520.0, 1400.0, 2600.0], [480.0, 1600.0, 2400.0],
                      [9.0, 9.0, 9.0]]], np.float32)
    status = np.array([[0, 0, 0, 2]], np.int32)
    f0 = np.array([[100.0, 100.0, 100.0, 100.0]], np.float32)
    c = R.centre(freq, status, f0, [4], (500.0, 1500.0, 2500.0), min_frames=3)
    assert c.count.tolist() == [3] and c.med.tolist() == [[500.0, 1500.0, 2500.0]] and c.q.tolist() == [1.0]
    c = R.centre(freq, status, f0, [2], (550.0, 1650.0, 2750.0), min_frames=2)               # lower median of two
    assert c.count.tolist() == [2] and c.med.tolist() == [[500.0, 1400.0, 2500.0]]
    assert c.q64[0] == pytest.approx((1.1 * 1650.0 / 1400.0 * 1.1) ** (1.0 / 3.0), rel=1e-15)
    assert R.centre(freq, status, f0, [4], (1000.0, 3000.0, 5000.0), min_frames=3).q.tolist() == [np.float32(1.2)]
    assert R.centre(freq, status, f0, [4], (250.0, 750.0, 1250.0), min_frames=3).q.tolist() == [np.float32(0.8)]
    c = R.centre(freq, status, f0, [4], (500.0, 1500.0, 2500.0), min_frames=4)
    assert c.count.tolist() == [0] and c.q.tolist() == [1.0] and not c.med.any()
    f0[0, 1] = 0.0
    assert R.centre(freq, status, f0, [9], (500.0, 1500.0, 2500.0), min_frames=1).count.tolist() == [2]
    assert R.centre(freq, status, None, [9], (500.0, 1500.0, 2500.0), min_frames=1).count.tolist() == [3]


# ---- the GPU test's inputs and the recorded figures ---------------------------------------------------------
@pytest.mark.parametrize("level", [True, False])
def test_gpu_cases_are_well_conditioned(level):
    """checked before any GPU comparison: on every case the restatement leaves out no sample (the cap is 1 %), flags
    no fallback, takes both branches of the map in every transformed row, and the recorded C leaves the bar under a
    quarter of an fp32 rounding"""
    assert R.C_FACTOR * R.C_MEASURED <= R.U / 4
    assert [c[0] for c in R.gpu_cases()] == ["odd", "two_frames", "empty_row", "synthetic", "zero_row"]
    assert [c[1].shape for c in R.gpu_cases()[:4]] == [c[1].shape for c in M.gpu_cases()]
    for name, wav, q, nv in R.gpu_cases():
        ref = R.case_ref(name, level)
        assert ref.left_out.mean() <= 0.01 and not ref.near.any(), name
        assert not (ref.status == R.FALLBACK).any(), name
        assert ref.status.shape == (wav.shape[0], M.n_frames(wav.shape[1]))
        for b in range(wav.shape[0]):
            if ref.q[b] != 1.0 and (ref.status[b] == R.OK).any():
                assert ref.below[b] > 0 and ref.above[b] > 0, (name, b)
    odd = R.case_ref("odd", level)
    assert odd.q.tolist() == [float(np.float32(0.85)), 1.0, float(np.float32(1.15))]
    assert (odd.status[0] == R.OK).all() and (odd.status[1] == 0).all()
    assert (odd.status[2, 8:] == R.SILENT).all() and (odd.status[2, :6] == R.OK).all()
    np.testing.assert_array_equal(odd.out[1], odd.x[1])                     # q = 1: copied
    empty = R.case_ref("empty_row", level)
    assert (empty.status[0] == R.SILENT).all() and not empty.out[0].any() and empty.gain[0] == 1.0
    zero = R.case_ref("zero_row", level)
    assert (zero.status[0] == R.SILENT).all() and not zero.out[0].any() and zero.gain[0] == 1.0
    if level:
        for b in (0, 2):
            n = int(odd.n_valid[b])
            np.testing.assert_allclose(np.sum(odd.out[b, :n] ** 2), np.sum(odd.x[b, :n] ** 2), rtol=1e-12)
    else:
        assert (odd.gain == 1.0).all()


def test_recorded_figures_match_the_restatement():
    """profiles/formant_norm_delta.json is what tools/formant_norm_delta.py measures, and the constants of the GPU
    test's bars are its figures (the spread re-measured on one case here, to stay quick)"""
    rec = R.recorded()
    assert rec["factor"] == R.C_FACTOR
    assert rec["spread_rel"] <= R.C_MEASURED <= 1.25 * rec["spread_rel"]
    assert set(rec["per_case"]) == {c[0] for c in R.gpu_cases()}
    assert all(v["near_frames"] == 0 and v["left_out_share"] <= 0.01 for v in rec["per_case"].values())
    name, wav, q, nv = R.gpu_cases()[0]
    ref = R.case_ref(name, True)
    ab = R.pole_warp(wav, q, nv, True, roots=M.aberth)
    rv = R.pole_warp(wav, q, nv, True, reverse_acf=True)
    assert (ab.status == ref.status).all() and (rv.status == ref.status).all()
    peak = np.abs(ref.out).max(1, keepdims=True)
    c = max((np.abs(ab.out - ref.out) / peak).max(), (np.abs(rv.out - ref.out) / peak).max())
    print("C on the first case", c, "recorded", rec["per_case"][name]["out_rel"])
    assert c == pytest.approx(rec["per_case"][name]["out_rel"], rel=0.5) and c <= R.C_MEASURED
    assert rec["per_case"][name]["below_knee"] == ref.below.tolist()
    assert rec["per_case"][name]["above_knee"] == ref.above.tolist()
    # the end-to-end figures: shapes, and the facts the GPU test relies on
    assert set(rec["open"]) == {str(q) for q in R.E2E_RATIOS} | {"input"}
    for q in R.E2E_RATIOS:
        o = rec["open"][str(q)]
        assert min(o["common"]) >= 8 and o["near"] == 0 and o["fallback_frames"] == 0
        assert np.array(o["distance"]).max(0).tolist() == o["worst"] and max(o["worst"]) < 0.05
        assert all(abs(s / q - 1.0) < 0.02 for s in o["shift"])
    cl = rec["closed"]
    assert cl["target_hz"] == list(R.CLOSED_TARGET) and [r[2] for r in cl["rows"]] == [0.9, 1.12]
    assert min(cl["count_before"] + cl["count_after"]) >= 8 and cl["near"] == 0 and cl["fallback_frames"] == 0
    for b in range(2):
        assert abs(math.log(cl["distance_after"][b])) == pytest.approx(cl["abs_ln_after"][b], rel=1e-12)
        assert cl["abs_ln_after"][b] < 0.01 < abs(math.log(cl["distance_before"][b]))
        assert 0.8 < cl["q"][b] < 1.2


def test_closed_loop_first_half_matches_the_recorded_figures():
    """the tracks, medians and q of the closed loop's two rows, recomputed (the pole warp itself is left to the tool)"""
    rows = R.closed_rows()
    B, N = rows.shape
    T = LF.n_frames(N)
    tr = LF.tracks(rows, np.full(B, N, np.int32))
    c = R.centre(tr.freq.astype(np.float32), tr.status, R.closed_f0(T), np.full(B, T, np.int32), R.CLOSED_TARGET)
    rec = R.recorded()["closed"]
    assert c.count.tolist() == rec["count_before"] and c.q.astype(float).tolist() == rec["q"]
    assert c.med.astype(float).tolist() == rec["median_before_hz"]


# ---- refusals, before any device is touched ------------------------------------------------------------
@pytest.mark.parametrize("settings, word", [
    ({"formant_norm": 3}, "--formant_norm 3: true or false"),
    ({"formant_norm": False, "formant_norm_ratio": 0.9}, "--formant_norm false and --formant_norm_ratio X exclude"),
    ({"formant_norm_ratio": 0.7}, "--formant_norm_ratio 0.7: a ratio between 0.8 and 1.2"),
    ({"formant_norm_ratio": 1.3}, "--formant_norm_ratio 1.3: a ratio between 0.8 and 1.2"),
    ({"formant_norm_ratio": "x"}, "--formant_norm_ratio x: a ratio"),
    ({"formant_norm_ratio": True}, "--formant_norm_ratio True: a ratio"),
    ({"formant_norm": True, "formant_target": "600,1350"}, "--formant_target 600,1350: three frequencies F1,F2,F3"),
    ({"formant_norm": True, "formant_target": "600,500,2500"}, "--formant_target 600,500,2500: three frequencies"),
    ({"formant_norm": True, "formant_target": "50,1350,2500"}, "90 <= F1 < F2 < F3 <= 5500"),
    ({"formant_norm": True, "formant_target": "600,1350,6000"}, "90 <= F1 < F2 < F3 <= 5500"),
    ({"formant_norm": True, "formant_target": "a,b,c"}, "--formant_target a,b,c: three frequencies"),
    ({"formant_norm": True, "formant_target": 600}, "--formant_target 600: three frequencies"),
    ({"formant_norm_ratio": 0.9, "formant_target": "600,1350,2500"}, "--formant_norm_ratio X and --formant_target"),
    ({"formant_norm_ratio": 0.9, "formant_q_min": 0.9}, "--formant_norm_ratio X leaves nothing to bound"),
    ({"formant_norm": True, "formant_q_min": 0.7}, "--formant_q_min 0.7: a ratio between 0.8 and 1"),
    ({"formant_norm": True, "formant_q_min": 1.1}, "--formant_q_min 1.1: a ratio between 0.8 and 1"),
    ({"formant_norm": True, "formant_q_max": 0.9}, "--formant_q_max 0.9: a ratio between 1 and 1.2"),
    ({"formant_norm": True, "formant_q_max": 1.3}, "--formant_q_max 1.3: a ratio between 1 and 1.2"),
    ({"formant_norm": True, "f0_method": "pyin"}, "--f0_method pyin"),
    ({"formant_norm": {"min_frames": 0}}, "min_frames 0: a count of frames"),
    ({"formant_norm": {"ratio": 0.9, "target_hz": [600, 1350, 2500]}},
     "ratio and target_hz exclude each other"),
])
def test_check_formant_norm_options_refuses_in_one_line(settings, word):
    from speech_anonymization_amd import formantnorm
    with pytest.raises(SystemExit) as e:
        formantnorm.check_formant_norm_options(settings)
    assert word in str(e.value) and "\n" not in str(e.value)


def test_check_formant_norm_options_returns_the_constructor_arguments():
    from speech_anonymization_amd import formantnorm
    default = {"level": True, "target_hz": (550.0, 1650.0, 2750.0), "q_min": 0.8, "q_max": 1.2, "min_frames": 8,
               "f0_method": "yin"}
    assert formantnorm.check_formant_norm_options({"formant_norm": True}) == default
    assert formantnorm.check_formant_norm_options({}) == default
    got = formantnorm.check_formant_norm_options({"formant_norm": True, "formant_target": "600,1350,2500",
                                                  "formant_q_min": 0.9, "formant_q_max": 1.1, "f0_method": "viterbi"})
    assert got == dict(default, target_hz=(600.0, 1350.0, 2500.0), q_min=0.9, q_max=1.1, f0_method="viterbi")
    assert formantnorm.check_formant_norm_options({"formant_norm_ratio": 0.9}) == dict(default, ratio=0.9)
    block = {"formant_norm": {"target_hz": [600, 1350, 2500], "q_min": 0.85, "min_frames": 12, "level": False,
                                      "f0_method": "viterbi"}}
    got = formantnorm.check_formant_norm_options(block)
    assert got == {"level": False, "target_hz": (600.0, 1350.0, 2500.0), "q_min": 0.85, "q_max": 1.2, "min_frames": 12,
                   "f0_method": "viterbi"}
    assert formantnorm.check_formant_norm_options(dict(block, formant_norm_ratio=1.1))["ratio"] == 1.1   # a flag outranks
    assert formantnorm.check_formant_norm_options(dict(block, formant_q_min=0.9))["q_min"] == 0.9
    assert formantnorm.check_formant_norm_options({"formant_norm": {"ratio": 0.9}})["ratio"] == 0.9
    fn = formantnorm.FormantNormalizer(**got)
    assert fn.target_hz == (600.0, 1350.0, 2500.0) and fn.ratio is None and fn.min_frames == 12 and fn.last is None
    assert formantnorm.FormantNormalizer().target_hz == formantnorm.TARGET_DEFAULT == R.TARGET_DEFAULT
    for kw in (dict(ratio=0.7), dict(ratio=1.3), dict(target_hz=(600.0, 1350.0)), dict(target_hz=(600.0, 500.0, 2500.0)),
               dict(q_min=0.7), dict(q_min=1.1), dict(q_max=1.3), dict(min_frames=0), dict(min_frames=2.5)):
        with pytest.raises(ValueError, match="FormantNormalizer"):
            formantnorm.FormantNormalizer(**kw)
    with pytest.raises(ValueError, match="f0_method"):
        formantnorm.FormantNormalizer(f0_method="pyin")


BASE = {"out_dir": "o", "synthetic": 4, "formant_norm": True}


@pytest.mark.parametrize("change, word", [
    ({"mcadams": 0.8}, "--formant_norm and --mcadams exclude each other"),
    ({"mcadams_min": 0.6, "mcadams_max": 0.9}, "--formant_norm and --mcadams exclude each other"),
    ({"recon_ckpt": "d"}, "--formant_norm and --recon_ckpt exclude each other"),
    ({"passthrough": True}, "--formant_norm and --passthrough true exclude each other"),
    ({"formant_ratio": 1.1}, "--formant_norm and --formant_ratio exclude each other"),
    ({"preserve_formants": True, "pitch_norm": True}, "--formant_norm and --preserve_formants true exclude each other"),
    ({"phase": "vocoder"}, "--formant_norm and --phase exclude each other"),
    ({"phase": "griffin_lim"}, "--formant_norm and --phase exclude each other"),
    ({"pitch_norm": True}, "--formant_norm true with --pitch_norm true needs --psola true"),
    ({"pitch_norm": True, "psola": False}, "--formant_norm true with --pitch_norm true needs --psola true"),
    ({"psola": True}, "--psola true goes with --pitch_norm true"),
    ({"pitch_norm": True, "psola": True, "pitch_target_hz": 900.0}, "--pitch_target_hz 900"),
    ({"formant_norm_ratio": 1.4}, "--formant_norm_ratio 1.4: a ratio"),
    ({"formant_target": "1,2,3"}, "--formant_target 1,2,3: three frequencies"),
    ({"lifter": 20}, "--lifter goes with"),
    ({"out_dir": None}, "--out_dir OUT is required"),
    ({"hip_graph": True}, "anonymize does not support --hip_graph"),
    ({"formant_norm": None, "formant_target": "600,1350,2500", "mcadams": 0.8},
     "--formant_target goes with --formant_norm true"),
    ({"formant_norm": False, "formant_q_min": 0.9, "pitch_norm": True}, "--formant_q_min goes with --formant_norm true"),
    ({"formant_norm": None, "formant_q_max": 1.1, "passthrough": True, "model_type": "convae"},
     "--formant_q_max goes with --formant_norm true"),
])
def test_check_anonymize_options_formant_norm_branches(change, word):
    from speech_anonymization_amd import vocoder
    with pytest.raises(SystemExit) as e:
        vocoder.check_anonymize_options(dict(BASE, **change), {}, {})
    assert word in str(e.value) and "\n" not in str(e.value)


def test_check_anonymize_options_lets_the_mode_through_and_keeps_the_others():
    from speech_anonymization_amd import vocoder
    ok = vocoder.check_anonymize_options
    ok(dict(BASE), {"device": "cuda:0"}, {})                                # no model_type: no model runs
    ok({"out_dir": "o", "synthetic": 2, "formant_norm_ratio": 0.9}, {}, {})              # the ratio implies the mode
    assert vocoder.anonymize_mode({"formant_norm_ratio": 0.9}) == "formant_norm"
    assert vocoder.anonymize_mode({"formant_norm": True, "pitch_norm": True}) == "formant_norm"
    assert vocoder.anonymize_mode({"formant_norm": False, "pitch_norm": True}) == "pitch_norm"
    ok(dict(BASE, formant_target="600,1350,2500", formant_q_min=0.9, formant_q_max=1.1), {}, {})
    ok(dict(BASE, f0_method="viterbi"), {}, {})                             # accepted with the mode, no report needed
    ok(dict(BASE, formant_norm=None, formant_norm_ratio=1.0, f0_method="yin"), {}, {})
    ok(dict(BASE, pitch_norm=True, psola=True), {}, {})
    ok(dict(BASE, pitch_norm=True, psola=True, pitch_target_hz=150.0, contour_scale=0.5), {}, {})
    for report in ("report_f0", "report_stoi", "report_prosody", "report_mcd", "report_formants"):
        ok(dict(BASE, **{report: True}), {}, {})
    # with none of the new flags, what was refused and accepted is what it was
    with pytest.raises(SystemExit, match="--recon_ckpt DIR is required without --passthrough true"):
        ok(dict(BASE, formant_norm=None, model_type="convae"), {}, {})
    with pytest.raises(SystemExit, match="--f0_method goes with --pitch_norm true or --report_f0 true"):
        ok({"out_dir": "o", "synthetic": 2, "mcadams": 0.8, "f0_method": "viterbi"}, {}, {})
    with pytest.raises(SystemExit, match="--psola true goes with --pitch_norm true"):
        ok({"out_dir": "o", "synthetic": 2, "mcadams": 0.8, "psola": True}, {}, {})
    with pytest.raises(SystemExit, match="--mcadams and --pitch_norm true exclude each other"):
        ok({"out_dir": "o", "synthetic": 2, "mcadams": 0.8, "pitch_norm": True}, {}, {})
    with pytest.raises(SystemExit, match="anonymize runs on one GPU"):
        ok(dict(BASE), {}, {"WORLD_SIZE": "2"})


def test_anonymize_refuses_before_it_touches_a_device(monkeypatch, tmp_path):
    def no_device(*a, **k):
        raise AssertionError("a device was touched")

    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    spec = importlib.util.spec_from_file_location("anonymize", os.path.join(ROOT, "anonymize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "formant_norm" in mod.MODES
    cfg = os.path.join(ROOT, "speechbrain_configs", "convae.yaml")
    for extra, word in ((["--formant_norm", "true", "--passthrough", "true"], "--formant_norm and --passthrough true"),
                        (["--formant_norm_ratio", "1.4"], "--formant_norm_ratio 1.4"),
                        (["--formant_norm", "true", "--formant_target", "600,1350"], "--formant_target 600,1350"),
                        (["--formant_norm", "true", "--pitch_norm", "true"], "needs --psola true"),
                        (["--formant_target", "600,1350,2500", "--mcadams", "0.8"], "goes with --formant_norm true")):
        with pytest.raises(SystemExit) as e:
            mod.main([cfg, "--synthetic", "2", "--out_dir", str(tmp_path / "never")] + extra)
        assert word in str(e.value) and "\n" not in str(e.value)
    assert not (tmp_path / "never").exists()


# ---- the library boundary -------------------------------------------------------------------------------
def _declared():
    """the entry points include/sa_hip.h declares (tests/test_abi.py's pattern)"""
    import re
    src = open(os.path.join(ROOT, "include", "sa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*int\s+(sa_\w+)\s*\(", src, flags=re.M))


def test_symbols_and_dimensions():
    from speech_anonymization_amd import _lib, ops
    new = {"sa_pole_warp_dim", "sa_pole_warp", "sa_formant_centre"}
    assert new <= set(_lib.SYMBOLS) and new <= _declared()
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new)
    assert [lib.sa_pole_warp_dim(i) for i in range(8)] == [320, 160, 20, 1, 64, 64, 4096, 850]
    assert [lib.sa_pole_warp_dim(i) for i in range(7)] == [lib.sa_mcadams_dim(i) for i in range(7)]
    assert lib.sa_pole_warp_dim(8) == -errno.EINVAL and lib.sa_pole_warp_dim(-1) == -errno.EINVAL
    assert (R.W, R.H, R.P, R.KNEE) == (320, 160, 20, 0.85) and ops.PW_KNEE == 0.85
    assert (ops.PW_Q_LOW, ops.PW_Q_HIGH) == (R.Q_LOW, R.Q_HIGH) == (0.5, 2.0)
    assert (ops.FORMANT_F_LOW, ops.FORMANT_F_HIGH) == (LF.F_LOW, LF.F_HIGH)


def test_entry_points_refuse_bad_arguments():
    """-EINVAL before any launch.  The pointers are host buffers nothing dereferences."""
    from speech_anonymization_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p, E, cf = ctypes.cast(buf, ctypes.c_void_p), -errno.EINVAL, ctypes.c_float

    def warp(wav=p, q=p, n_valid=p, B=2, N=1600, level=1, out=p, ws=p, status=None, gain=None):
        return lib.sa_pole_warp(wav, q, n_valid, B, N, level, out, ws, status, gain, None)

    for bad in (dict(wav=None), dict(q=None), dict(n_valid=None), dict(out=None), dict(ws=None), dict(B=0),
                dict(B=-1), dict(B=65536), dict(N=0), dict(N=-5), dict(N=(1 << 30) + 1)):
        assert warp(**bad) == E, bad

    def centre(freq=p, status=p, f0=None, frames=p, B=2, T=20, t=(550.0, 1650.0, 2750.0), lo=0.8, hi=1.2, m=8, q=p):
        return lib.sa_formant_centre(freq, status, f0, frames, B, T, cf(t[0]), cf(t[1]), cf(t[2]), cf(lo), cf(hi), m,
                                     None, q, None, None)

    for bad in (dict(freq=None), dict(status=None), dict(frames=None), dict(q=None), dict(B=0), dict(B=65536),
                dict(T=0), dict(T=104859), dict(t=(80.0, 1650.0, 2750.0)), dict(t=(1650.0, 550.0, 2750.0)),
                dict(t=(550.0, 1650.0, 1650.0)), dict(t=(550.0, 1650.0, 5600.0)), dict(lo=0.4), dict(lo=1.1),
                dict(hi=0.9), dict(hi=2.1), dict(m=0), dict(m=-2)):
        assert centre(**bad) == E, bad


def test_ops_and_class_refuse_cpu_tensors_before_loading_anything(monkeypatch):
    from speech_anonymization_amd import _lib, formantnorm, ops
    from speech_anonymization_amd._lib import SaHipError

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    i32 = dict(dtype=torch.int32)
    with pytest.raises(SaHipError, match="GPU"):
        ops.pole_warp(torch.zeros(1, 500), torch.ones(1), torch.full((1,), 500, **i32))
    with pytest.raises(SaHipError, match="GPU"):
        ops.formant_centre(torch.zeros(1, 4, 3), torch.zeros(1, 4, **i32), None, torch.full((1,), 4, **i32),
                           (550.0, 1650.0, 2750.0))
    with pytest.raises(SaHipError, match="GPU"):
        formantnorm.FormantNormalizer()(torch.zeros(1, 500), torch.ones(1))
    with pytest.raises(SaHipError, match="GPU"):
        formantnorm.FormantNormalizer(ratio=0.9)(torch.zeros(1, 500), torch.ones(1))


# ---- the recipe ---------------------------------------------------------------------------------------------
def test_recipe_config_loads_and_refuses():
    from speech_anonymization_amd import formantnorm, gender, pitchnorm
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    path = os.path.join(ROOT, "speechbrain_configs", "gender_classifier_formant_norm.yaml")
    with open(path) as fin:
        settings = load_hyperpyyaml(fin, {})
    assert settings["formant_norm"]["target_hz"] == [550.0, 1650.0, 2750.0]
    assert settings["output_folder"].endswith("gender_classifier_formant_norm")
    default = {"level": True, "target_hz": (550.0, 1650.0, 2750.0), "q_min": 0.8, "q_max": 1.2, "min_frames": 8,
               "f0_method": "yin"}
    check = formantnorm.check_recipe_options
    assert check(settings, {}, {}) == (default, None)
    assert check(dict(settings, pitch_norm=True, pitch_target_hz=150.0, f0_method="viterbi"), {}, {}) == \
        (dict(default, f0_method="viterbi"), {"target_hz": 150.0, "psola": True, "f0_method": "viterbi"})
    block = dict(settings["formant_norm"], pitch_norm=True)
    assert check(dict(settings, formant_norm=block), {}, {})[1] == {"target_hz": 170.0, "psola": True, "f0_method": "yin"}
    with open(path) as fin:
        ratio = load_hyperpyyaml(fin, {"formant_norm_ratio": 0.9})
    assert check(ratio, {}, {})[0]["ratio"] == 0.9
    with open(path) as fin:
        target = load_hyperpyyaml(fin, {"formant_target": "600,1350,2500", "formant_q_max": 1.1})
    assert check(target, {}, {})[0] == dict(default, target_hz=(600.0, 1350.0, 2500.0), q_max=1.1)
    with pytest.raises(SystemExit, match="gender_classifier_train_formant_norm does not support --hip_graph"):
        check(dict(settings, hip_graph=True), {}, {})
    with pytest.raises(SystemExit, match="gender_classifier_train_formant_norm runs on one GPU"):
        check(settings, {"distributed_launch": True}, {})
    with pytest.raises(SystemExit, match="gender_classifier_train_formant_norm runs on one GPU"):
        check(settings, {}, {"WORLD_SIZE": "4"})
    with pytest.raises(SystemExit, match="--formant_norm_ratio 0.2"):
        check(dict(settings, formant_norm_ratio=0.2), {}, {})
    with pytest.raises(SystemExit, match="--pitch_target_hz 900"):
        check(dict(settings, pitch_norm=True, pitch_target_hz=900.0), {}, {})
    with pytest.raises(SystemExit, match="--pitch_norm 3: true or false"):
        check(dict(settings, pitch_norm=3), {}, {})
    assert os.path.exists(os.path.join(ROOT, "gender_classifier_train_formant_norm.py"))
    # the recipe's row: GenderBrain with the formant normaliser first and, with --pitch_norm true, the PSOLA pitch
    # normaliser behind it; what the hook does with the list at every stage is tests/test_gender_recipes_cpu.py's
    row = gender.RECIPES["gender_classifier_train_formant_norm"]
    assert row.brain is gender.GenderBrain
    assert [type(t) for t in row.transforms(row.check(settings, {}, {}))] == [formantnorm.FormantNormalizer]
    both = row.transforms(row.check(dict(settings, pitch_norm=True), {}, {}))
    assert [type(t) for t in both] == [formantnorm.FormantNormalizer, pitchnorm.PitchNormalizer] and both[1].psola


def test_formant_then_pitch_transform_run_at_every_stage_before_the_features(monkeypatch):
    """the hook on a list of two, as the recipe with --pitch_norm true passes it: the first sees the raw waveform object
    at TRAIN, VALID and TEST, the second what the first returned, and the front end what the second returned"""
    import types
    from speech_anonymization_amd import gender
    from speech_anonymization_amd.brain import Batch, Stage

    class Modules(dict):
        __getattr__ = dict.__getitem__

    seen = []

    def stub(name, add):
        def call(wavs, lens):
            seen.append((name, wavs))
            return wavs + add
        return call

    def fbank(wavs):
        seen.append(("fbank", wavs))
        return wavs[:, :, None]

    monkeypatch.setattr(gender.xvector, "train_log_probs", lambda emb, cl, feats, lens: feats)
    b = object.__new__(gender.GenderBrain)
    b.device = torch.device("cpu")
    b.modules = Modules(compute_features=fbank, mean_var_norm=lambda feats, lens: feats, embedding_model=None,
                        classifier=None)
    b.hparams = types.SimpleNamespace(waveform_transforms=[stub("formant", 1.0), stub("pitch", 2.0)])
    wav, lens = torch.zeros(2, 8), torch.ones(2)
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        del seen[:]
        out = b.compute_forward(Batch(wav, lens, torch.zeros(2, dtype=torch.long)), stage)
        assert [k for k, _ in seen] == ["formant", "pitch", "fbank"] and seen[0][1] is wav
        assert torch.equal(seen[1][1], wav + 1.0) and torch.equal(seen[2][1], wav + 3.0) and out.shape == (2, 8, 1)
