"""The modulation-spectrum smoothing on the GPU (include/sa_hip.h carries the definition) against the
fp64 numpy restatement tests/modspec_ref.py.

The kernel's arithmetic is fp64 and its result is rounded once, so the bars are rounding bars, not measurements:

    |C - ref| <= 2^-23 |ref| + 2^-126                                              per component
    |Lout - ref| <= (2 J + 8) 2^-52 (|L[t]| + sum_j |h_j| (|L[c(t - j)]| + |L[c(t + j)]|))
    peak equal in bits
    the share of C components whose bits differ from the restatement's at most 1e-3

The last keeps the ulp bar from hiding structure: tools/modspec_delta.py records that the restatement under its own
perturbations (the sum from the far end, L nudged by an ulp) changes none of these cases' components.

The class is held to its restatement within 8 x the spread that carrying the inversion in fp32 causes (figure (b) of
profiles/modspec_delta.json, read, not typed in).  End to end, on two amplitude-modulated harmonic rows, the
modulation depth at f_m after / before is held to the ideal low-pass (1 at 4 Hz, 0 at 20 Hz) within twice the
distance the restatement itself keeps from it (figure (c); DESIGN section 25's rule, per row)."""
import ctypes
import errno
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from speech_anonymization_amd import modspec  # noqa: F401  (without the feature nothing here can run)
from tests import anon_cli
from tests import modspec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
gpu = pytest.mark.gpu
NAN = float("nan")


def _f(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV).contiguous()


def _dims():
    from speech_anonymization_amd import _lib
    return [_lib.load().sa_modspec_dim(i) for i in range(9)]


def _raw(Rin, h, depth, frames, floor_rel=1e-4, max_gain_db=40.0, log=True, J=None, B=None, T=None, rc_want=0,
         null=()):
    """sa_modspec_smooth through the library itself, into NaN-poisoned outputs -> (C, peak, Lout) on the device"""
    from speech_anonymization_amd import _lib, ops
    lib = _lib.load()
    Rd = Rin if torch.is_tensor(Rin) else _dev(Rin, torch.complex64)
    hd, dd, fd = _dev(h, torch.float64), _dev(depth, torch.float32), _dev(frames, torch.int32)
    Bt, Tt, _ = Rd.shape
    C = torch.full_like(Rd, complex(NAN, NAN))
    peak = torch.full((Bt,), NAN, dtype=torch.float64, device=DEV)
    Lout = torch.full((Bt, Tt, 201), NAN, dtype=torch.float64, device=DEV) if log else None
    ws = ops.modspec_workspace(Bt, Tt, DEV)
    args = {"R": Rd, "taps": hd, "depth": dd, "frames": fd, "C": C, "peak": peak, "Lout": Lout, "ws": ws}
    for name in null:
        args[name] = None
    if "alias" in null:
        args["C"] = Rd
    rc = lib.sa_modspec_smooth(_f(args["R"]), _f(args["taps"]), len(h) - 1 if J is None else J, _f(args["depth"]),
                               _f(args["frames"]), Bt if B is None else B, Tt if T is None else T,
                               ctypes.c_float(floor_rel), ctypes.c_float(max_gain_db * R.LN10_OVER_20),
                               _f(args["C"]), _f(args["peak"]), _f(args["Lout"]), _f(args["ws"]), _lib.stream())
    torch.cuda.synchronize()
    assert rc == rc_want, rc
    return C, peak, Lout


def _bits(t):
    return t.contiguous().view(torch.float32).view(torch.int32) if t.dtype == torch.complex64 else \
        t.contiguous().view(torch.int64)


@gpu
def test_dims_and_workspace():
    """the constants the cases are placed by"""
    d = _dims()
    assert d[:4] == [400, 160, 201, 64] and d[4] % d[6] == 0 and d[4] >= 64 and 1 <= d[5] <= 201
    from speech_anonymization_amd import _lib
    lib = _lib.load()
    assert lib.sa_modspec_dim(9) == lib.sa_modspec_dim(-1) == -errno.EINVAL
    assert lib.sa_modspec_workspace_bytes(3, 211) == 8 * 3 * 4
    assert lib.sa_modspec_workspace_bytes(1, 1 << 23) == 8 * d[7]
    for B, T in ((0, 5), (65536, 5), (1, 0), (1, (1 << 23) + 1)):
        assert lib.sa_modspec_workspace_bytes(B, T) == -errno.EINVAL


@pytest.fixture(scope="module")
def tile():
    return _dims()[4]


# the cases are listed at the tile size the header documents; test_cases_sit_on_the_kernels_tiles holds it to the
# library's
CASES = R.cases(128)


@gpu
def test_cases_sit_on_the_kernels_tiles(tile):
    assert [c[:5] for c in R.cases(tile)] == [c[:5] for c in CASES]
    assert any(c[2] == 2 * tile + 1 for c in CASES)


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_against_the_restatement(case):
    from speech_anonymization_amd import ops
    name, B, T, frames, J, depth, floor_rel, gain_db = case
    Rin, h = R.case_input(B, T), R.case_taps(J)
    assert len(h) == J + 1
    Cr, pr, Lr, bound = R.smooth(Rin, h, depth, frames, floor_rel, gain_db)
    C, peak, Lout = _raw(Rin, h, depth, frames, floor_rel, gain_db)
    C, peak, Lout = C.cpu().numpy(), peak.cpu().numpy(), Lout.cpu().numpy()
    # every poisoned output was overwritten
    assert np.isfinite(C.view(np.float32)).all() and np.isfinite(peak).all() and np.isfinite(Lout).all()
    assert (peak.view(np.int64) == pr.view(np.int64)).all()
    for got, ref in ((C.real, Cr.real), (C.imag, Cr.imag)):
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        bar = 2.0 ** -23 * np.abs(ref.astype(np.float64)) + 2.0 ** -126
        print(f"{name}: worst |C - ref| / bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all()
    lbar = (2 * J + 8) * 2.0 ** -52 * bound
    lerr = np.abs(Lout - Lr)
    live = lbar > 0
    print(f"{name}: worst |Lout - ref| / bar {float((lerr[live] / lbar[live]).max()) if live.any() else 0:.3f}")
    assert (lerr <= lbar).all()
    share = R.bits_differ(C, Cr)
    print(f"{name}: share of C components whose bits differ {share:.2e}")
    assert share <= 1e-3
    # what is copied is R's bits: frames from T_b on, rows of depth 0 (after the clamp), rows without frames
    for b in range(B):
        tb = min(max(frames[b], 0), T)
        assert (C[b, tb:].view(np.uint32) == Rin[b, tb:].view(np.uint32)).all() and (Lout[b, tb:] == 0).all()
        if R.clamp_depth(depth[b]) == 0.0 or tb == 0:
            assert (C[b].view(np.uint32) == Rin[b].view(np.uint32)).all()
    if J == 0:                                               # h = (1): C = R by arithmetic
        assert (C.view(np.uint32) == Rin.view(np.uint32)).all()
    # the gain clamp is reached where it was made small, and the floor where a frame lies under it
    if gain_db < 40.0:
        g = np.abs((Lout - R.log_mag(Rin, frames, floor_rel)[0])[0])
        gmax = float(np.float32(gain_db * R.LN10_OVER_20))
        assert g.max() <= gmax * (1 + 1e-12) and (g >= gmax * (1 - 1e-12)).mean() > 0.1
    # the binding gives the raw call's bits, with and without Lout
    Rd = _dev(Rin, torch.complex64)
    a = ops.modspec_smooth(Rd, _dev(h, torch.float64), _dev(depth, torch.float32), _dev(frames, torch.int32), floor_rel,
                           gain_db, return_log=True)
    b2 = ops.modspec_smooth(Rd, _dev(h, torch.float64), _dev(depth, torch.float32), _dev(frames, torch.int32),
                            floor_rel, gain_db)
    assert len(b2) == 2
    for got, want in zip(a, (C, peak, Lout)):
        assert torch.equal(_bits(got).cpu(), _bits(torch.from_numpy(want)))
    for got, want in zip(b2, (C, peak)):
        assert torch.equal(_bits(got).cpu(), _bits(torch.from_numpy(want)))


@gpu
def test_identity_taps_of_50_hz_give_r(tile):
    from speech_anonymization_amd import ops
    Rin = _dev(R.case_input(3, 211), torch.complex64)
    taps, J = ops.modspec_taps(50.0, DEV)
    assert J == 4 and taps.cpu().tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    C, _ = ops.modspec_smooth(Rin, taps, torch.ones(3, device=DEV),
                              torch.full((3,), 211, dtype=torch.int32, device=DEV))
    assert torch.equal(_bits(C), _bits(Rin))


@gpu
def test_two_runs_and_a_row_alone_give_the_same_bits():
    B, T, frames = R.case_shapes(128)[0]
    Rin = R.case_input(B, T)
    for J in (20, 64):
        h = R.case_taps(J)
        one = _raw(Rin, h, R.CASE_DEPTH, frames)
        two = _raw(Rin, h, R.CASE_DEPTH, frames)
        for x, y in zip(one, two):
            assert torch.equal(_bits(x), _bits(y))
        for b in range(B):
            alone = _raw(Rin[b:b + 1], h, R.CASE_DEPTH[b:b + 1], frames[b:b + 1])
            for x, y in zip(one, alone):
                assert torch.equal(_bits(x[b:b + 1]), _bits(y))


@gpu
def test_frames_and_depth_are_clamped():
    B, T = 3, 67
    Rin, h = R.case_input(B, T), R.case_taps(20)
    a = _raw(Rin, h, (2.0, -1.0, NAN), (T + 9, -4, 40))
    b = _raw(Rin, h, (1.0, 0.0, 0.0), (T, 0, 40))
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


@gpu
def test_entry_point_and_binding_refuse():
    """only arguments the library rejects before launching: -EINVAL, and the poisoned outputs untouched"""
    from speech_anonymization_amd import _lib, ops
    E = -errno.EINVAL
    B, T = 2, 67
    Rin, h = R.case_input(B, T), R.case_taps(20)
    depth, frames = (1.0, 0.5), (67, 30)
    bad = [dict(null=("R",)), dict(null=("taps",)), dict(null=("depth",)), dict(null=("frames",)), dict(null=("C",)),
           dict(null=("peak",)), dict(null=("ws",)), dict(null=("alias",)), dict(B=0), dict(B=65536), dict(T=0),
           dict(T=(1 << 23) + 1), dict(J=-1), dict(J=65), dict(floor_rel=0.0), dict(floor_rel=1.0),
           dict(floor_rel=NAN), dict(max_gain_db=0.0), dict(max_gain_db=-3.0), dict(max_gain_db=NAN)]
    for kw in bad:
        C, peak, Lout = _raw(Rin, h, depth, frames, rc_want=E, **kw)
        assert bool(torch.isnan(torch.view_as_real(C)).all()) and bool(torch.isnan(peak).all()), kw
        assert bool(torch.isnan(Lout).all()), kw
    # the binding: one line each, before the library is asked
    Rd, hd = _dev(Rin, torch.complex64), _dev(h, torch.float64)
    dd, fd = _dev(depth, torch.float32), _dev(frames, torch.int32)
    refused = [(Rd.cpu(), hd, dd, fd), (Rd[:, :, :200], hd, dd, fd), (torch.view_as_real(Rd)[..., 0], hd, dd, fd),
               (Rd, hd.float(), dd, fd), (Rd, hd[None], dd, fd),
               (Rd, torch.zeros(66, dtype=torch.float64, device=DEV), dd, fd),
               (Rd, hd[::2], dd, fd), (Rd, hd, dd.double(), fd), (Rd, hd, dd[:1], fd), (Rd, hd, dd, fd.long()),
               (Rd, hd, dd, fd[:1])]
    for args in refused:
        with pytest.raises(_lib.SaHipError) as e:
            ops.modspec_smooth(*args)
        assert "\n" not in str(e.value)
    for kw in (dict(floor_rel=0.0), dict(floor_rel=1.0), dict(max_gain_db=0.0)):
        with pytest.raises(_lib.SaHipError):
            ops.modspec_smooth(Rd, hd, dd, fd, **kw)
    for c in (3.19, 50.1, NAN, True):
        with pytest.raises(_lib.SaHipError):
            ops.modspec_taps(c, DEV)


# ---------------------------------------------------------------------------------------------------
# the class, end to end
# ---------------------------------------------------------------------------------------------------
@gpu
def test_class_against_its_restatement_without_a_host_copy():
    rec = R.load_delta()["class"]
    wav = R.e2e_rows()
    B, N = wav.shape
    wd, lens = torch.as_tensor(wav).to(DEV), torch.tensor(R.CLASS_LENS, device=DEV)
    ms = modspec.ModulationSmoother(R.E2E_CUTOFF)
    first = ms(wd, lens)                                     # (warm-up: the library loads, the tables are built)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                  # a device-to-host copy raises from here on
    try:
        second = ms(wd, lens)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(first, second) and second.shape == wd.shape and second.dtype == torch.float32
    peak, frames = ms.last
    assert peak.is_cuda and frames.is_cuda and frames.dtype == torch.int32
    nv = R.n_valid(R.CLASS_LENS, N)
    assert frames.cpu().tolist() == (nv // 160 + 1).tolist()
    out = second.cpu().double().numpy()
    for b in range(B):
        assert (out[b, nv[b]:] == 0).all()
    ref = R.smoother(wav, R.CLASS_LENS, R.E2E_CUTOFF)
    dist = np.linalg.norm(out - ref, axis=1) / np.linalg.norm(ref, axis=1)
    spread = max(rec["istft32_rel"])
    print(f"relative Frobenius distance per row {dist.tolist()}, fp32-ISTFT spread {spread:.3e}, bar {8 * spread:.3e}")
    assert (dist <= 8.0 * spread).all()


@gpu
def test_modulation_above_the_cutoff_is_removed_and_below_it_kept():
    rec = R.load_delta()["e2e"]
    wav = R.e2e_rows()
    B, N = wav.shape
    ms = modspec.ModulationSmoother(R.E2E_CUTOFF)
    out = ms(torch.as_tensor(wav).to(DEV), torch.ones(B, device=DEV)).cpu().double().numpy()
    ratios = R.e2e_ratios(out, wav)
    for b, fm in enumerate(R.E2E_FM):
        dev_ref = rec["deviation"][b]
        print(f"f_m {fm:g} Hz: mod_depth out / in {ratios[b]:.6f} (restatement {rec['ratio'][b]:.6f}), wanted "
              f"{R.E2E_WANTED[b]:g}, bar {2 * dev_ref:.3e}")
        assert abs(ratios[b] - R.E2E_WANTED[b]) <= 2.0 * dev_ref
    assert ratios[0] > 0.9 and ratios[1] < 0.5               # and the figures mean what the feature is for


# ---------------------------------------------------------------------------------------------------
# the command line and the recipe
# ---------------------------------------------------------------------------------------------------
@gpu
def test_anonymize_modspec_mode_in_a_child(tmp_path):
    out = tmp_path / "modspec"
    res = anon_cli.run_child(["--device", DEV, "--synthetic", "4", "--out_dir", str(out), "--modspec_cutoff_hz", "10",
                              "--report_f0", "true"])
    assert res["modspec"] is True and res["cutoff_hz"] == 10.0 and res["depth"] == 1.0 and res["taps"] == 20
    assert res["n_iter"] is None
    assert not {"pitch_norm", "model_type", "recon_ckpt", "mcadams", "resynth", "seed"} & set(res)
    assert sorted(os.listdir(out)) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    assert len(res["utterances"]) == 4
    for u in res["utterances"]:
        assert {"id", "samples", "peak", "frames", "f0_mean_hz", "voiced_share"} <= set(u)
        assert u["frames"] == u["samples"] // 160 + 1 and 0 < u["peak"] < 4


@gpu
def test_anonymize_modspec_with_every_report(tmp_path, capsys):
    res = anon_cli.run(capsys, ["--device", DEV, "--synthetic", "3", "--batch_size", "3", "--out_dir", str(tmp_path),
                                "--modspec_cutoff_hz", "5", "--modspec_depth", "0.5", "--report_f0", "true",
                                "--report_stoi", "true", "--report_prosody", "true", "--report_mcd", "true",
                                "--report_formants", "true"])
    assert res["modspec"] is True and res["cutoff_hz"] == 5.0 and res["depth"] == 0.5 and res["taps"] == 40
    for u in res["utterances"]:
        assert {"frames", "stoi", "f0_corr", "mcd_db", "formant_shift", "f0_mean_hz"} <= set(u)


@gpu
def test_recipe_trains_one_epoch(tmp_path):
    """a fresh child process, under a time limit; no error bar: one epoch on 16 synthetic utterances"""
    out = tmp_path / "modspec_recipe"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gender_classifier_train_modspec.py"),
                        os.path.join(ROOT, "speechbrain_configs", "gender_classifier_modspec.yaml"), "--device", DEV,
                        "--output_folder", str(out), "--synthetic", "16", "--number_of_epochs", "1",
                        "--modspec_cutoff_hz", "8"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["modspec"] is True and summary["cutoff_hz"] == 8.0 and summary["depth"] == 1.0
    assert 0.0 <= summary["test_error"] <= 1.0
