"""The feature front end (csrc/sa_fbank.hip: sa_fbank, sa_fbank_normalize) per element against
tests/fbank_ref.py (fp64 formulas on the same fp32 inputs), at the edges of its loops: both sides of every
32-frame tile boundary and of every N % 160 step, T < 16 and empty chunks of the 16-chunk partition, a second
turn of the 8-lane utterance loop, the round(len * T) ties, n = 1 and n = 2.

What the bars are.  The Mel product is a 2-way bf16 split by design (ph mh + pl mh + ph ml): about
3 * 2^-18 = 1.1e-5 relative on every energy however clean the spectrum is.  So the Fbank bar is not "a few
fp32 ulps" and is not taken case by case: it is 8 x the worst error, POOLED over all cases, of two plain fp32
CPU evaluations (torch.stft as the reference runs it; the direct fp32 matmul), measured from the reference side
only by tools/fbank_delta.py -> profiles/fbank_delta.json.  It is fine enough for structure -- a wrong sample
at a frame or tile edge, a lost h- or m-level split term (2^-9), a wrong maximum behind the floor -- and is not
meant to see the l-level terms.  The normalisation bars are 8 x the same tool's figures for
oracle.features.InputNormalization in fp32.  tests/test_fbank_ref_cpu.py shows that wrong variants of the
formulas exceed these bars on these cases.  The kernel's own worst errors are printed, never asserted; on an
MI355X they were 0.7e-5 (N = 1) to 2.2e-5 (N >= 10239) per case against the bar of 3.4e-4, 3.8e-5 dB on a floor,
and 2.4 u / 2.9 u / 3.7 u on mean / std / output against 26 u."""
import numpy as np
import pytest
import torch

from tests import fbank_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# profiles/fbank_delta.json (python tools/fbank_delta.py): the worst fbank_ref.mel_error of the two fp32
# evaluations over all of fbank_ref.gpu_cases() (torch.stft, case zero-4960), and the margin of ref64.distance_tau
MEL_DELTA_WORST = 4.218038184879603e-05
MEL_BAR = 8.0 * MEL_DELTA_WORST
# same file: the worst of fbank_ref.norm_errors of the fp32 oracle over fbank_ref.norm_cases(), in u = 2^-24
NORM_DELTA_WORST_U = 3.249298440532101
NORM_BAR_U = 8.0 * NORM_DELTA_WORST_U
STATE_KEYS = ("count", "glob_mean", "glob_std", "spk_dict_mean", "spk_dict_std", "spk_dict_count")
# 10 * log10f(1e-10f) in fp32: log10f gives -10 - 1 ulp there (on the device as in numpy), so -100 - 7.6e-6
SILENCE_DB = np.float32(10.0) * np.log10(np.float32(1e-10))


def dev():
    return torch.device("cuda:0")


_FB = {}


def fbank(mode):
    from speech_anonymization_amd import Fbank
    if mode not in _FB:
        _FB[mode] = Fbank(16000, 400, 80, top_db_mode=mode).to(dev())
    return _FB[mode]


# ================================================================================================
# sa_fbank
# ================================================================================================
@pytest.mark.parametrize("N", R.FBANK_N)
def test_fbank_per_element(N):
    T, nt = 1 + N // 160, (1 + N // 160 + 31) // 32
    for kind in ("rows", "zero"):
        name = f"{kind}-{N}"
        wav = R.gpu_cases()[name]
        M64 = R.case_ref(name)
        B = wav.shape[0]
        wd = wav.to(dev())
        f = fbank("utterance")(wd)
        f2 = fbank("utterance")(wd)
        fb = fbank("batch")(wd)
        torch.cuda.synchronize()
        assert f.raw.shape == (B, T, 80) and f.tilemax.shape == (B, nt) and f.raw.dtype == torch.float32
        assert torch.equal(f.raw, f2.raw) and torch.equal(f.tilemax, f2.tilemax)          # two runs, the same bits
        assert torch.equal(f.raw, fb.raw) and torch.equal(f.tilemax, fb.tilemax)          # the mode is not the kernel's
        raw = f.raw.cpu()
        assert bool(torch.isfinite(raw).all())
        # ---- every element against fp64
        e = R.mel_error(raw, M64)
        per_row = e.amax(dim=(1, 2))
        labels = R.SIGNALS if kind == "rows" else ("first", "zero", "third")
        print(f"fbank {name}: worst e {float(e.max()):.3e} (bar {MEL_BAR:.3e}); "
              + ", ".join(f"{l} {float(v):.2e}" for l, v in zip(labels, per_row)))
        assert float(e.max()) <= MEL_BAR
        # ---- exact: tile maxima, digital silence, the clamp
        for i in range(nt):
            assert torch.equal(f.tilemax[:, i], f.raw[:, 32 * i:32 * i + 32].amax(dim=(1, 2))), i
        silent = (R.frames(wav).abs().amax(dim=2) == 0.0)                                  # [B, T]: all-zero frames
        if kind == "zero":
            assert bool(silent[1].all())
        sil = float(SILENCE_DB)
        assert abs(sil + 100.0) <= 2.0 ** -17                                              # one ulp of fp32 at 100
        if bool(silent.any()):
            assert bool((raw[silent] == sil).all())
        # ---- the floor: derived from the bar (the largest element is the largest of its own frame)
        raw64 = R.raw_db(M64)
        for feats, mode in ((f, "utterance"), (fb, "batch")):
            tm = feats.tilemax
            fl = (tm.amax(dim=1) if mode == "utterance" else tm.max().expand(B)) - feats.top_db
            want = torch.maximum(feats.raw, fl.view(-1, 1, 1))
            assert torch.equal(feats.clamped(), want)
            assert torch.equal(want, torch.maximum(feats.raw, (feats.raw.amax(dim=(1, 2)) if mode == "utterance"
                                                               else feats.raw.max().expand(B)).view(-1, 1, 1) - 80.0))
            d = (fl.cpu().double() - R.floors(raw64, mode)).abs()
            print(f"  floor {mode}: worst |d| {float(d.max()):.3e} dB (bound {R.floor_bound(MEL_BAR):.3e})")
            assert float(d.max()) <= R.floor_bound(MEL_BAR)
            if kind == "zero":
                c = feats.clamped()[1].cpu()
                if mode == "utterance":
                    assert bool((c == sil).all())
                else:                                          # the all-zero row sits at the batch's floor, not at -100
                    assert N < 159 or float(fl[1]) > sil
                    assert bool((c == max(float(fl[1]), sil)).all())


@pytest.mark.parametrize("N,T", [(5120, 33), (1, 1)])
def test_fbank_abi_writes_all_of_its_buffers_and_nothing_else(N, T):
    """sa_fbank on poisoned buffers with guard rows behind B*T*80 and B*ntiles"""
    from speech_anonymization_amd import _lib as L
    lib = L.load()
    B, GUARD = 2, 4
    nt = lib.sa_fbank_ntiles(T)
    assert nt == (T + 31) // 32
    wav = R.gpu_cases()[f"zero-{N}"][:B].contiguous().to(dev())
    fb = fbank("utterance")
    feats = torch.full(((B + GUARD) * T * 80,), -7.0, device=dev())
    tmax = torch.full(((B + GUARD) * nt,), -7.0, device=dev())
    L.check(lib.sa_fbank(L.ptr(wav), B, N, L.ptr(fb.window), L.ptr(fb.dft), L.ptr(fb.mel), L.ptr(feats), L.ptr(tmax),
                         L.stream()), "sa_fbank")
    want = fb(wav)
    torch.cuda.synchronize()
    assert bool((feats[B * T * 80:] == -7.0).all()) and bool((tmax[B * nt:] == -7.0).all())
    assert bool((feats[:B * T * 80] != -7.0).all()) and bool((tmax[:B * nt] != -7.0).all())
    assert torch.equal(feats[:B * T * 80].view(B, T, 80), want.raw) and torch.equal(tmax[:B * nt].view(B, nt), want.tilemax)
    assert lib.sa_fbank(L.ptr(wav), 0, N, L.ptr(fb.window), L.ptr(fb.dft), L.ptr(fb.mel), L.ptr(feats), L.ptr(tmax),
                        L.stream()) == -22


# ================================================================================================
# sa_fbank_normalize
# ================================================================================================
def _run_sequence(nrm, feats, lens, calls, refs, xs, label):
    """feats[i % len(feats)] through nrm for every call, each result against refs[i]; -> worst (mean, std, out)"""
    worst = [0.0, 0.0, 0.0]
    for i, ((training, epoch), ref) in enumerate(zip(calls, refs)):
        nrm.train(training)
        before = nrm.state.clone()
        out = nrm(feats[i % len(feats)], lens, epoch=epoch, pad_multiple=36)
        torch.cuda.synchronize()
        x = xs[i % len(xs)]
        T = x.shape[1]
        assert out.shape == ref[0].shape and out.dtype == torch.float32
        assert out.shape[1] == (T if T % 36 == 0 else T + 36 - T % 36)                    # no padding at T % 36 == 0
        if out.shape[1] > T:
            assert float(out[:, T:].abs().max()) == 0.0                                   # pad rows: exact zeros
        assert nrm.count == ref[1]
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(nrm.state).all())
        if not training or (epoch >= R.UNTIL and int(before[0]) > 0):
            assert torch.equal(nrm.state[1:], before[1:])                                 # frozen / eval: the same bits
        if not training:
            assert torch.equal(nrm.state, before)
        e = R.norm_errors(out.cpu(), nrm.glob_mean.cpu(), nrm.glob_std.cpu(), x, ref)
        print(f"norm {label} call {i} (train {training}, epoch {epoch}): mean {e[0] / U:.2f} u, std {e[1] / U:.2f} u, "
              f"out {e[2] / U:.2f} u (bar {NORM_BAR_U:.1f} u)")
        worst = [max(a, b) for a, b in zip(worst, e)]
    return worst


def _normaliser():
    from speech_anonymization_amd import InputNormalization
    return InputNormalization("global", update_until_epoch=R.UNTIL).to(dev())


def _load(nrm):
    count, gm, gs = R.loaded_state()
    nrm.load_state_dict(dict(count=count, glob_mean=gm, glob_std=gs))
    assert nrm.count == count and torch.equal(nrm.glob_mean.cpu(), gm) and torch.equal(nrm.glob_std.cpu(), gs)


@pytest.mark.parametrize("name", list(R.norm_cases()))
def test_normalisation_per_element(name):
    xs, lens = R.norm_cases()[name]
    fresh, loaded = R.norm_case_ref(name)
    xd = [x.to(dev()) for x in xs]
    nrm = _normaliser()
    assert tuple(nrm.state_dict().keys()) == STATE_KEYS and nrm.count == 0
    worst = _run_sequence(nrm, xd, lens, R.CALLS, fresh, xs, name)
    sd = nrm.state_dict()
    assert tuple(sd.keys()) == STATE_KEYS and sd["count"] == 3
    assert sd["spk_dict_mean"] == {} and sd["spk_dict_std"] == {} and sd["spk_dict_count"] == {}
    _load(nrm)
    worst2 = _run_sequence(nrm, xd, lens, R.LOAD_CALL, loaded, xs, name + " loaded")
    assert nrm.count == 6
    assert max(worst + worst2) <= NORM_BAR_U * U


@pytest.mark.parametrize("mode,case", [("utterance", "rows-11360"), ("batch", "zero-5120")])
def test_normalisation_with_the_fused_clamp(mode, case):
    """FbankFeatures in: the top-dB clamp is applied inside the statistics and the apply pass.  The reference
    starts from the kernel's own raw features (so that the Fbank's error is not inherited) and clamps them at
    fl32(max - 80), the floor as the kernel forms it: one fp32 subtraction of exact inputs."""
    wav = R.gpu_cases()[case]
    B = wav.shape[0]
    f = fbank(mode)(wav.to(dev()))
    torch.cuda.synchronize()
    raw = f.raw.cpu()
    mx = raw.amax(dim=(1, 2)) if mode == "utterance" else raw.max().expand(B)
    x = torch.maximum(raw, (mx - 80.0).view(-1, 1, 1))                  # fp32: max and one rounded subtraction
    assert torch.equal(x, f.clamped().cpu())
    assert bool((x > raw).any())                                         # the clamp does act on this case
    lens = torch.tensor(([1.0, 0.83, 0.61] + [0.5] * B)[:B])
    nrm = _normaliser()
    refs = R.norm_sequence([x], lens, R.CALLS, R.UNTIL)
    worst = _run_sequence(nrm, [f], lens, R.CALLS, refs, [x], f"fused {mode} {case}")
    _load(nrm)
    refs = R.norm_sequence([x], lens, R.LOAD_CALL, R.UNTIL, R.loaded_state())
    worst2 = _run_sequence(nrm, [f], lens, R.LOAD_CALL, refs, [x], f"fused {mode} {case} loaded")
    assert max(worst + worst2) <= NORM_BAR_U * U
