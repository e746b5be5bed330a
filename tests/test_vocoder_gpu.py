"""The Griffin-Lim inversion on the GPU (csrc/sa_vocoder.hip, speech_anonymization_amd.vocoder, anonymize.py; DESIGN
section 14) against an fp64 restatement of its definitions that lives in this file: direct sums through the same
fp32 tables and inputs converted to double.  Every figure is printed before it is asserted.

The per-kernel bars are derived, not measured; u = 2^-24 is the relative error of one fp32 rounding:
  mel_to_mag  S^2 within (80 + 64) u sum_m |p_m M[m][k]|: 80 for the dot product, 64 for the exponent's argument
              (|v ln10 / 10| <= 23 for |v| <= 100 dB, rounded twice) and the exponential.
  gl_istft    y within (400 + 8) u sum_frames w[j] (1/400) sum_k c_k |C_t,k| / E: 400 for the sum of up to 402 terms
              of magnitude <= c_k |C_t,k| / 400, 8 for the scale, the window, the 3-frame sum, the envelope, the division.
  gl_project  R within (400 + 8) u sum_j |w[j] ypad[160 t + j]|.
  update      from the kernel's own R: |C' - C'_ref| <= 16 u S per element, nothing excluded.
The transforms run at (B, T) in {(1, 2), (1, 3), (2, G), (2, G + 1), (3, 73)}, G = sa_gl_tile(): the two-frame edge
envelope, a single tile, the tile edge, a ragged last tile, several tiles.

The loop (B = 3, T = 73, 32 iterations, phases of seed 5) must reach the restatement's spectral convergence within
delta, the relative spread (max - min) / min of the restatement's own batch-mean spectral convergence over the phase
seeds 0..7 -- the scale on which two trajectories of this non-convex iteration differ.  Measured once on the CPU for
the signals below (tools/vocoder_delta.py prints them): DELTA_TRUE for true STFT magnitudes, DELTA_MEL for the
feature round trip's mean |dB| error.  See the constants for the figures.  The GPU's signal also tracks the
restatement's directly (TRACK_MEASURED), which is asserted with a stated margin."""
import os

import numpy as np
import pytest
import torch

from speech_anonymization_amd import vocoder
from tests import anon_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = 2.0 ** -24
HOP, NFFT, NBIN = 160, 400, 201
B_LOOP, T_LOOP, N_ITER, SEED = 3, 73, 32, 5
# measured on the CPU by tools/vocoder_delta.py (fp64 restatement, phase seeds 0..7, the signals of signals()):
#   spectral convergence, true magnitudes: 0.0810 0.0768 0.0936 0.0771 0.0905 0.0816 0.0826 0.0787 (0.564 at 0 iterations)
#   round trip mean |dB|: 1.333 1.381 1.400 1.335 1.390 1.318 1.369 1.317 (95th percentile 7.3 .. 7.8 dB)
DELTA_TRUE = 0.2191     # (0.09357 - 0.07675) / 0.07675
DELTA_MEL = 0.0633      # (1.4001 - 1.3167) / 1.3167
# the fp32 loop's signal against the fp64 restatement's after 32 iterations, relative Frobenius: measured 9.81e-5 on an
# MI355X (a torch fp32 loop on the CPU: 7e-5); the bar is three times that, the room for another summation order
TRACK_MEASURED, TRACK_BAR = 9.81e-5, 3e-4


# ---------------------------------------------------------------------------------------------------
# the fp64 restatement (numpy; runs without a GPU)
# ---------------------------------------------------------------------------------------------------
def tables64():
    """the kernels' own fp32 tables as double: window [400], COS / SIN [201, 400] read at (k j) mod 400"""
    w, tw = vocoder.host_tables()
    w, tw = w.double().numpy(), tw.double().numpy()
    kj = (np.arange(NBIN)[:, None] * np.arange(NFFT)[None, :]) % NFFT
    return w, tw[:NFFT][kj], tw[NFFT:][kj]


def ola(frames, w, T):
    """sum_t w[j] frames[b, t, j] at p = 160 t + j -> [B, N + 400]"""
    out = np.zeros((frames.shape[0], (T - 1) * HOP + NFFT))
    for t in range(T):
        out[:, HOP * t:HOP * t + NFFT] += w * frames[:, t]
    return out


def ref_istft(C):
    """section 2 of the definitions -> (y [B, N], bound [B, N] without its factor (400 + 8) u)"""
    w, COS, SIN = tables64()
    B, T, _ = C.shape
    N = (T - 1) * HOP
    c = np.full(NBIN, 2.0)
    c[0] = c[200] = 1.0
    cre, cim = C.real * c, -C.imag * c
    cim[..., 0] = cim[..., 200] = 0.0
    x = (cre @ COS + cim @ SIN) / NFFT
    E = vocoder.envelope(T)[200:200 + N]
    amp = np.repeat(((np.abs(C) * c).sum(-1) / NFFT)[..., None], NFFT, axis=-1)
    return ola(x, w, T)[:, 200:200 + N] / E, ola(amp, w, T)[:, 200:200 + N] / E


def ref_stft(y):
    """section 3, linear part -> (R [B, T, 201], bound [B, T, 1] without its factor)"""
    w, COS, SIN = tables64()
    B, N = y.shape
    T = 1 + N // HOP
    yp = np.pad(y, ((0, 0), (200, 200)))
    z = np.stack([w * yp[:, HOP * t:HOP * t + NFFT] for t in range(T)], axis=1)
    return z @ COS.T - 1j * (z @ SIN.T), np.abs(z).sum(-1, keepdims=True)


def ref_update(R, Tprev, S, m):
    A = R - m * Tprev
    return S * A / (np.abs(A) + 1e-16)


def ref_loop(S, phi, n_iter, m):
    C = S * np.exp(1j * phi)
    Tprev = np.zeros_like(C)
    for _ in range(n_iter):
        R = ref_stft(ref_istft(C)[0])[0]
        C, Tprev = ref_update(R, Tprev, S, m), R
    return ref_istft(C)[0]


def ref_sc(y, S):
    mag = np.abs(ref_stft(y)[0])
    return np.sqrt(((mag - S) ** 2).sum((1, 2))) / np.sqrt((S ** 2).sum((1, 2)))


def ref_mel_to_power(x, mean, std, M):
    """section 1 before the square root -> (max(0, p M), sum_m |p_m M[m][k]|)"""
    p = 10.0 ** ((x * std + mean) / 10.0)
    return np.maximum(p @ M, 0.0), p @ np.abs(M)


def ref_fbank(wav):
    """the front end in fp64: |STFT|^2 @ fb -> 10 log10(max(., 1e-10)) -> max(x, amax per utterance - 80)"""
    from speech_anonymization_amd.features import _mel_matrix
    fb = _mel_matrix(80, 400, 16000)[:201, :80].double().numpy()
    db = 10.0 * np.log10(np.maximum(np.abs(ref_stft(wav)[0]) ** 2 @ fb, 1e-10))
    return np.maximum(db, db.max(axis=(1, 2), keepdims=True) - 80.0)


def ref_round_trip(wav, phi, n_iter, m):
    """Fbank -> Mel inverse -> loop -> Fbank in fp64 -> mean |dB| difference"""
    f0 = ref_fbank(wav)
    M = vocoder.mel_pinv().astype(np.float32).astype(np.float64)
    S = np.sqrt(ref_mel_to_power(f0, 0.0, 1.0, M)[0])
    f1 = ref_fbank(ref_loop(S, phi, n_iter, m))
    return float(np.abs(f1 - f0).mean()), float(np.percentile(np.abs(f1 - f0), 95))


def signals(B=B_LOOP, T=T_LOOP):
    """19 harmonics (amplitude 0.25 / h) of 110 (1 + 0.6 b) Hz with 2 % vibrato at 5 Hz, plus 0.01 white noise"""
    N = (T - 1) * HOP
    t = np.arange(N) / 16000.0
    rs = np.random.RandomState(1234)
    out = np.zeros((B, N))
    for b in range(B):
        f0 = 110.0 * (1.0 + 0.6 * b)
        ph = 2 * np.pi * f0 * (t - 0.02 * np.cos(2 * np.pi * 5.0 * t) / (2 * np.pi * 5.0))
        out[b] = sum(0.25 / h * np.sin(h * ph) for h in range(1, 20)) + 0.01 * rs.standard_normal(N)
    return out.astype(np.float32)


def m32(momentum=0.99):
    """momentum / (1 + momentum) as the kernel receives it: rounded to fp32"""
    return float(np.float32(momentum / (1.0 + momentum)))


# ---------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _tile():
    from speech_anonymization_amd import _lib
    return _lib.load().sa_gl_tile()


def _shapes():
    G = _tile()
    return [(1, 2), (1, 3), (2, G), (2, G + 1), (3, 73)]


def _spectrum(B, T, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((B, T, NBIN)) + 1j * rs.standard_normal((B, T, NBIN))).astype(np.complex64)


@gpu
def test_mel_to_mag_against_fp64_and_padding_unread():
    """Tf = 72 with frames = 61: the padding frames hold NaN and must not be read; features across +-100 dB after
    de-normalisation; bins 0 and 200 exactly zero; a second shape with one frame and several utterances"""
    from speech_anonymization_amd import ops
    _, _, M = vocoder.tables(DEV)
    M64 = M.double().cpu().numpy()
    rs = np.random.RandomState(3)
    for B, Tf, T in [(2, 72, 61), (3, 1, 1), (1, 40, 40)]:
        mean = rs.uniform(-20, 10, 80).astype(np.float32)
        std = rs.uniform(0.5, 20, 80).astype(np.float32)
        x = rs.uniform(-6, 6, (B, Tf, 80)).astype(np.float32)
        x = np.clip(x, (-100 - mean) / std, (100 - mean) / std).astype(np.float32)     # |x std + mean| <= 100 dB
        x[:, T:] = np.nan
        S = ops.mel_to_mag(torch.from_numpy(x).to(DEV), torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV),
                           M, T).double().cpu().numpy()
        want, mag = ref_mel_to_power(x[:, :T].astype(np.float64), mean.astype(np.float64), std.astype(np.float64), M64)
        assert S.shape == (B, T, NBIN) and np.isfinite(S).all()
        err, bar = np.abs(S ** 2 - want), (80 + 64) * U * mag
        print(f"mel_to_mag B={B} Tf={Tf} T={T}: worst error / bar {np.max(err[..., 1:200] / bar[..., 1:200]):.3f}")
        assert (err <= bar).all()
        assert not S[..., 0].any() and not S[..., 200].any()


@gpu
def test_gl_istft_against_fp64():
    from speech_anonymization_amd import ops
    w, tw, _ = vocoder.tables(DEV)
    for B, T in _shapes():
        C = _spectrum(B, T, 10 * B + T)
        y = ops.gl_istft(torch.from_numpy(C).to(DEV), w, tw).double().cpu().numpy()
        want, bound = ref_istft(C.astype(np.complex128))
        assert y.shape == (B, (T - 1) * HOP)
        err, bar = np.abs(y - want), (400 + 8) * U * bound
        print(f"gl_istft B={B} T={T}: worst error / bar {np.max(err / bar):.3f}, "
              f"relative Frobenius error {np.linalg.norm(err) / np.linalg.norm(want):.2e}")
        assert (err <= bar).all()
    zero = ops.gl_istft(torch.zeros(2, 9, NBIN, dtype=torch.complex64, device=DEV), w, tw)
    assert zero.shape == (2, 8 * HOP) and not bool(zero.any())


@gpu
def test_gl_project_linear_part_and_update_against_fp64():
    """R against the direct sum; C' against the definition applied pointwise in fp64 to the kernel's own R (so the
    ill-conditioned 1 / |A| is not in the comparison), with S that holds zeros and spans six decades"""
    from speech_anonymization_amd import ops
    w, tw, _ = vocoder.tables(DEV)
    m = m32()
    for B, T in _shapes():
        rs = np.random.RandomState(100 * B + T)
        y = rs.uniform(-1, 1, (B, (T - 1) * HOP)).astype(np.float32)
        S = (10.0 ** rs.uniform(-3, 3, (B, T, NBIN))).astype(np.float32)
        S[rs.uniform(size=S.shape) < 0.05] = 0.0
        Tprev = (30.0 * _spectrum(B, T, 7 * B + T)).astype(np.complex64)
        Cn, R = ops.gl_project(torch.from_numpy(y).to(DEV), torch.from_numpy(S).to(DEV),
                               torch.from_numpy(Tprev).to(DEV), m, w, tw)
        Cn, R = Cn.cpu().numpy().astype(np.complex128), R.cpu().numpy().astype(np.complex128)
        want, bound = ref_stft(y.astype(np.float64))
        err, bar = np.abs(R - want), (400 + 8) * U * bound
        print(f"gl_project B={B} T={T}: R worst error / bar {np.max(err / bar):.3f}, "
              f"relative Frobenius error {np.linalg.norm(err) / np.linalg.norm(want):.2e}")
        assert (err <= bar).all()
        S64 = S.astype(np.float64)
        cwant = ref_update(R, Tprev.astype(np.complex128), S64, m)
        cerr = np.abs(Cn - cwant)
        print(f"gl_project B={B} T={T}: update worst error / (u S) {np.max(cerr[S64 > 0] / (U * S64[S64 > 0])):.3f} (bar 16)")
        assert (cerr <= 16 * U * S64).all()
    # Tprev = 0 and m = 0: C' = S R / |R|; a silent signal gives R = 0 and C' = 0
    Cn, R = ops.gl_project(torch.zeros(1, 4 * HOP, device=DEV), torch.ones(1, 5, NBIN, device=DEV),
                           torch.zeros(1, 5, NBIN, dtype=torch.complex64, device=DEV), 0.0, w, tw)
    assert not bool(torch.view_as_real(R).any()) and not bool(torch.view_as_real(Cn).any())


@gpu
def test_ops_refuse_what_the_kernels_cannot_take():
    from speech_anonymization_amd import _lib, ops
    from speech_anonymization_amd._lib import SaHipError
    w, tw, M = vocoder.tables(DEV)
    C = torch.zeros(2, 9, NBIN, dtype=torch.complex64, device=DEV)
    with pytest.raises(SaHipError, match="contiguous"):
        ops.gl_istft(torch.zeros(9, 2, NBIN, dtype=torch.complex64, device=DEV).transpose(0, 1), w, tw)
    with pytest.raises(SaHipError, match="complex64"):
        ops.gl_istft(C.to(torch.complex128), w, tw)
    with pytest.raises(SaHipError, match="T in 2"):
        ops.gl_istft(C[:, :1].contiguous(), w, tw)
    with pytest.raises(SaHipError, match="shape"):
        ops.gl_project(torch.zeros(2, 7 * HOP, device=DEV), torch.zeros(2, 9, NBIN, device=DEV), C, 0.5, w, tw)
    with pytest.raises(SaHipError, match="frames"):
        ops.mel_to_mag(torch.zeros(1, 4, 80, device=DEV), torch.zeros(80, device=DEV), torch.ones(80, device=DEV), M, 5)
    with pytest.raises(SaHipError, match="float32"):
        ops.mel_to_mag(torch.zeros(1, 4, 80, device=DEV).double(), torch.zeros(80, device=DEV),
                       torch.ones(80, device=DEV), M)
    lib, p = _lib.load(), _lib.ptr
    y = torch.zeros(2, 8 * HOP, device=DEV)
    assert lib.sa_gl_istft(p(C), p(w), p(tw), 2, 1, p(y), None) == -22           # T < 2
    assert lib.sa_gl_istft(p(C), p(w), p(tw), 0, 9, p(y), None) == -22           # B < 1
    assert lib.sa_gl_istft(p(C), p(w), p(tw), 65536, 9, p(y), None) == -22       # beyond grid.y
    assert lib.sa_gl_istft(None, p(w), p(tw), 2, 9, p(y), None) == -22
    assert lib.sa_gl_project(p(y), None, p(C), _lib.C.c_float(0.5), p(w), p(tw), 2, 9, p(C), p(C), None) == -22
    assert lib.sa_mel_to_mag(p(y), p(w), p(w), p(M), 1, 5, 4, p(y), None) == -22  # frames > Tf
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# the loop, the round trip
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_case():
    """the signals, their true STFT magnitudes (fp32, the input of both sides), the phases of seed 5 and the
    restatement's result: computed once, read by the tests below"""
    sig = signals()
    S = np.abs(ref_stft(sig.astype(np.float64))[0]).astype(np.float32)
    phi = vocoder.GriffinLim(seed=SEED).draw_phase(S.shape)
    y_ref = ref_loop(S.astype(np.float64), phi.double().numpy(), N_ITER, m32())
    y0_ref = ref_loop(S.astype(np.float64), phi.double().numpy(), 0, m32())
    return sig, S, phi, y_ref, y0_ref


@gpu
def test_loop_converges_like_the_restatement(loop_case):
    sig, S, phi, y_ref, y0_ref = loop_case
    S64 = S.astype(np.float64)
    sc_ref, sc0 = float(ref_sc(y_ref, S64).mean()), float(ref_sc(y0_ref, S64).mean())
    Sd = torch.from_numpy(S).to(DEV)
    y = vocoder.GriffinLim(n_iter=N_ITER, momentum=0.99, seed=SEED)(Sd)
    assert y.shape == (B_LOOP, (T_LOOP - 1) * HOP) and y.dtype == torch.float32
    sc_dev = vocoder.spectral_convergence(y, Sd).double().cpu().numpy()
    y64 = y.double().cpu().numpy()
    sc_gpu = float(ref_sc(y64, S64).mean())
    track = float(np.linalg.norm(y64 - y_ref) / np.linalg.norm(y_ref))
    print(f"spectral convergence: gpu {sc_gpu:.5f} (on the device {sc_dev.mean():.5f}), restatement {sc_ref:.5f}, "
          f"0 iterations {sc0:.4f}, delta {DELTA_TRUE}; signal against the restatement's: {track:.2e} relative")
    assert abs(float(sc_dev.mean()) - sc_gpu) <= 1e-4 * sc_gpu
    assert sc_gpu <= sc_ref * (1.0 + DELTA_TRUE)
    assert sc_gpu < sc0 / 3.0
    assert track <= TRACK_BAR, (track, TRACK_MEASURED)
    # 0 iterations is one istft of S e^{i phi}; the generator of a module makes the phases of draw_phase
    y0 = vocoder.GriffinLim(n_iter=0, seed=SEED)(Sd).double().cpu().numpy()
    assert np.linalg.norm(y0 - y0_ref) <= 1e-5 * np.linalg.norm(y0_ref)


@gpu
def test_feature_round_trip(loop_case):
    """Fbank.clamped() -> invert_features (identity normaliser) -> Fbank again: mean |dB| over all (b, t, m) against
    the fp64 restatement of the same path from the same phases"""
    from speech_anonymization_amd import features
    from speech_anonymization_amd._lib import SaHipError
    sig = loop_case[0]
    phi = vocoder.GriffinLim(seed=SEED).draw_phase((B_LOOP, T_LOOP, NBIN)).double().numpy()
    ref_mean, ref_p95 = ref_round_trip(sig.astype(np.float64), phi, N_ITER, m32())
    fbank = features.Fbank().to(DEV)
    ident = features.InputNormalization(norm_type="global")
    with pytest.raises(SaHipError, match="count"):
        vocoder.invert_features(torch.zeros(1, 4, 80, device=DEV), ident)
    ident.load_state_dict({"count": 1, "glob_mean": torch.zeros(80), "glob_std": torch.ones(80)})
    f0 = fbank(torch.from_numpy(sig).to(DEV)).clamped()
    pad = torch.full((B_LOOP, 108 - T_LOOP, 80), float("nan"), device=DEV)          # padding frames are dropped unread
    lens = torch.tensor([1.0, 0.75, 0.5])
    wav, lens_out = vocoder.invert_features(torch.cat([f0, pad], dim=1), ident, lens, frames=T_LOOP,
                                            n_iter=N_ITER, seed=SEED)
    assert wav.shape == (B_LOOP, (T_LOOP - 1) * HOP) and torch.equal(lens_out, lens)
    assert bool(torch.isfinite(wav).all())
    d = (fbank(wav).clamped() - f0).abs().double().cpu().numpy()
    got, p95 = float(d.mean()), float(np.percentile(d, 95))
    print(f"round trip mean |dB|: gpu {got:.4f} (95th percentile {p95:.2f}), restatement {ref_mean:.4f} "
          f"({ref_p95:.2f}), delta {DELTA_MEL}")
    assert got <= ref_mean * (1.0 + DELTA_MEL)


# ---------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------
def _anonymize(out, extra):
    return anon_cli.run_child(["--device", DEV, "--model_type", "fcae", "--out_dir", str(out), "--synthetic", "4",
                               "--n_iter", "8", "--seed", "3"] + extra, timeout=180)


def _check_outputs(out, res):
    from speech_anonymization_amd import data
    batches = list(data.synthetic_gender_dataset(4, 3, seed=3))                     # convae.yaml: batch_size 3
    lens = torch.cat([b.sig[1] for b in batches])
    N = vocoder.n_samples(1 + 16000 // HOP)
    assert sorted(os.listdir(out)) == [f"synthetic_{i:04d}.wav" for i in range(4)]
    assert [u["id"] for u in res["utterances"]] == [f"synthetic_{i:04d}" for i in range(4)]
    for i, u in enumerate(res["utterances"]):
        sig = data.read_audio(os.path.join(out, u["id"] + ".wav"))
        assert sig.numel() == int(float(lens[i]) * N) == u["samples"], (i, sig.numel(), u)
        assert 0.0 < u["spectral_convergence"] < 1.0 and u["peak"] > 0.0
        assert abs(float(sig.abs().max()) - min(u["peak"], 1.0)) <= 2.0 / 32767


@gpu
def test_anonymize_command_line_fcae(tmp_path):
    """a checkpoint as tests/test_reconstruct_gpu.py makes one (the ModuleList's state dict; the normaliser here with
    count 1, since one that has seen no data is refused): 4 WAVs read back, int(len N) samples each, the JSON line"""
    from speech_anonymization_amd import fcae
    z = np.load(os.path.join(ROOT, "tests", "golden", "fcae_trained.npz"))       # the reference's trained weights
    model = fcae.FullyConnectedAutoencoder(80, 3)
    model.load_state_dict({k[len("ckpt/0."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("ckpt/0.")})
    d = str(tmp_path / "anon" / "CKPT+trained")
    os.makedirs(d)
    torch.save(torch.nn.ModuleList([model]).state_dict(), os.path.join(d, "model.ckpt"))
    torch.save({"count": 1, "glob_mean": torch.full((80,), -30.0), "glob_std": torch.full((80,), 15.0),
                "spk_dict_mean": {}, "spk_dict_std": {}, "spk_dict_count": {}}, os.path.join(d, "normalizer.ckpt"))
    out = tmp_path / "wav"
    res = _anonymize(out, ["--recon_ckpt", d])
    assert res["model_type"] == "fcae" and res["recon_ckpt"] == d and not res["passthrough"] and res["n_iter"] == 8
    _check_outputs(out, res)


@gpu
def test_anonymize_command_line_passthrough_needs_no_checkpoint(tmp_path):
    out = tmp_path / "wav"
    res = _anonymize(out, ["--passthrough", "true"])
    assert res["passthrough"] and res["recon_ckpt"] is None
    _check_outputs(out, res)
