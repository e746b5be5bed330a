"""Host side of the Griffin-Lim inversion (speech_anonymization_amd.vocoder): the Mel
pseudo-inverse, the window envelope, the sample count, anonymize.py's refusals and the ops' refusal of CPU tensors.
No GPU."""
import numpy as np
import pytest
import torch

from speech_anonymization_amd import vocoder
from speech_anonymization_amd._lib import SaHipError
from speech_anonymization_amd.features import _hamming, _mel_matrix


def _fb():
    return _mel_matrix(80, 400, 16000)[:201, :80].double().numpy()


def test_mel_pinv_is_the_truncated_pseudo_inverse():
    """[80, 201]; bins 0 and 200, which no filter covers, exactly zero; entries of order one (the uncut inverse has
    4.5e6); M fb is a projector (Moore-Penrose: (fb+ fb)^2 = fb+ fb, symmetric) to 1e-9.

    Kept rank: the specification of this matrix (numpy.linalg.pinv(fb, rcond=1e-3)) quoted 76 for it, which is the
    number of NON-ZERO singular values of fb, not the number above the cutoff.  The filterbank's singular values are
    2.406 ... 0.523 (75 of them), then 9.5e-8 -- the one that gives the uncut inverse its condition number 2.5e7 and
    its 4.5e6 entries, and which the cutoff exists to remove -- then four zeros (four low filters reach no bin
    centre).  So rcond = 1e-3 (and 1e-2 alike, which gives the same matrix) keeps 75, and 76 kept would be the uncut matrix.
    The test pins what the specified formula gives: 75, with the gap on either side of the cutoff."""
    M, fb = vocoder.mel_pinv(), _fb()
    assert M.shape == (80, 201) and M.dtype == np.float64
    assert not M[:, 0].any() and not M[:, 200].any()
    print(f"max |M| = {np.abs(M).max():.3f}, rank {np.linalg.matrix_rank(M)}")
    assert np.abs(M).max() <= 2.0
    sv = np.linalg.svd(fb, compute_uv=False)
    print("singular values of fb around the cutoff:", sv[73:77] / sv[0])
    assert sv[74] / sv[0] > 0.1 and sv[75] / sv[0] < 1e-6          # nothing near 1e-3: the cutoff is not delicate
    assert int((sv > 1e-3 * sv[0]).sum()) == 75 and int((sv > 1e-12 * sv[0]).sum()) == 76
    assert np.linalg.matrix_rank(M) == 75
    P = M @ fb
    assert np.abs(P @ P - P).max() <= 1e-9
    assert np.abs(P - P.T).max() <= 1e-9
    assert vocoder.mel_pinv() is M and not M.flags.writeable


def test_envelope_is_the_brute_force_sum_and_stays_positive():
    w2 = _hamming(400).astype(np.float64) ** 2
    for T in (2, 3, 4, 73):
        N = vocoder.n_samples(T)
        E = vocoder.envelope(T)
        assert E.shape == (N + 400,)
        want = np.array([sum(w2[p - 160 * t] for t in range(T) if 0 <= p - 160 * t < 400) for p in range(N + 400)])
        assert np.abs(E - want).max() <= 1e-12, T
        inner = E[200:200 + N]
        print(f"T={T}: envelope on the output span {inner.min():.4f} .. {inner.max():.4f}")
        assert inner.min() > 0.9


def test_n_samples():
    assert vocoder.n_samples(2) == 160 and vocoder.n_samples(73) == 11520 and vocoder.n_samples(1008) == 161120
    for T in (2, 3, 101):
        assert 1 + vocoder.n_samples(T) // 160 == T            # the front end's frame count of that many samples
    for bad in (1, 0, -3):
        with pytest.raises(ValueError):
            vocoder.n_samples(bad)


def test_host_tables_are_rounded_once_from_fp64():
    w, tw = vocoder.host_tables()
    i = np.arange(400, dtype=np.float64)
    assert w.dtype == torch.float32 and np.array_equal(w.numpy(), _hamming(400))
    assert np.array_equal(tw.numpy()[:400], np.cos(2 * np.pi * i / 400).astype(np.float32))
    assert np.array_equal(tw.numpy()[400:], np.sin(2 * np.pi * i / 400).astype(np.float32))


GOOD = {"model_type": "fcae", "recon_ckpt": "/some/CKPT+x", "out_dir": "/tmp/out", "synthetic": 4}


@pytest.mark.parametrize("change,run_opts,environ,word", [
    ({"model_type": "vae"}, {}, {}, "unknown model_type"),
    ({"model_type": None}, {}, {}, "unknown model_type"),
    ({"recon_ckpt": None}, {}, {}, "--recon_ckpt"),
    ({}, {"distributed_launch": True}, {}, "data parallelism"),
    ({}, {}, {"WORLD_SIZE": "2"}, "data parallelism"),
    ({"hip_graph": True}, {}, {}, "hip_graph"),
    ({}, {"hip_graph": True}, {}, "hip_graph"),
    ({"out_dir": None}, {}, {}, "--out_dir"),
    ({"synthetic": None}, {}, {}, "--csv"),
    ({"csv": "a.csv"}, {}, {}, "exclude"),
])
def test_check_anonymize_options_refuses_in_one_line(change, run_opts, environ, word):
    with pytest.raises(SystemExit) as e:
        vocoder.check_anonymize_options(dict(GOOD, **change), run_opts, environ)
    msg = str(e.value)
    assert word in msg and "\n" not in msg


def test_check_anonymize_options_accepts():
    vocoder.check_anonymize_options(dict(GOOD), {}, {})
    vocoder.check_anonymize_options(dict(GOOD, recon_ckpt=None, passthrough=True), {"device": "cuda:0"}, {})
    vocoder.check_anonymize_options(dict(GOOD, synthetic=None, csv="a.csv", model_type="convae"), {}, {"WORLD_SIZE": "1"})


def test_ops_refuse_cpu_tensors_before_loading_anything(monkeypatch):
    from speech_anonymization_amd import _lib, ops

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    w, tw = vocoder.host_tables()
    M = torch.from_numpy(vocoder.mel_pinv().astype(np.float32))
    with pytest.raises(SaHipError, match="GPU"):
        ops.mel_to_mag(torch.zeros(1, 4, 80), torch.zeros(80), torch.ones(80), M)
    with pytest.raises(SaHipError, match="GPU"):
        ops.gl_istft(torch.zeros(1, 4, 201, dtype=torch.complex64), w, tw)
    with pytest.raises(SaHipError, match="GPU"):
        ops.gl_project(torch.zeros(1, 480), torch.zeros(1, 4, 201), torch.zeros(1, 4, 201, dtype=torch.complex64),
                       0.5, w, tw)
    with pytest.raises(SaHipError, match="GPU"):
        vocoder.GriffinLim()(torch.zeros(1, 4, 201))
    with pytest.raises(SaHipError, match="GPU"):
        vocoder.invert_features(torch.zeros(1, 4, 80), None)


def test_griffin_lim_draws_its_phases_from_its_own_seeded_generator():
    a, b, c = vocoder.GriffinLim(seed=5), vocoder.GriffinLim(seed=5), vocoder.GriffinLim(seed=6)
    torch.manual_seed(0)
    pa = a.draw_phase((2, 3, 201))
    torch.manual_seed(1)
    pb = b.draw_phase((2, 3, 201))
    assert pa.dtype == torch.float32 and torch.equal(pa, pb) and not torch.equal(pa, c.draw_phase((2, 3, 201)))
    assert float(pa.min()) >= 0.0 and float(pa.max()) < 2 * np.pi + 1e-6
    assert not torch.equal(pa, a.draw_phase((2, 3, 201)))            # the generator moves on
    assert abs(a.m - 0.99 / 1.99) < 1e-15
    with pytest.raises(ValueError):
        vocoder.GriffinLim(momentum=1.0)
