"""model_type fcae without a GPU: the parameter container, checkpoint keys, the plain-torch restatement against
the reference fixture, the library's entry points and the entry script's argument handling."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import fcae_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ZERO_GRADS = ("sex_classifier.classify.0.bias", "sex_classifier.classify.5.bias")     # a bias in front of a BatchNorm
# fp32 against fp64 of the restatement itself: up to 2.3e-8 rel-MSE per tensor at the shapes of the GPU tests;
# 30x that (the margin DESIGN section 5 gives the fp32 mode), rounded up
FP32_NOISE_BAR = 1e-6


def _ckpt():
    z = np.load(os.path.join(GOLD, "fcae_trained.npz"))
    return {k[len("ckpt/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("ckpt/")}


def test_state_dict_is_the_reference_checkpoints():
    from speech_anonymization_amd import fcae
    model = fcae.FullyConnectedAutoencoder(80, 3)
    sd, ck = model.state_dict(), _ckpt()
    assert len(list(model.parameters())) == 30 and sum(p.numel() for p in model.parameters()) == 24682
    assert ["0." + k for k in sd] == list(ck)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ck["0." + k].shape) and v.dtype == ck["0." + k].dtype, k
    assert "encoder.0.weight" in sd and "sex_classifier.classify.7.bias" in sd
    assert "sex_classifier.norm.running_var" in sd and "sex_classifier.classify.6.num_batches_tracked" in sd


def test_modulelist_prefixed_checkpoint_loads():
    """model.ckpt of the reference is the state_dict of ModuleList([model]): keys '0.encoder.0.weight' ..."""
    from speech_anonymization_amd import fcae
    model = fcae.FullyConnectedAutoencoder(80, 3)
    ck = _ckpt()
    res = torch.nn.ModuleList([model]).load_state_dict(ck, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in model.state_dict().items():
        assert torch.equal(v, ck["0." + k]), k


def test_constructor_refuses_other_feature_sizes_and_cpu_forward():
    from speech_anonymization_amd import fcae
    from speech_anonymization_amd._lib import SaHipError
    with pytest.raises(SaHipError):
        fcae.FullyConnectedAutoencoder(40, 3)
    with pytest.raises(SaHipError, match="GPU only"):
        fcae.FullyConnectedAutoencoder(80, 3)(torch.zeros(3, 10, 80))


def _fixture_model(z, dtype):
    m = R.FullyConnectedAutoencoder(80, 3)
    m.load_state_dict({k[len("init/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init/")})
    return m.to(dtype)


def _sub(t, n=2048):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n]


def test_restatement_fp32_reproduces_the_reference_fixture_bit_for_bit():
    torch.set_num_threads(1)
    z = np.load(os.path.join(GOLD, "fcae_S.npz"))
    feats, gender = torch.from_numpy(z["feats"]), torch.from_numpy(z["gender"])
    m = _fixture_model(z, torch.float32)
    tr = R.run_step(m, feats, gender, True)
    for k in ("recon", "logp", "loss"):
        assert np.array_equal(tr[k].numpy(), z[k]), k
    assert len(tr["grads"]) == 30
    for k, g in tr["grads"].items():
        assert np.array_equal(_sub(g).numpy(), z["grad_sub/" + k]), k
    for k, v in tr["buffers"].items():
        assert np.array_equal(v.numpy(), z["buffer/" + k]), k
    ev = R.run_step(m, feats, gender, False)
    assert np.array_equal(ev["logp"].numpy(), z["eval_logp"])
    assert np.array_equal(_sub(ev["recon"]).numpy(), z["eval_recon_sub"])


def test_restatement_fp64_agrees_with_the_fixture_to_fp32_noise():
    z = np.load(os.path.join(GOLD, "fcae_S.npz"))
    feats, gender = torch.from_numpy(z["feats"]).double(), torch.from_numpy(z["gender"])
    tr = R.run_step(_fixture_model(z, torch.float64), feats, gender, True)
    for k in ("recon", "logp", "loss"):
        e = R.relmse(torch.from_numpy(z[k]), tr[k])
        assert e <= FP32_NOISE_BAR, (k, e)
    for k, g in tr["grads"].items():
        fix = torch.from_numpy(z["grad_sub/" + k])
        if k in ZERO_GRADS:
            # mathematically zero: fp64 leaves ~1e-14, the reference's fp32 up to ~1e-5
            assert float(g.abs().max()) < 1e-10 and float(fix.abs().max()) < 1e-3, k
            continue
        e = R.relmse(fix, _sub(g))
        assert e <= FP32_NOISE_BAR, (k, e)
    for k, v in tr["buffers"].items():
        if "running" in k:
            e = R.relmse(torch.from_numpy(z["buffer/" + k]), v)
            assert e <= FP32_NOISE_BAR, (k, e)


def test_library_exports_the_fcae_entry_points():
    import __graft_entry__ as g
    g.build()
    from speech_anonymization_amd import _lib
    names = ["sa_fc_tiles", "sa_fc_groups", "sa_fc_nparam", "sa_fc_nhead", "sa_fc_max_rows", "sa_fc_enc_fwd",
             "sa_fc_bn_fin", "sa_fc_mid_fwd", "sa_fc_head_fwd", "sa_fc_head_bwd", "sa_fc_mid_bwd", "sa_fc_bn_bwd_fin",
             "sa_fc_enc_bwd", "sa_fc_wreduce"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    # no GPU is touched by the geometry queries and by refused arguments
    assert lib.sa_fc_nparam() == 18780 and lib.sa_fc_nparam() + lib.sa_fc_nhead() + 40 == 24682
    assert lib.sa_fc_max_rows() >= 64
    assert lib.sa_fc_tiles(1008) == 16 and lib.sa_fc_tiles(2) == 1 and lib.sa_fc_tiles(65) == 2
    assert lib.sa_fc_groups(32, 1008) == 256 and lib.sa_fc_groups(3, 100) == 6
    assert lib.sa_fc_groups(3, 1) == -22 and lib.sa_fc_wreduce(None, 4, None, None) == -22
    assert lib.sa_fc_enc_fwd(None, None, None, None, None, None, 3, 100, None) == -22


def test_entry_script_accepts_fcae_and_refuses_it_data_parallel():
    import speechbrain_convae_train as entry
    assert entry.MODEL_TYPES == ("convae", "fcae", "endtoend")
    for t in entry.MODEL_TYPES:
        entry.check_model_type(t, {}, environ={})
    with pytest.raises(SystemExit) as e:
        entry.check_model_type("mlp", {}, environ={})
    assert all(t in str(e.value) for t in entry.MODEL_TYPES) and "\n" not in str(e.value)
    with pytest.raises(SystemExit) as e:
        entry.check_model_type("fcae", {"distributed_launch": True}, environ={})
    assert "fcae" in str(e.value) and "\n" not in str(e.value)
    with pytest.raises(SystemExit):
        entry.check_model_type("fcae", {}, environ={"WORLD_SIZE": "2"})
    entry.check_model_type("convae", {"distributed_launch": True}, environ={"WORLD_SIZE": "2"})


def test_entry_script_refuses_fcae_data_parallel_before_any_device(tmp_path, monkeypatch):
    """through main(): the message comes before a process group or a GPU is touched.  The process-group set-up is
    replaced by a tripwire, so an entry script that reached it would fail here at once instead of waiting for a
    second rank that never comes."""
    import speechbrain_convae_train as entry

    def tripwire(*a, **kw):
        raise AssertionError("the process group was set up before model_type fcae was refused")
    monkeypatch.setattr(entry.sdist, "ddp_init_group", tripwire)
    cfg = os.path.join(ROOT, "speechbrain_configs", "convae.yaml")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        entry.main([cfg, "--model_type", "fcae", "--folder", str(tmp_path), "--synthetic", "6"])
    assert "one GPU" in str(e.value)
