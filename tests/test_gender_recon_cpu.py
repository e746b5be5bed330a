"""The gender-classifier recipe on reconstructed features, host side (no GPU): the config, the refusals of
gender_classifier_train_recon.py, the mapping of a speechbrain_convae_train.py checkpoint onto the anonymiser,
GenderReconBrain.prepare_features on stub modules, and who owns which parameter."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "speechbrain_configs", "gender_classifier_recon.yaml")
GOLD = os.path.join(ROOT, "tests", "golden")


def _settings(tmp_path, **over):
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    with open(CFG) as f:
        return load_hyperpyyaml(f, dict({"output_folder": str(tmp_path)}, **over))


def test_config_holds_plain_settings_with_the_reference_values(tmp_path):
    text = open(CFG).read()
    assert "!" not in text.replace("# ", "")           # no tags: values only
    st = _settings(tmp_path)
    assert (st["number_of_epochs"], st["batch_size"], st["adam_lr"], st["classes"]) == (10, 32, 0.001, 2)
    assert st["plateau"] == {"factor": 0.5, "patience": 2, "hold_until_epoch": 2}
    assert st["xvector"]["embedding_dim"] == 128
    assert st["xvector"]["channels"] == [512, 512, 512, 512, 1500]
    assert st["fbank"] == {"sample_rate": 16000, "n_fft": 400, "n_mels": 80}
    assert (st["model_type"], st["recon_ckpt"], st["recon_normalizer"]) == ("fcae", None, "own")

    def plain(v):
        if isinstance(v, dict):
            return all(plain(x) for x in v.values())
        if isinstance(v, list):
            return all(plain(x) for x in v)
        return v is None or isinstance(v, (bool, int, float, str))
    assert plain(st)
    from speech_anonymization_amd import gender
    hp = gender.build(st)
    assert hp["epoch_counter"].limit == 10
    s = hp["lr_annealing"]
    assert (s.factor, s.patience, s.dont_halve_until_epoch) == (0.5, 2, 2)
    assert set(hp["checkpointer"].recoverables) == {"embedding_model", "classifier", "normalizer", "counter"}


def test_command_line_reaches_the_settings():
    from speech_anonymization_amd.yaml_loader import parse_arguments
    f, run, ov = parse_arguments([CFG, "--device", "cuda:0", "--recon_ckpt", "/x/CKPT+1", "--model_type", "convae",
                                  "--synthetic", "64", "--recon_normalizer", "checkpoint"])
    assert f == CFG and run == {"device": "cuda:0"}
    assert ov == {"recon_ckpt": "/x/CKPT+1", "model_type": "convae", "synthetic": 64, "recon_normalizer": "checkpoint"}


@pytest.mark.parametrize("settings,run_opts,environ,words", [
    (dict(model_type="cyclegan", recon_ckpt="/x"), {}, {}, ("unknown model_type", "cyclegan")),
    (dict(model_type="fcae", recon_ckpt=None), {}, {}, ("--recon_ckpt",)),
    (dict(model_type="fcae", recon_ckpt="/x"), {"distributed_launch": True}, {}, ("one GPU",)),
    (dict(model_type="convae", recon_ckpt="/x"), {}, {"WORLD_SIZE": "2"}, ("one GPU",)),
    (dict(model_type="convae", recon_ckpt="/x"), {"hip_graph": True}, {}, ("--hip_graph",)),
    (dict(model_type="convae", recon_ckpt="/x", hip_graph=True), {}, {}, ("--hip_graph",)),
    (dict(model_type="fcae", recon_ckpt="/x", recon_normalizer="theirs"), {}, {}, ("recon_normalizer",)),
])
def test_refusals_are_one_line_each(settings, run_opts, environ, words):
    from speech_anonymization_amd import gender
    with pytest.raises(SystemExit) as e:
        gender.check_recon_options(settings, run_opts, environ=environ)
    msg = str(e.value)
    assert "\n" not in msg
    for w in words:
        assert w in msg, msg


def test_accepted_options_pass():
    from speech_anonymization_amd import gender
    for mt in ("convae", "fcae", "endtoend"):
        gender.check_recon_options(dict(model_type=mt, recon_ckpt="/x", recon_normalizer="checkpoint"), {},
                                   environ={"WORLD_SIZE": "1"})


def test_entry_script_refuses_before_anything_is_built(tmp_path):
    """main() with no --recon_ckpt exits in one line; nothing is written"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gctr", os.path.join(ROOT, "gender_classifier_train_recon.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        mod.main([CFG, "--device", "cpu", "--model_type", "fcae", "--output_folder", str(out)])
    assert "--recon_ckpt" in str(e.value) and "\n" not in str(e.value)
    assert not out.exists()


def _fcae_ckpt_dir(tmp_path):
    """a CKPT+* directory as speechbrain_convae_train.py writes it, from the trained reference weights"""
    z = np.load(os.path.join(GOLD, "fcae_trained.npz"))
    ck = {k[len("ckpt/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("ckpt/")}
    assert all(k.startswith("0.") for k in ck)
    d = tmp_path / "CKPT+fcae"
    d.mkdir()
    torch.save(ck, d / "model.ckpt")
    torch.save({"count": 7, "glob_mean": torch.arange(80.0), "glob_std": torch.full((80,), 2.0), "spk_dict_mean": {},
                "spk_dict_std": {}, "spk_dict_count": {}}, d / "normalizer.ckpt")
    return str(d), ck


def test_checkpoint_keys_map_onto_the_named_model(tmp_path):
    from speech_anonymization_amd import fcae, gender
    d, ck = _fcae_ckpt_dir(tmp_path)
    model = gender.build_anonymiser("fcae", batch_size=8)
    assert isinstance(model, fcae.FullyConnectedAutoencoder)
    out = gender.load_anonymiser(model, d)
    assert out is model and not model.training
    sd = model.state_dict()
    assert set(sd) == {k[2:] for k in ck}
    for k, v in ck.items():
        assert torch.equal(sd[k[2:]], v), k
    assert not any(p.requires_grad for p in model.parameters())
    # the same file offered as another model_type: one line naming the first missing key
    conv = gender.build_anonymiser("convae")
    first = next(k for k in conv.state_dict() if "0." + k not in ck)
    assert first == "encoder.3.weight"                  # (encoder.0 / encoder.2 exist in both models)
    with pytest.raises(SystemExit) as e:
        gender.load_anonymiser(conv, d)
    msg = str(e.value)
    assert "\n" not in msg and "missing key" in msg and repr(first) in msg and "ConvAutoencoder" in msg
    # a key too many is refused as well (strict)
    torch.save(dict(ck, **{"0.extra.weight": torch.zeros(1)}), os.path.join(d, "model.ckpt"))
    with pytest.raises(SystemExit) as e:
        gender.load_anonymiser(gender.build_anonymiser("fcae"), d)
    assert "unexpected key 'extra.weight'" in str(e.value) and "\n" not in str(e.value)
    with pytest.raises(SystemExit) as e:
        gender.load_anonymiser(gender.build_anonymiser("fcae"), str(tmp_path / "nowhere"))
    assert "model.ckpt" in str(e.value)


def test_checkpoint_normaliser_is_loaded_frozen(tmp_path):
    from speech_anonymization_amd import gender
    d, _ = _fcae_ckpt_dir(tmp_path)
    n = gender.load_recon_normalizer(d)
    assert not n.training and n.update_until_epoch == 0
    assert n.count == 7 and torch.equal(n.glob_mean, torch.arange(80.0)) and torch.equal(n.glob_std, torch.full((80,), 2.0))
    os.remove(os.path.join(d, "normalizer.ckpt"))
    with pytest.raises(SystemExit) as e:
        gender.load_recon_normalizer(d)
    assert "normalizer.ckpt" in str(e.value)


class _Fbank(torch.nn.Module):
    def forward(self, wavs):
        return wavs.unsqueeze(-1).repeat(1, 1, 80)[:, :6]


class _Norm(torch.nn.Module):
    """stands for InputNormalization: y = (x - shift); records every call and whether it would have updated"""

    def __init__(self, shift):
        super().__init__()
        self.shift, self.calls, self.updates, self.epochs = shift, 0, 0, []

    def forward(self, feats, lens, epoch=0):
        self.calls += 1
        self.updates += int(self.training)
        self.epochs.append(epoch)
        return feats - self.shift


class _Anonymiser(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.seen = []

    def reconstruct(self, feats):
        self.seen.append((feats.clone(), self.training))
        return 2.0 * feats

    def forward(self, feats):
        raise AssertionError("the recipe must call reconstruct, never forward")


@pytest.mark.parametrize("which", ["own", "checkpoint"])
def test_prepare_features_feeds_the_reconstruction_on(which):
    from speech_anonymization_amd import gender
    from speech_anonymization_amd.brain import Stage
    own, theirs, model = _Norm(1.0), _Norm(5.0).eval(), _Anonymiser()
    brain = gender.GenderReconBrain(modules={"compute_features": _Fbank(), "mean_var_norm": own, "model": model},
                                    hparams={"recon_normalizer": which, "recon_norm": theirs},
                                    run_opts={"device": "cpu"})
    wavs, lens = torch.arange(24.0).reshape(2, 12), torch.ones(2)
    feats = _Fbank()(wavs)
    brain.modules.train()                               # what Brain.fit does, the anonymiser included
    out = brain.prepare_features(wavs, lens, Stage.TRAIN)
    want_in = feats - (1.0 if which == "own" else 5.0)
    assert len(model.seen) == 1 and torch.equal(model.seen[0][0], want_in)
    assert torch.equal(out, 2.0 * want_in) and out.shape == (2, 6, 80)
    # the recipe's own global normaliser follows every training batch, with no epoch passed
    assert (own.calls, own.updates, own.epochs) == (1, 1, [0])
    # the anonymiser's normaliser is outside Brain.modules, stays in eval mode and is never updated
    assert theirs.updates == 0 and not theirs.training and theirs.calls == (1 if which == "checkpoint" else 0)
    brain.modules.eval()
    brain.prepare_features(wavs, lens, Stage.VALID)
    assert (own.calls, own.updates) == (2, 1) and theirs.updates == 0


def test_anonymiser_is_neither_optimised_nor_checkpointed(tmp_path):
    from speech_anonymization_amd import gender
    d, _ = _fcae_ckpt_dir(tmp_path)
    st = _settings(tmp_path / "run", recon_ckpt=d, model_type="fcae")
    model = gender.load_anonymiser(gender.build_anonymiser("fcae", batch_size=st["batch_size"]), d)
    hp = dict(st, **gender.build(st))
    hp["modules"]["model"] = model
    b = gender.GenderReconBrain(modules=hp["modules"], opt_class=hp["opt_class"], hparams=hp, run_opts={"device": "cpu"},
                                checkpointer=hp["checkpointer"])
    b.on_fit_start()
    assert b.modules["model"] is model                  # still there for prepare_features
    mine = {id(p) for p in model.parameters()} | {id(t) for t in model.buffers()}
    in_opt = {id(p) for g in b.optimizer.param_groups for p in g["params"]}
    assert in_opt and not (in_opt & mine)
    want = {id(p) for k in ("embedding_model", "classifier") for p in b.modules[k].parameters()}
    assert in_opt == want
    rec = hp["checkpointer"].recoverables
    assert set(rec) == {"embedding_model", "classifier", "normalizer", "counter", "optimizer"}
    for obj in rec.values():
        if isinstance(obj, torch.nn.Module):
            assert obj is not model and not ({id(p) for p in obj.parameters()} & mine)
    assert not any(p.requires_grad for p in model.parameters())
