"""The gender-classifier recipe on the host side (no GPU): speechbrain's ReduceLROnPlateau as
restated in speech_anonymization_amd.gender, the config and its CLASS_MAP entries, the command
line, and the checkpoint layout that speechbrain_convae_train.py --external_classifier_ckpt reads."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "speechbrain_configs", "gender_classifier.yaml")


class _Opt:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]


def test_reduce_lr_on_plateau_hand_worked():
    """factor 0.5, patience 2, dont_halve_until_epoch 2 (the recipe's settings), worked by hand:
    epochs 1-2 only move the anchor (to 1.0, then 0.9); 3: 0.95 > 0.9 -> patience 1; 4: 0.92 ->
    patience 2; 5: 0.91, patience spent -> halve, counter reset; 6: 0.8 <= 0.9 -> new anchor;
    7, 8, 9: worse three times -> halve at 9; lr_min bounds the result."""
    from speech_anonymization_amd.gender import ReduceLROnPlateau, update_learning_rate
    s = ReduceLROnPlateau(factor=0.5, patience=2, dont_halve_until_epoch=2)
    opt = _Opt(1e-3)
    losses = [1.0, 0.9, 0.95, 0.92, 0.91, 0.8, 0.85, 0.81, 0.9]
    want_next = [1e-3, 1e-3, 1e-3, 1e-3, 5e-4, 5e-4, 5e-4, 5e-4, 2.5e-4]
    want_anchor = [1.0, 0.9, 0.9, 0.9, 0.9, 0.8, 0.8, 0.8, 0.8]
    for ep, (loss, nl, an) in enumerate(zip(losses, want_next, want_anchor), start=1):
        old, new = s([opt], ep, loss)
        assert old == opt.param_groups[0]["lr"]
        assert new == pytest.approx(nl, rel=0, abs=1e-15), ep
        assert s.anchor == an, ep
        update_learning_rate(opt, new)
    assert s.losses == losses
    s2 = ReduceLROnPlateau(lr_min=3e-4, factor=0.5, patience=0, dont_halve_until_epoch=0)
    opt = _Opt(1e-3)
    assert s2([opt], 1, 1.0) == (1e-3, 1e-3)
    assert s2([opt], 2, 2.0) == (1e-3, 5e-4)
    update_learning_rate(opt, 5e-4)
    assert s2([opt], 3, 3.0) == (5e-4, 3e-4)            # 2.5e-4 bounded below
    sd = s2.state_dict()
    s3 = ReduceLROnPlateau()
    s3.load_state_dict(sd)
    assert (s3.anchor, s3.patience_counter, s3.losses) == (1.0, 0, [1.0, 2.0, 3.0])


def test_class_map_and_config(tmp_path):
    """the recipe's config holds plain settings; gender.build() makes the objects from them.  The
    CLASS_MAP entries let a speechbrain-style YAML that names the x-vector classes load too."""
    from speech_anonymization_amd import brain, checkpoint, features, gender, losses, xvector
    from speech_anonymization_amd.yaml_loader import CLASS_MAP, Unavailable, load_hyperpyyaml
    assert CLASS_MAP["speechbrain.lobes.models.Xvector.Xvector"] == "speech_anonymization_amd.xvector.Xvector"
    assert CLASS_MAP["speechbrain.lobes.models.Xvector.Classifier"] == "speech_anonymization_amd.xvector.Classifier"
    assert CLASS_MAP["speechbrain.nnet.schedulers.ReduceLROnPlateau"] == "speech_anonymization_amd.gender.ReduceLROnPlateau"
    text = open(CFG).read()
    assert "!" not in text.replace("# ", "")           # no tags: values only
    with open(CFG) as f:
        st = load_hyperpyyaml(f, {"output_folder": str(tmp_path)})
    assert (st["batch_size"], st["number_of_epochs"], st["adam_lr"], st["classes"]) == (32, 8, 0.001, 2)
    hp = gender.build(st)
    m = hp["modules"]
    assert set(m) == {"compute_features", "embedding_model", "classifier", "mean_var_norm"}
    assert isinstance(m["compute_features"], features.Fbank)
    assert isinstance(m["mean_var_norm"], features.InputNormalization)
    assert isinstance(m["embedding_model"], xvector.Xvector) and isinstance(m["classifier"], xvector.Classifier)
    assert [b.conv.kernel_size for b in m["embedding_model"].blocks[0:15:3]] == [(5,), (3,), (3,), (1,), (1,)]
    assert [b.dilation for b in m["embedding_model"].blocks[0:15:3]] == [1, 2, 3, 1, 1]
    assert m["embedding_model"].blocks[12].conv.out_channels == 1500
    assert m["classifier"].out.w.out_features == 2
    assert not m["embedding_model"].training             # constructed in eval mode
    s = hp["lr_annealing"]
    assert isinstance(s, gender.ReduceLROnPlateau)
    assert (s.factor, s.patience, s.dont_halve_until_epoch) == (0.5, 2, 2)
    assert hp["opt_class"].func is torch.optim.Adam and hp["opt_class"].keywords == {"lr": 0.001}
    assert isinstance(hp["compute_cost"], losses.NLLLoss)
    assert isinstance(hp["epoch_counter"], brain.EpochCounter) and hp["epoch_counter"].limit == 8
    ck = hp["checkpointer"]
    assert isinstance(ck, checkpoint.Checkpointer) and ck.checkpoints_dir == os.path.join(str(tmp_path), "save")
    assert ck.recoverables["embedding_model"] is m["embedding_model"]
    assert ck.recoverables["normalizer"] is m["mean_var_norm"]
    assert ck.recoverables["counter"] is hp["epoch_counter"]
    # the seed fixes the initial weights
    again = gender.build(st)["modules"]["embedding_model"]
    assert torch.equal(again.blocks[0].conv.weight, m["embedding_model"].blocks[0].conv.weight)
    # a speechbrain-style YAML naming the classes resolves them; augmentation stays a placeholder
    y = ("emb: !new:speechbrain.lobes.models.Xvector.Xvector\n    in_channels: 80\n"
         "cls: !new:speechbrain.lobes.models.Xvector.Classifier\n    input_shape: [null, null, 128]\n"
         "sched: !new:speechbrain.nnet.schedulers.ReduceLROnPlateau\n    patience: 1\n"
         "corrupt: !new:speechbrain.lobes.augment.EnvCorrupt\n    noise_prob: 1.0\n")
    hp2 = load_hyperpyyaml(y)
    assert isinstance(hp2["emb"], xvector.Xvector) and isinstance(hp2["cls"], xvector.Classifier)
    assert isinstance(hp2["sched"], gender.ReduceLROnPlateau) and hp2["sched"].patience == 1
    assert isinstance(hp2["corrupt"], Unavailable)


def test_argument_parsing():
    from speech_anonymization_amd.yaml_loader import parse_arguments
    f, run, ov = parse_arguments([CFG, "--device", "cuda:0", "--synthetic", "96", "--number_of_epochs", "4",
                                  "--output_folder=/x/y"])
    assert f == CFG
    assert run == {"device": "cuda:0"}
    assert ov == {"synthetic": 96, "number_of_epochs": 4, "output_folder": "/x/y"}


def _brain(tmp_path):
    from speech_anonymization_amd import gender
    from speech_anonymization_amd.yaml_loader import load_hyperpyyaml
    with open(CFG) as f:
        st = load_hyperpyyaml(f, {"output_folder": str(tmp_path)})
    hp = dict(st, **gender.build(st))
    b = gender.GenderBrain(modules=hp["modules"], opt_class=hp["opt_class"], hparams=hp,
                           run_opts={"device": "cpu"}, checkpointer=hp["checkpointer"])
    b.on_fit_start()
    return b, hp


def test_checkpoint_layout_and_best_by_error(tmp_path):
    from speech_anonymization_amd import gender
    from speech_anonymization_amd.brain import Stage
    b, hp = _brain(tmp_path)
    with torch.no_grad():                       # distinguishable weights per epoch
        for p in b.modules.embedding_model.parameters():
            p.normal_()
    for ep, (err, loss) in enumerate([(0.3, 0.7), (0.1, 0.5), (0.2, 0.6)], start=1):
        hp["epoch_counter"].current = ep
        b.train_loss = 1.0
        b.on_stage_start(Stage.VALID, ep)
        b.n_err, b.n_utt = int(err * 10), 10
        b.on_stage_end(Stage.VALID, loss, ep)
        if ep == 2:
            best_w = b.modules.embedding_model.blocks[0].conv.weight.detach().clone()
        with torch.no_grad():
            b.modules.embedding_model.blocks[0].conv.weight.add_(1.0)
    ck = hp["checkpointer"].find_checkpoints(min_key="error")
    assert len(ck) == 2                         # the best and the most recent are kept
    best = ck[0]
    assert set(os.listdir(best)) == {"embedding_model.ckpt", "classifier.ckpt", "normalizer.ckpt", "counter.ckpt",
                                     "optimizer.ckpt", "CKPT.yaml", "label_encoder.txt"}
    import yaml
    meta = yaml.safe_load(open(os.path.join(best, "CKPT.yaml")))
    assert meta["error"] == pytest.approx(0.1) and meta["loss"] == pytest.approx(0.5)
    assert open(os.path.join(best, "counter.ckpt")).read() == "2"
    assert open(os.path.join(best, "label_encoder.txt")).read().splitlines()[:2] == ["'M' => 0", "'F' => 1"]
    assert os.path.exists(os.path.join(str(tmp_path), "train_log.txt"))
    # halving follows the validation losses 0.7, 0.5, 0.6: none yet (patience 2)
    assert b.optimizer.param_groups[0]["lr"] == 0.001
    clf = gender.load_external_classifier(best)
    assert torch.equal(clf.embedding_model.blocks[0].conv.weight, best_w)


def test_state_dicts_round_trip_into_encoder_classifier(tmp_path):
    """CPU-built Xvector / Classifier state dicts -> the checkpoint files -> EncoderClassifier,
    strict, with every tensor equal (the keys of the reference's classifier.ckpt)."""
    from speech_anonymization_amd import gender, xvector
    from speech_anonymization_amd.brain import Stage
    b, hp = _brain(tmp_path)
    with torch.no_grad():
        for m in (b.modules.embedding_model, b.modules.classifier):
            for t in list(m.parameters()) + [x for n, x in m.named_buffers() if "running" in n]:
                t.uniform_(0.5, 1.5)
    hp["epoch_counter"].current = 1
    b.train_loss = 1.0
    b.on_stage_start(Stage.VALID, 1)
    b.on_stage_end(Stage.VALID, 0.5, 1)
    d = hp["checkpointer"].find_checkpoints(min_key="error")[0]
    enc = xvector.EncoderClassifier()
    for name, mod in (("embedding_model", enc.embedding_model), ("classifier", enc.classifier)):
        sd = torch.load(os.path.join(d, name + ".ckpt"), map_location="cpu", weights_only=True)
        mod.load_state_dict(sd, strict=True)
        ref = b.modules[name].state_dict()
        assert sd.keys() == ref.keys()
        for k in ref:
            assert torch.equal(sd[k], ref[k]), k
    assert "norm.norm.weight" in enc.classifier.state_dict()
    assert "DNN.block_0.linear.w.weight" in enc.classifier.state_dict()
    assert "blocks.16.w.weight" in enc.embedding_model.state_dict()
    clf = gender.load_external_classifier(d)
    assert not clf.training
