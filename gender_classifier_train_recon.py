#!/usr/bin/env python3
"""Trains the x-vector gender classifier on RECONSTRUCTED features (the reference's
gender_classifier_train_recon.py): a trained anonymiser runs in inference on every batch and the classifier
of gender_classifier_train.py learns from its output.  Its test error answers "how well does an attacker who
knows the anonymiser recover sex from what it emits?".

    python gender_classifier_train_recon.py speechbrain_configs/gender_classifier_recon.yaml \
        --device cuda:0 --recon_ckpt DIR --model_type fcae|convae|endtoend [--synthetic N] [--key value ...]

DIR is a CKPT+* directory written by speechbrain_convae_train.py (model.ckpt with the ModuleList's ``0.``
keys, normalizer.ckpt).  ``--recon_normalizer checkpoint`` puts the anonymiser's own normaliser in front of
it instead of the recipe's fresh one.  model_type endtoend also takes
``--external_classifier_ckpt DIR`` for its frozen in-graph classifier, which this recipe never runs.
Everything else is gender_classifier_train.py: manifests or ``--synthetic N``, the checkpoint layout, the JSON
summary as the last line (with recon_ckpt and model_type added)."""
import json
import os
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import data, gender
from speech_anonymization_amd.yaml_loader import load_hyperpyyaml, parse_arguments


def main(argv):
    hparams_file, run_opts, overrides = parse_arguments(argv)
    synthetic = overrides.pop("synthetic", None)
    with open(hparams_file) as fin:
        settings = load_hyperpyyaml(fin, overrides)
    gender.check_recon_options(settings, run_opts)
    os.makedirs(settings["output_folder"], exist_ok=True)
    print(gender.augment_notice("gender_classifier_train_recon", settings))
    ext = None
    if settings["model_type"] == "endtoend" and settings.get("external_classifier_ckpt"):
        ext = gender.load_external_classifier(settings["external_classifier_ckpt"])
    model = gender.load_anonymiser(
        gender.build_anonymiser(settings["model_type"], settings.get("precision", "bf16x3"), ext,
                                int(settings["batch_size"])), settings["recon_ckpt"])
    hparams = dict(settings, **gender.build(settings))
    if settings.get("recon_normalizer", "own") == "checkpoint":
        hparams["recon_norm"] = gender.load_recon_normalizer(settings["recon_ckpt"])
    hparams["modules"]["model"] = model                    # frozen: not a recoverable, not in the optimiser
    run_opts.setdefault("max_grad_norm", settings.get("max_grad_norm", 5.0))
    brain = gender.GenderReconBrain(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams,
                                    run_opts=run_opts, checkpointer=hparams["checkpointer"])
    bs, seed = int(hparams["batch_size"]), int(hparams["seed"])
    counter = hparams["epoch_counter"]
    if synthetic:
        n = int(synthetic)
        held = max(bs, n // 4)
        make = lambda k, s, ep=0: data.synthetic_gender_dataset(k, bs, seed=s + ep)
        train = lambda epoch: make(n, seed, 1000 * epoch)
        valid = lambda epoch: make(held, seed + 1)
        test = lambda: make(held, seed + 2)
    else:
        rep = {"data_root": hparams["data_folder"]}
        csv = {k: os.path.join(hparams["data_folder"], v) for k, v in hparams["manifests"].items()}
        tr = data.CsvDataset(csv["train"], rep)
        va = data.CsvDataset(csv["valid"], rep, "ascending")
        te = data.CsvDataset(csv["test"], rep, "ascending")
        train = lambda epoch: data.batches(tr, bs, bool(hparams.get("shuffle", True)), seed, epoch=epoch)
        valid = lambda epoch: data.batches(va, bs)
        test = lambda: data.batches(te, bs)

    class Loader:
        def __init__(self, f):
            self.f = f

        def __iter__(self):
            return iter(self.f(max(1, int(counter.current))))

    brain.fit(counter, Loader(train), Loader(valid))
    brain.evaluate(test(), min_key="error")
    print(json.dumps({"test_loss": brain.last_stats["loss"], "test_error": brain.last_stats["error"],
                      "best_checkpoint": getattr(brain, "best_checkpoint", None),
                      "recon_ckpt": settings["recon_ckpt"], "model_type": settings["model_type"]}))


if __name__ == "__main__":
    main(sys.argv[1:])
