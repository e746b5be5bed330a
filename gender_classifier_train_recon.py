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
from speech_anonymization_amd import gender
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
    counter = hparams["epoch_counter"]
    train, valid, test = gender.loaders(hparams, synthetic, counter)
    brain.fit(counter, train, valid)
    brain.evaluate(test, min_key="error")
    print(json.dumps({"test_loss": brain.last_stats["loss"], "test_error": brain.last_stats["error"],
                      "best_checkpoint": getattr(brain, "best_checkpoint", None),
                      "recon_ckpt": settings["recon_ckpt"], "model_type": settings["model_type"]}))


if __name__ == "__main__":
    main(sys.argv[1:])
