#!/usr/bin/env python3
"""Trains the external x-vector gender classifier (the reference's gender_classifier_train.py):

    python gender_classifier_train.py speechbrain_configs/gender_classifier.yaml \
        --device cuda:0 [--key value overrides]

It reads the CSV manifests named under ``manifests`` (column ``gender``: M / F) in ``data_folder``; ``--synthetic N`` trains on N generated utterances instead (two classes
separable by pitch, data.synthetic_gender_dataset; held-out validation and test sets of N/4 each).
The best checkpoint by validation error, under ``<save_folder>/CKPT+*``, is the directory
``speechbrain_convae_train.py --external_classifier_ckpt`` takes.  The last line printed is a JSON
summary (test loss and error, the checkpoint used)."""
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
    os.makedirs(settings["output_folder"], exist_ok=True)
    print(gender.augment_notice("gender_classifier_train", settings))
    hparams = dict(settings, **gender.build(settings))
    run_opts.setdefault("max_grad_norm", settings.get("max_grad_norm", 5.0))
    brain = gender.GenderBrain(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams,
                               run_opts=run_opts, checkpointer=hparams["checkpointer"])
    counter = hparams["epoch_counter"]
    train, valid, test = gender.loaders(hparams, synthetic, counter)
    brain.fit(counter, train, valid)
    brain.evaluate(test, min_key="error")
    print(json.dumps({"test_loss": brain.last_stats["loss"], "test_error": brain.last_stats["error"],
                      "best_checkpoint": getattr(brain, "best_checkpoint", None)}))


if __name__ == "__main__":
    main(sys.argv[1:])
