#!/usr/bin/env python3
"""Trains the x-vector gender classifier on TEMPO-CHANGED waveforms: the informed attacker of the time-scale
modification.  Every waveform, at train, valid and test alike, is played at another tempo by WSOLA
(speech_anonymization_amd.timescale) before the classifier's front end sees it: pitch and spectral
envelope stay, the duration changes, and the changed lengths go on to the normaliser and the pooling.  Its test error
answers "how much of sex does a classifier still recover once the speaking rate is moved, or scattered?".

    python gender_classifier_train_tempo.py speechbrain_configs/gender_classifier_tempo.yaml \
        --device cuda:0 [--tempo X | --tempo_min LO --tempo_max HI] [--synthetic N] [--key value ...]

``--tempo X`` overrides ``tempo`` of the ``tempo_options`` block; ``--tempo_min LO --tempo_max HI`` draw one tempo per
utterance from a host generator seeded with the block's ``seed``.  One GPU, no --hip_graph.

Everything else is gender_classifier_train.py: manifests or ``--synthetic N``, the checkpoint layout, the JSON
summary as the last line (with the tempo settings added)."""
import json
import os
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender, timescale
from speech_anonymization_amd.yaml_loader import load_hyperpyyaml, parse_arguments


def main(argv):
    hparams_file, run_opts, overrides = parse_arguments(argv)
    synthetic = overrides.pop("synthetic", None)
    with open(hparams_file) as fin:
        settings = load_hyperpyyaml(fin, overrides)
    opts = timescale.check_recipe_options(settings, run_opts)
    os.makedirs(settings["output_folder"], exist_ok=True)
    print(gender.augment_notice("gender_classifier_train_tempo", settings))
    hparams = dict(settings, **gender.build(settings))
    hparams["time_scaler"] = timescale.TimeScaler(**opts)
    run_opts.setdefault("max_grad_norm", settings.get("max_grad_norm", 5.0))
    brain = gender.GenderTempoBrain(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams,
                                    run_opts=run_opts, checkpointer=hparams["checkpointer"])
    counter = hparams["epoch_counter"]
    train, valid, test = gender.loaders(hparams, synthetic, counter)
    brain.fit(counter, train, valid)
    brain.evaluate(test, min_key="error")
    summary = {"test_loss": brain.last_stats["loss"], "test_error": brain.last_stats["error"],
               "best_checkpoint": getattr(brain, "best_checkpoint", None), "tempo_mode": True}
    summary.update({k: (list(v) if isinstance(v, tuple) else v) for k, v in opts.items()})
    print(json.dumps(summary))


if __name__ == "__main__":
    main(sys.argv[1:])
