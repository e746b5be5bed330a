#!/usr/bin/env python3
"""Trains the x-vector gender classifier on MODULATION-SMOOTHED waveforms: the informed attacker of the
modulation-spectrum smoothing.  Every waveform, at train, valid and test alike, has the log magnitude of every STFT
bin low-pass filtered along time, its phases kept, and is inverted once (speech_anonymization_amd.modspec; DESIGN
section 28) before the classifier's front end sees it.  Its test error answers "how much of sex does a classifier
still recover once the fast fluctuations of every band's level -- articulation rate, rhythm, onset sharpness -- are
smoothed away?".

    python gender_classifier_train_modspec.py speechbrain_configs/gender_classifier_modspec.yaml \
        --device cuda:0 [--modspec_cutoff_hz X] [--modspec_depth D] [--synthetic N] [--key value ...]

``--modspec_cutoff_hz X`` and ``--modspec_depth D`` override ``cutoff_hz`` and ``depth`` of the ``modspec_options``
block.  The transform draws no random numbers.  One GPU, no --hip_graph.

Everything else is gender_classifier_train.py: manifests or ``--synthetic N``, the checkpoint layout, the JSON
summary as the last line (with the smoothing's settings added)."""
import json
import os
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender, modspec
from speech_anonymization_amd.yaml_loader import load_hyperpyyaml, parse_arguments


def main(argv):
    hparams_file, run_opts, overrides = parse_arguments(argv)
    synthetic = overrides.pop("synthetic", None)
    with open(hparams_file) as fin:
        settings = load_hyperpyyaml(fin, overrides)
    opts = modspec.check_recipe_options(settings, run_opts)
    os.makedirs(settings["output_folder"], exist_ok=True)
    print(gender.augment_notice("gender_classifier_train_modspec", settings))
    hparams = dict(settings, **gender.build(settings))
    hparams["pitch_normalizer"] = modspec.ModulationSmoother(**opts)  # (the brain's hook for a waveform transform)
    run_opts.setdefault("max_grad_norm", settings.get("max_grad_norm", 5.0))
    brain = gender.GenderPitchNormBrain(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams,
                                        run_opts=run_opts, checkpointer=hparams["checkpointer"])
    counter = hparams["epoch_counter"]
    train, valid, test = gender.loaders(hparams, synthetic, counter)
    brain.fit(counter, train, valid)
    brain.evaluate(test, min_key="error")
    summary = {"test_loss": brain.last_stats["loss"], "test_error": brain.last_stats["error"],
               "best_checkpoint": getattr(brain, "best_checkpoint", None), "modspec": True}
    summary.update(opts)
    print(json.dumps(summary))


if __name__ == "__main__":
    main(sys.argv[1:])
