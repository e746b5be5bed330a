#!/usr/bin/env python3
"""Trains the x-vector gender classifier on McADAMS-TRANSFORMED waveforms: the informed attacker of VoicePrivacy's
signal-processing baseline (B2; B1.b with a coefficient per utterance).  Every waveform, at train, valid and test
alike, has the poles of its frame-wise LPC filter moved from angle phi to phi^alpha before the classifier's front
end sees it (speech_anonymization_amd.mcadams).  Its test error answers "how much of sex does a
classifier still recover when it is trained on the anonymised speech itself?".

    python gender_classifier_train_mcadams.py speechbrain_configs/gender_classifier_mcadams.yaml \
        --device cuda:0 [--mcadams A | --mcadams_min LO --mcadams_max HI] [--synthetic N] [--key value ...]

``--mcadams A`` uses one coefficient for every utterance; ``--mcadams_min LO --mcadams_max HI`` draws one per
utterance from [LO, HI] (deterministic in the ``mcadams_options`` block's seed and the batch count).  One GPU, no
--hip_graph.

Everything else is gender_classifier_train.py: manifests or ``--synthetic N``, the checkpoint layout, the JSON
summary as the last line (with the alpha settings added)."""
import json
import os
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender, mcadams
from speech_anonymization_amd.yaml_loader import load_hyperpyyaml, parse_arguments


def main(argv):
    hparams_file, run_opts, overrides = parse_arguments(argv)
    synthetic = overrides.pop("synthetic", None)
    with open(hparams_file) as fin:
        settings = load_hyperpyyaml(fin, overrides)
    opts = mcadams.check_recipe_options(settings, run_opts)
    os.makedirs(settings["output_folder"], exist_ok=True)
    print(gender.augment_notice("gender_classifier_train_mcadams", settings))
    hparams = dict(settings, **gender.build(settings))
    hparams["pitch_normalizer"] = mcadams.McAdams(**opts)       # (the brain's hook for a waveform transform)
    run_opts.setdefault("max_grad_norm", settings.get("max_grad_norm", 5.0))
    brain = gender.GenderPitchNormBrain(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams,
                                        run_opts=run_opts, checkpointer=hparams["checkpointer"])
    counter = hparams["epoch_counter"]
    train, valid, test = gender.loaders(hparams, synthetic, counter)
    brain.fit(counter, train, valid)
    brain.evaluate(test, min_key="error")
    summary = {"test_loss": brain.last_stats["loss"], "test_error": brain.last_stats["error"],
               "best_checkpoint": getattr(brain, "best_checkpoint", None), "mcadams": True}
    summary.update({k: (list(v) if isinstance(v, tuple) else v) for k, v in opts.items()})
    print(json.dumps(summary))


if __name__ == "__main__":
    main(sys.argv[1:])
