#!/usr/bin/env python3
"""Trains the x-vector gender classifier on FORMANT-NORMALISED waveforms: the informed attacker of the formant
normalisation.  Every waveform, at train, valid and test alike, has its vocal-tract resonances brought to one target
before the classifier's front end sees it (speech_anonymization_amd.formantnorm): the utterance's
formants are tracked, and every frame's complex LPC poles move from angle phi to q phi with the ratio q that brings
them there.  Its test error answers "how much of sex does a classifier still recover when every vocal tract looks the
same length?"; with ``--pitch_norm true`` the pitch is normalised too (TD-PSOLA, which keeps the envelope), and both
cues end at their targets.

    python gender_classifier_train_formant_norm.py speechbrain_configs/gender_classifier_formant_norm.yaml \
        --device cuda:0 [--formant_target F1,F2,F3 | --formant_norm_ratio X] [--formant_q_min A --formant_q_max B]
        [--f0_method yin|viterbi] [--pitch_norm true [--pitch_target_hz 170]] [--synthetic N] [--key value ...]

One GPU, no --hip_graph.  Everything else is gender_classifier_train.py: manifests or ``--synthetic N``, the
checkpoint layout, the JSON summary as the last line (with the normaliser's settings added)."""
import json
import os
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import formantnorm, gender, pitchnorm
from speech_anonymization_amd.yaml_loader import load_hyperpyyaml, parse_arguments


def main(argv):
    hparams_file, run_opts, overrides = parse_arguments(argv)
    synthetic = overrides.pop("synthetic", None)
    flags = {k: overrides.pop(k) for k in ("formant_norm",) if k in overrides}      # (the key is the file's block)
    with open(hparams_file) as fin:
        settings = load_hyperpyyaml(fin, overrides)
    if flags.get("formant_norm") is not True and flags:
        raise SystemExit(f"--formant_norm {flags['formant_norm']}: this recipe normalises the formants; leave the flag "
                         "out")
    opts, pitch = formantnorm.check_recipe_options(settings, run_opts)
    os.makedirs(settings["output_folder"], exist_ok=True)
    print(gender.augment_notice("gender_classifier_train_formant_norm", settings))
    hparams = dict(settings, **gender.build(settings))
    hparams["formant_normalizer"] = formantnorm.FormantNormalizer(**opts)
    hparams["pitch_normalizer"] = None if pitch is None else pitchnorm.PitchNormalizer(**pitch)
    run_opts.setdefault("max_grad_norm", settings.get("max_grad_norm", 5.0))
    brain = gender.GenderFormantNormBrain(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams,
                                          run_opts=run_opts, checkpointer=hparams["checkpointer"])
    counter = hparams["epoch_counter"]
    train, valid, test = gender.loaders(hparams, synthetic, counter)
    brain.fit(counter, train, valid)
    brain.evaluate(test, min_key="error")
    summary = {"test_loss": brain.last_stats["loss"], "test_error": brain.last_stats["error"],
               "best_checkpoint": getattr(brain, "best_checkpoint", None), "formant_norm": True}
    summary.update({k: (list(v) if isinstance(v, tuple) else v) for k, v in opts.items()})
    summary["pitch_norm"] = pitch is not None
    if pitch is not None:
        summary.update(pitch_target_hz=pitch["target_hz"], psola=True)
    print(json.dumps(summary))


if __name__ == "__main__":
    main(sys.argv[1:])
