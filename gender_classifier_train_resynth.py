#!/usr/bin/env python3
"""Trains the x-vector gender classifier on SOURCE-FILTER RESYNTHESISED waveforms: the informed attacker of the
classic LPC vocoder.  Every waveform, at train, valid and test alike, keeps each frame's LPC envelope and energy and
has its excitation replaced by pulses at the F0 track and noise (speech_anonymization_amd.sourcefilter; DESIGN
section 27) before the classifier's front end sees it.  Its test error answers "how much of sex does a classifier
still recover once the speaker's own excitation -- jitter, shimmer, breathiness, the glottal pulse shape -- is gone
(and, with a pitch target, the pitch as well)?".

    python gender_classifier_train_resynth.py speechbrain_configs/gender_classifier_resynth.yaml \
        --device cuda:0 [--resynth_pitch_hz X] [--aspiration A] [--f0_method yin|viterbi] [--synthetic N]
        [--key value ...]

``--resynth_pitch_hz X`` lays the pulses down so that every utterance's mean voiced F0 becomes X; without it (and
without ``pitch_target_hz`` in the ``resynth_options`` block) every utterance keeps its own pitch.  The noise seeds
are deterministic in the block's seed and the batch count.  One GPU, no --hip_graph.

Everything else is gender_classifier_train.py: manifests or ``--synthetic N``, the checkpoint layout, the JSON
summary as the last line (with the resynthesis settings added)."""
import json
import os
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender, sourcefilter
from speech_anonymization_amd.yaml_loader import load_hyperpyyaml, parse_arguments


def main(argv):
    hparams_file, run_opts, overrides = parse_arguments(argv)
    synthetic = overrides.pop("synthetic", None)
    with open(hparams_file) as fin:
        settings = load_hyperpyyaml(fin, overrides)
    opts = sourcefilter.check_recipe_options(settings, run_opts)
    os.makedirs(settings["output_folder"], exist_ok=True)
    print(gender.augment_notice("gender_classifier_train_resynth", settings))
    hparams = dict(settings, **gender.build(settings))
    hparams["pitch_normalizer"] = sourcefilter.SourceFilter(**opts)   # (the brain's hook for a waveform transform)
    run_opts.setdefault("max_grad_norm", settings.get("max_grad_norm", 5.0))
    brain = gender.GenderPitchNormBrain(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams,
                                        run_opts=run_opts, checkpointer=hparams["checkpointer"])
    counter = hparams["epoch_counter"]
    train, valid, test = gender.loaders(hparams, synthetic, counter)
    brain.fit(counter, train, valid)
    brain.evaluate(test, min_key="error")
    summary = {"test_loss": brain.last_stats["loss"], "test_error": brain.last_stats["error"],
               "best_checkpoint": getattr(brain, "best_checkpoint", None), "resynth": True}
    summary.update(opts)
    print(json.dumps(summary))


if __name__ == "__main__":
    main(sys.argv[1:])
