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
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender


def main(argv):
    gender.run_recipe("gender_classifier_train_tempo", argv)


if __name__ == "__main__":
    main(sys.argv[1:])
