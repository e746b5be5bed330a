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
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender


def main(argv):
    gender.run_recipe("gender_classifier_train_modspec", argv)


if __name__ == "__main__":
    main(sys.argv[1:])
