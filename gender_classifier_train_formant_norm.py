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
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender


def main(argv):
    gender.run_recipe("gender_classifier_train_formant_norm", argv)


if __name__ == "__main__":
    main(sys.argv[1:])
