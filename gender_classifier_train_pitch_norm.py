#!/usr/bin/env python3
"""Trains the x-vector gender classifier on PITCH-NORMALISED waveforms (the reference's
gender_classifier_train_pitch_norm.py, its signal-processing baseline): every waveform, at train, valid and test
alike, has its voiced F0 scaled to a mean of ``pitch_target_hz`` before the classifier's front end sees it
(speech_anonymization_amd.pitchnorm).  Its test error answers "how much of sex does a classifier
still recover once the mean pitch is gone?" -- the number the learned anonymisers are compared against.

    python gender_classifier_train_pitch_norm.py speechbrain_configs/gender_classifier_pitch_norm.yaml \
        --device cuda:0 [--pitch_target_hz 170] [--preserve_formants true | --formant_ratio X] [--lifter 30] \
        [--phase griffin_lim|vocoder] [--contour_scale G [--contour_smooth S]] [--f0_method yin|viterbi] \
        [--psola true] [--synthetic N] [--key value ...]

``--preserve_formants true`` moves the pitch and leaves the spectral envelope where it was (what the reference's
WORLD re-synthesis does); ``--formant_ratio X`` scales it by X instead.  Without either the
formants move with the pitch.  ``--phase vocoder`` re-synthesises with the input's own phases carried through the
stretch instead of Griffin-Lim's reconstruction: one pass instead of 32 iterations.
``--contour_scale G`` (with ``--phase vocoder``) moves the F0 CONTOUR to target + G (f0 - mean) with a ratio per
frame: 1 is the reference's additive shift, 0 a monotone voice; ``--contour_smooth S`` is the
half-width in frames of the triangle the contour is smoothed with (default 2).  ``--f0_method viterbi`` forms the F0
track the ratios come from with a path decode through every frame's d' dips instead of first-dip
YIN.  ``--psola true`` (or ``psola: true`` in the YAML's ``pitch_norm:`` block) moves the pitch in the time domain
instead (TD-PSOLA): grains between pitch marks laid down again at the new spacing, which keeps the
envelope and the duration and needs no phase; it takes ``--contour_scale`` without ``--phase vocoder`` and none of
--phase, --preserve_formants true, --formant_ratio and --lifter.

Everything else is gender_classifier_train.py: manifests or ``--synthetic N``, the checkpoint layout, the JSON
summary as the last line (with pitch_target_hz added, and the envelope settings that were given)."""
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender


def main(argv):
    gender.run_recipe("gender_classifier_train_pitch_norm", argv)


if __name__ == "__main__":
    main(sys.argv[1:])
