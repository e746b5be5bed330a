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
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender


def main(argv):
    gender.run_recipe("gender_classifier_train_mcadams", argv)


if __name__ == "__main__":
    main(sys.argv[1:])
