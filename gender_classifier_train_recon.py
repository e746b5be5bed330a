#!/usr/bin/env python3
"""Trains the x-vector gender classifier on RECONSTRUCTED features (the reference's
gender_classifier_train_recon.py): a trained anonymiser runs in inference on every batch and the classifier
of gender_classifier_train.py learns from its output.  Its test error answers "how well does an attacker who
knows the anonymiser recover sex from what it emits?".

    python gender_classifier_train_recon.py speechbrain_configs/gender_classifier_recon.yaml \
        --device cuda:0 --recon_ckpt DIR --model_type fcae|convae|endtoend [--synthetic N] [--key value ...]

DIR is a CKPT+* directory written by speechbrain_convae_train.py (model.ckpt with the ModuleList's ``0.``
keys, normalizer.ckpt).  ``--recon_normalizer checkpoint`` puts the anonymiser's own normaliser in front of
it instead of the recipe's fresh one.  model_type endtoend also takes
``--external_classifier_ckpt DIR`` for its frozen in-graph classifier, which this recipe never runs.
Everything else is gender_classifier_train.py: manifests or ``--synthetic N``, the checkpoint layout, the JSON
summary as the last line (with recon_ckpt and model_type added)."""
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender


def main(argv):
    gender.run_recipe("gender_classifier_train_recon", argv)


if __name__ == "__main__":
    main(sys.argv[1:])
