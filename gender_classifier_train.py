#!/usr/bin/env python3
"""Trains the external x-vector gender classifier (the reference's gender_classifier_train.py):

    python gender_classifier_train.py speechbrain_configs/gender_classifier.yaml \
        --device cuda:0 [--key value overrides]

It reads the CSV manifests named under ``manifests`` (column ``gender``: M / F) in ``data_folder``; ``--synthetic N`` trains on N generated utterances instead (two classes
separable by pitch, data.synthetic_gender_dataset; held-out validation and test sets of N/4 each).
The best checkpoint by validation error, under ``<save_folder>/CKPT+*``, is the directory
``speechbrain_convae_train.py --external_classifier_ckpt`` takes.  The last line printed is a JSON
summary (test loss and error, the checkpoint used)."""
import sys

import speech_anonymization_amd as pkg  # noqa: F401  (registers the package name)
from speech_anonymization_amd import gender


def main(argv):
    gender.run_recipe("gender_classifier_train", argv)


if __name__ == "__main__":
    main(sys.argv[1:])
