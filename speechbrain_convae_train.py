#!/usr/bin/env python3
"""Entry point with the reference's command line (speechbrain_convae_train.py:1-8,514-615):

    python speechbrain_convae_train.py speechbrain_configs/convae.yaml \
        --device cuda:0 --model_type [convae / fcae / endtoend] --folder <output_dir> [--key value overrides]

    # data-parallel on one node (one process per GPU, RCCL):
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
        speechbrain_convae_train.py speechbrain_configs/convae.yaml --distributed_launch

Extra options of this build: ``--synthetic N`` trains on N synthetic utterances per epoch instead
of CSV manifests (there is no dataset on the GPU box).  ``--external_classifier_ckpt DIR`` (a
checkpoint of gender_classifier_train.py) adds the ACC_external / ACC_external_orig columns.
``--spec_augment true`` augments the model's input features at Stage.TRAIN (time warp, frequency and
time masks: the reference's ``augmentation``, settings under ``spec_augment_options``).  The
frozen-ASR utility loss and WER are not part of this path."""
import os
import sys

import torch

import speech_anonymization_amd as pkg
from speech_anonymization_amd import brain as B, convae, data, distributed as sdist
from speech_anonymization_amd.yaml_loader import load_hyperpyyaml, parse_arguments


MODEL_TYPES = ("convae", "fcae", "endtoend")


def check_model_type(model_type, run_opts, environ=None):
    """what can be refused before anything touches a GPU or a process group"""
    environ = os.environ if environ is None else environ
    if model_type not in MODEL_TYPES:
        raise SystemExit(f"unknown model_type {model_type!r}: this path implements convae, fcae and endtoend")
    if model_type == "fcae":
        if run_opts.get("distributed_launch") or int(environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("model_type fcae runs on one GPU: data parallelism is not implemented for it")
        if run_opts.get("hip_graph"):
            raise SystemExit("model_type fcae does not support --hip_graph (its step is nine launches)")


def setup_spec_augment(hparams):
    """--spec_augment true: SpecAugment of the input features at Stage.TRAIN (the reference's hparams.augmentation,
    :65-67), for every model type.  A specaug.SpecAugment the YAML built itself is kept; otherwise one is built
    from spec_augment_options.  Prints one line when it is on."""
    if not hparams.get("spec_augment"):
        return None
    from speech_anonymization_amd import specaug
    aug = hparams.get("augmentation")
    if not isinstance(aug, specaug.SpecAugment):
        aug = hparams["augmentation"] = specaug.SpecAugment(**dict(hparams.get("spec_augment_options") or {}))
    if sdist.if_main_process():
        print(f"speechbrain_convae_train: SpecAugment of the input features on: {aug.describe()}")
    return aug


def main(argv):
    hparams_file, run_opts, overrides = parse_arguments(argv)
    synthetic = overrides.pop("synthetic", None)
    n_samples = int(overrides.pop("synthetic_samples", 161120))
    with open(hparams_file) as fin:
        hparams = load_hyperpyyaml(fin, overrides)
    check_model_type(hparams["model_type"], run_opts)
    rank, local_rank, world = sdist.ddp_init_group(run_opts)
    run_opts.setdefault("device", f"cuda:{local_rank}")
    if sdist.if_main_process():
        os.makedirs(hparams["output_folder"], exist_ok=True)

    # a checkpoint directory of gender_classifier_train.py (embedding_model.ckpt / classifier.ckpt, strict
    # keys): the external classifier of ACC_external / ACC_external_orig in both model types (reference
    # :261-269) and the frozen in-graph classifier of model_type endtoend
    ck = hparams.get("external_classifier_ckpt")
    if ck:
        from speech_anonymization_amd.gender import load_external_classifier
        hparams["external_classifier"] = load_external_classifier(ck)
    if hparams["model_type"] == "convae":
        model = convae.ConvAutoencoder(precision=hparams.get("precision", "bf16x3"))
    elif hparams["model_type"] == "endtoend":              # reference :551-558 (EndToEnd.ConvReconstruction)
        from speech_anonymization_amd import endtoend, xvector
        clf = load_external_classifier(ck) if ck else xvector.EncoderClassifier()
        model = endtoend.ConvReconstruction(clf, precision=hparams.get("precision", "bf16x3"))
    else:                                                  # reference :556-558 (FullyConnected.FullyConnectedAutoencoder)
        from speech_anonymization_amd import fcae          # fp32 whatever `precision` says
        model = fcae.FullyConnectedAutoencoder(80, hparams["batch_size"])

    setup_spec_augment(hparams)
    sa_brain = B.SexAnonymizationTraining(modules=hparams["modules"], opt_class=hparams["Adam"],
                                          hparams=hparams, run_opts=run_opts,
                                          checkpointer=hparams.get("checkpointer"))
    model = model.to(sa_brain.device)
    sa_brain.modules["ConvAE"] = model
    hparams["model"].append(sa_brain.modules["ConvAE"])      # ModuleList index 0 (reference :580)
    if hparams.get("asr_utility"):
        # reference :560-574 attaches the pretrained recogniser as sa_brain.asr_brain; its weights
        # are a hub fetch, so here `--asr_utility random` builds the same architecture with random
        # frozen weights (throughput-only) and a path loads this module's own state_dict
        from speech_anonymization_amd import asr
        rec = asr.ASR(dtype=torch.bfloat16 if sa_brain.device.type == "cuda" else None)
        if hparams["asr_utility"] != "random":
            rec.load_state_dict(torch.load(hparams["asr_utility"], map_location="cpu", weights_only=True))
        sa_brain.asr_brain = rec.to(sa_brain.device)
        if not hasattr(sa_brain.hparams, "loss_utility"):
            from speech_anonymization_amd import losses
            sa_brain.hparams.loss_utility = losses.CosineSimilarityLoss()

    bs = hparams["batch_size"]
    if synthetic:
        train = lambda: data.synthetic_dataset(int(synthetic), bs, n_samples, rank=rank, world=world)
        valid = lambda: data.synthetic_dataset(bs * world, bs, n_samples, seed=1, rank=rank, world=world)
    else:
        rep = {"data_root": hparams["data_folder"]}
        tr = data.CsvDataset(hparams["train_csv"], rep, hparams.get("sorting", "random"))
        va = data.CsvDataset(hparams["valid_csv"], rep, "ascending")
        shuffle = hparams["train_dataloader_opts"].get("shuffle", False) and hparams.get("sorting") == "random"
        train = lambda epoch: data.batches(tr, bs, shuffle, hparams["seed"], rank, world, epoch)
        valid = lambda epoch: data.batches(va, bs, False, 0, rank, world)
    if synthetic:
        train_, valid_ = train, valid
        train, valid = (lambda epoch: train_()), (lambda epoch: valid_())

    class Loader:
        """re-iterable; the epoch number seeds the shuffle (seed + epoch).  It is the epoch counter's
        own number, so a resumed run continues with the shuffle orders of the epochs it has not
        seen yet instead of replaying those of epochs 1..k."""

        def __init__(self, f, counter):
            self.f, self.counter = f, counter

        def __iter__(self):
            return iter(self.f(max(1, int(self.counter.current))))

    counter = hparams["epoch_counter"]
    sa_brain.fit(counter, Loader(train, counter), Loader(valid, counter))
    # the library-owned communicator (SA_COMM=lib) and its side stream go before the process group
    # that carried its id, and before interpreter teardown
    sdist.lib_comm_destroy()
    if sdist.world_size() > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
