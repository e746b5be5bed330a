"""The external x-vector gender classifier's training recipe (the reference's
gender_classifier_train.py:58-216 and its config, restated; settings in this repository's
speechbrain_configs/gender_classifier.yaml, objects made by build()): Fbank ->
global InputNormalization -> Xvector -> Classifier, mean NLL loss, Adam, speechbrain's
ReduceLROnPlateau on the validation loss, and the checkpoint with the lowest classification
``error`` kept.  A checkpoint directory holds embedding_model.ckpt / classifier.ckpt (the key sets
of xvector.EncoderClassifier, strict), normalizer.ckpt, counter.ckpt, optimizer.ckpt, CKPT.yaml and
label_encoder.txt, so it is directly usable as ``speechbrain_convae_train.py
--external_classifier_ckpt DIR`` (the classifier of ACC_external in both model types, and the frozen
classifier of model_type endtoend).

Labels are data.SEX (M = 0, F = 1), the indices the ConvAE recipe compares ACC_external against.
The reference's CategoricalEncoder numbers the classes in order of first appearance instead, which
can swap them; the mapping used is written next to the weights (label_encoder.txt).

Waveform augmentation is opt-in (``augment: true``; augment.TrainAugment): white additive
noise rows in place of EnvCorrupt's OpenRIR noise, and TimeDomainSpecAugment, at Stage.TRAIN only.  Off -- the
default -- the recipe trains without it.

The second half of the module is the same recipe on RECONSTRUCTED features (the reference's
gender_classifier_train_recon.py; GenderReconBrain and the loading of the frozen anonymiser).  At its end stand
RECIPES, one row per gender_classifier_train*.py script, and run_recipe, the ``main`` of all of them: the recipes
on TRANSFORMED waveforms (pitch_norm, mcadams, formant_norm, resynth, modspec, tempo) are GenderBrain with their
transform in ``hparams.waveform_transforms``."""
import collections
import functools
import json
import os

import torch

from . import data, features, formantnorm, losses, mcadams, modspec, pitchnorm, sourcefilter, timescale, xvector
from .brain import Brain, EpochCounter, FileTrainLogger, Stage
from .checkpoint import Checkpointer
from .data import SEX
from .yaml_loader import load_hyperpyyaml, parse_arguments


class ReduceLROnPlateau:
    """speechbrain.nnet.schedulers.ReduceLROnPlateau (v0.5.x), restated -- parity unpinned.
    Until epoch ``dont_halve_until_epoch`` the rate is kept and the anchor follows the loss; after
    it, a loss at or below the anchor resets the patience counter and becomes the anchor, a worse
    loss uses up one unit of patience, and once patience is spent the rate is multiplied by
    ``factor`` and the counter reset.  The result is bounded below by ``lr_min``."""

    def __init__(self, lr_min=1e-8, factor=0.5, patience=2, dont_halve_until_epoch=65):
        self.lr_min, self.factor, self.patience = lr_min, factor, patience
        self.dont_halve_until_epoch = dont_halve_until_epoch
        self.patience_counter, self.losses, self.anchor = 0, [], 99999

    def __call__(self, optim_list, current_epoch, current_loss):
        for opt in optim_list:
            current_lr = opt.param_groups[0]["lr"]
            current_lr = float(current_lr) if torch.is_tensor(current_lr) else current_lr
            if current_epoch <= self.dont_halve_until_epoch:
                next_lr = current_lr
                self.anchor = current_loss
            elif current_loss <= self.anchor:
                self.patience_counter = 0
                next_lr = current_lr
                self.anchor = current_loss
            elif self.patience_counter < self.patience:
                self.patience_counter += 1
                next_lr = current_lr
            else:
                next_lr = current_lr * self.factor
                self.patience_counter = 0
            next_lr = max(next_lr, self.lr_min)
        self.losses.append(current_loss)
        return current_lr, next_lr

    def state_dict(self):
        return {"losses": list(self.losses), "anchor": self.anchor, "patience_counter": self.patience_counter}

    def load_state_dict(self, sd):
        self.losses, self.anchor = list(sd["losses"]), sd["anchor"]
        self.patience_counter = sd["patience_counter"]


def update_learning_rate(optimizer, new_lr):
    """speechbrain.nnet.schedulers.update_learning_rate"""
    for g in optimizer.param_groups:
        if torch.is_tensor(g["lr"]):
            g["lr"].fill_(new_lr)
        else:
            g["lr"] = new_lr


def write_label_encoder(path):
    """the class indices, in the text format of speechbrain's CategoricalEncoder.save"""
    with open(os.path.join(path, "label_encoder.txt"), "w") as f:
        for k, v in sorted(SEX.items(), key=lambda kv: kv[1]):
            f.write(f"'{k}' => {v}\n")
        f.write("================\n'starting_index' => 0\n")


def load_external_classifier(ckpt_dir, device=None):
    """xvector.EncoderClassifier from a checkpoint directory of this recipe (strict keys), eval mode"""
    clf = xvector.EncoderClassifier()
    clf.embedding_model.load_state_dict(torch.load(os.path.join(ckpt_dir, "embedding_model.ckpt"),
                                                   map_location="cpu", weights_only=True), strict=True)
    clf.classifier.load_state_dict(torch.load(os.path.join(ckpt_dir, "classifier.ckpt"), map_location="cpu",
                                              weights_only=True), strict=True)
    clf.eval()
    return clf.to(device) if device is not None else clf


def build(hp):
    """the recipe's objects from the plain settings of speechbrain_configs/gender_classifier.yaml
    (seeded first, so the initial weights follow ``seed``); returned as hparams entries."""
    torch.manual_seed(int(hp["seed"]))
    fb, xv, pl = hp["fbank"], hp["xvector"], hp["plateau"]
    emb = xvector.Xvector(in_channels=fb["n_mels"], lin_neurons=xv["embedding_dim"], tdnn_channels=xv["channels"],
                          tdnn_kernel_sizes=xv["kernel_sizes"], tdnn_dilations=xv["dilations"])
    cl = xvector.Classifier(input_shape=[None, None, xv["embedding_dim"]], lin_neurons=xv["embedding_dim"],
                            out_neurons=hp["classes"])
    norm = features.InputNormalization(norm_type="global")
    counter = EpochCounter(hp["number_of_epochs"])
    out = hp["output_folder"]
    modules = {"compute_features": features.Fbank(fb["sample_rate"], fb["n_fft"], fb["n_mels"]),
               "mean_var_norm": norm, "embedding_model": emb, "classifier": cl}
    if hp.get("augment"):
        from . import augment
        cfg = augment.settings(hp.get("augment_options"), sample_rate=fb["sample_rate"])
        augment.check_settings(cfg, hp["batch_size"])
        modules["augmentation"] = augment.TrainAugment(seed=int(hp["seed"]), **vars(cfg))
    return {
        "modules": modules,
        "epoch_counter": counter,
        "compute_cost": losses.NLLLoss(),
        "opt_class": functools.partial(torch.optim.Adam, lr=float(hp["adam_lr"])),
        "lr_annealing": ReduceLROnPlateau(factor=pl["factor"], patience=pl["patience"],
                                          dont_halve_until_epoch=pl["hold_until_epoch"]),
        "train_logger": FileTrainLogger(os.path.join(out, "train_log.txt")),
        "checkpointer": Checkpointer(os.path.join(out, "save"), {"embedding_model": emb, "classifier": cl,
                                                                 "normalizer": norm, "counter": counter}),
    }


class GenderBrain(Brain):
    """gender_classifier_train.py:58-216 on the Brain base (fused Adam, clipping at max_grad_norm,
    the lazy finite check, checkpoint resume).  ``hparams.waveform_transforms`` (absent: none) run on every batch at
    every stage, train, valid and test alike, before augmentation and features: what the reference's pitch-norm
    ``audio_pipeline`` does to every waveform it loads, and the hook of every waveform recipe in RECIPES."""

    def augment(self, wavs, lens, stage):
        """modules.augmentation (reference :79-86) at Stage.TRAIN: -> the augmented waveforms and their lengths.
        ``_aug`` keeps (lengths, repeat) of the batch in flight for compute_forward and compute_objectives."""
        self._aug = None
        if stage == Stage.TRAIN and "augmentation" in self.modules:
            wavs, lens, repeat = self.modules["augmentation"](wavs, lens, host_lens=self.__dict__.get("_host_lens"))
            self._aug = (lens, repeat)
        return wavs, lens

    def prepare_features(self, wavs, lens, stage):
        wavs, lens = self.augment(wavs, lens, stage)
        feats = self.modules.compute_features(wavs)
        # no epoch is passed (reference :104): the global statistics follow every training batch
        return self.modules.mean_var_norm(feats, lens)

    def transform_waveforms(self, wavs, lens, loader_lens):
        """``hparams.waveform_transforms`` in order, each called as t(wavs, lens) -> wavs (width and lengths kept) or
        (wavs, lens).  A transform marked ``host_lengths`` is given ``loader_lens``, the lengths as the loader made
        them, so that it knows its output's width without a device read; once a transform has returned lengths of
        its own, those are what every later step sees and ``_host_lens`` is None."""
        for t in getattr(self.hparams, "waveform_transforms", None) or ():
            out = t(wavs, loader_lens if loader_lens is not None and getattr(t, "host_lengths", False) else lens)
            if isinstance(out, tuple):
                wavs, lens = out
                loader_lens = self._host_lens = None
            else:
                wavs = out
        return wavs, lens

    def compute_forward(self, batch, stage):
        # the loader's CPU lengths: the augmentation draws its chunk positions from them without a device read
        loader_lens = batch.sig[1]
        self._host_lens = None if loader_lens.is_cuda else loader_lens
        batch = batch.to(self.device)
        wavs, lens = self.transform_waveforms(*batch.sig, loader_lens)
        feats = self.prepare_features(wavs, lens, stage)
        if self.__dict__.get("_aug"):
            lens = self._aug[0]
        return xvector.train_log_probs(self.modules.embedding_model, self.modules.classifier, feats, lens)

    def compute_objectives(self, predictions, batch, stage):
        label = batch.gender.to(self.device)
        if stage == Stage.TRAIN and self.__dict__.get("_aug") and self._aug[1] > 1:
            label = label.repeat(self._aug[1])              # clean rows, then their noisy copies
        logp = predictions.squeeze(1)
        loss = self.hparams.compute_cost(logp, label)
        if stage != Stage.TRAIN:
            self.n_err += int((logp.argmax(dim=-1) != label).sum())
            self.n_utt += int(label.numel())
        return loss

    def on_stage_start(self, stage, epoch=None):
        self.n_err, self.n_utt = 0, 0
        if stage == Stage.TRAIN and "augmentation" in self.modules:
            self.modules["augmentation"].reseed(epoch)       # (seed, epoch): the same draws after a resume

    def on_stage_end(self, stage, stage_loss, epoch=None):
        if stage == Stage.TRAIN:
            self.train_loss = stage_loss
            return
        stats = {"loss": stage_loss, "error": self.n_err / max(1, self.n_utt)}
        self.last_stats = stats
        logger = getattr(self.hparams, "train_logger", None)
        if stage == Stage.VALID:
            old_lr, new_lr = self.hparams.lr_annealing([self.optimizer], epoch, stage_loss)
            update_learning_rate(self.optimizer, new_lr)
            if logger is not None:
                logger.log_stats({"Epoch": epoch, "lr": old_lr}, train_stats={"loss": self.train_loss},
                                 valid_stats=stats)
            if self.checkpointer is not None:
                path = self.checkpointer.save_and_keep_only(meta=stats, min_keys=["error"])
                write_label_encoder(path)
        elif logger is not None:
            logger.log_stats({"Epoch loaded": self.hparams.epoch_counter.current}, test_stats=stats)

    def on_evaluate_start(self, max_key=None, min_key=None):
        """speechbrain's evaluate(): the model of the best checkpoint by max_key / min_key"""
        if self.checkpointer is None:
            return
        ckpts = self.checkpointer.find_checkpoints(max_key=max_key, min_key=min_key)
        if not ckpts:
            return
        self.best_checkpoint = ckpts[0]
        for name in ("embedding_model", "classifier", "mean_var_norm"):
            fn = os.path.join(ckpts[0], ("normalizer" if name == "mean_var_norm" else name) + ".ckpt")
            sd = torch.load(fn, map_location="cpu", weights_only=True)
            self.modules[name].load_state_dict(sd)


def augment_notice(script, settings):
    """the one line either script prints about waveform augmentation"""
    if not settings.get("augment"):
        return (f"{script}: waveform augmentation (EnvCorrupt, TimeDomainSpecAugment) is not part of "
                "this build; training without it")
    from . import augment
    c = augment.settings(settings.get("augment_options"))
    noise = (f"additive white noise at {c.snr_low:g}-{c.snr_high:g} dB SNR doubling the batch (OpenRIR noise and "
             "reverberation are not built)") if c.noise else "no noise rows"
    return (f"{script}: waveform augmentation on: speeds {list(c.speeds)}, frequency drop "
            f"{c.drop_freq_count_low}-{c.drop_freq_count_high} notches, chunk drop {c.drop_chunk_count_low}-"
            f"{c.drop_chunk_count_high} x {c.drop_chunk_length_low}-{c.drop_chunk_length_high} samples, {noise}")


class _EpochLoader:
    """an iterable that asks ``batches(epoch)`` anew on every pass, with the epoch the counter is in (1 before the
    first)"""

    def __init__(self, batches, counter):
        self.batches, self.counter = batches, counter

    def __iter__(self):
        return iter(self.batches(max(1, int(self.counter.current))))


def loaders(hparams, synthetic, counter):
    """what the four gender recipes train on -> (train loader, valid loader, test iterable): ``synthetic`` utterances of
    data.synthetic_gender_dataset (a fresh draw per training epoch, a quarter as many held out), or the manifests"""
    bs, seed = int(hparams["batch_size"]), int(hparams["seed"])
    if synthetic:
        n = int(synthetic)
        held = max(bs, n // 4)
        make = lambda k, s, ep=0: data.synthetic_gender_dataset(k, bs, seed=s + ep)
        train = lambda epoch: make(n, seed, 1000 * epoch)
        valid = lambda epoch: make(held, seed + 1)
        test = make(held, seed + 2)
    else:
        rep = {"data_root": hparams["data_folder"]}
        csv = {k: os.path.join(hparams["data_folder"], v) for k, v in hparams["manifests"].items()}
        tr = data.CsvDataset(csv["train"], rep)
        va = data.CsvDataset(csv["valid"], rep, "ascending")
        train = lambda epoch: data.batches(tr, bs, bool(hparams.get("shuffle", True)), seed, epoch=epoch)
        valid = lambda epoch: data.batches(va, bs)
        test = data.batches(data.CsvDataset(csv["test"], rep, "ascending"), bs)
    return _EpochLoader(train, counter), _EpochLoader(valid, counter), test


# ---------------------------------------------------------------------------------------------------
# the same recipe on reconstructed features (the reference's gender_classifier_train_recon.py)
# ---------------------------------------------------------------------------------------------------
RECON_MODEL_TYPES = ("convae", "fcae", "endtoend")
RECON_NORMALIZERS = ("own", "checkpoint")


def check_recon_options(settings, run_opts, environ=None):
    """what gender_classifier_train_recon.py refuses before anything touches a GPU, one line each"""
    mt = settings.get("model_type")
    if mt not in RECON_MODEL_TYPES:
        raise SystemExit(f"unknown model_type {mt!r}: the anonymiser is one of convae, fcae and endtoend")
    if not settings.get("recon_ckpt"):
        raise SystemExit("--recon_ckpt DIR is required: a CKPT+* directory of speechbrain_convae_train.py "
                         "(model.ckpt, normalizer.ckpt)")
    if settings.get("recon_normalizer", "own") not in RECON_NORMALIZERS:
        raise SystemExit(f"unknown recon_normalizer {settings.get('recon_normalizer')!r}: own or checkpoint")
    pitchnorm.refuse_run_modes("gender_classifier_train_recon", settings, run_opts, environ)


def build_anonymiser(model_type, precision="bf16x3", external_classifier=None, batch_size=None):
    """the model class ``model_type`` names, as speechbrain_convae_train.py constructs it (on the CPU)"""
    if model_type == "convae":
        from .convae import ConvAutoencoder
        return ConvAutoencoder(precision=precision)
    if model_type == "endtoend":
        from .endtoend import ConvReconstruction
        return ConvReconstruction(external_classifier, precision=precision)
    if model_type == "fcae":
        from .fcae import FullyConnectedAutoencoder
        return FullyConnectedAutoencoder(80, batch_size)
    raise SystemExit(f"unknown model_type {model_type!r}: the anonymiser is one of convae, fcae and endtoend")


def load_anonymiser(model, ckpt_dir):
    """``model.ckpt`` of a CKPT+* directory of speechbrain_convae_train.py holds the state dict of the
    recipe's torch.nn.ModuleList (keys prefixed ``0.``): into ``model``, strict.  A key mismatch (a checkpoint
    of another model_type) exits in one line naming the first missing key.  -> model, frozen, eval mode"""
    fn = os.path.join(ckpt_dir, "model.ckpt")
    if not os.path.isfile(fn):
        raise SystemExit(f"--recon_ckpt {ckpt_dir}: no model.ckpt there")
    sd = torch.load(fn, map_location="cpu", weights_only=True)
    sd = {k[2:]: v for k, v in sd.items() if k.startswith("0.")}
    want = model.state_dict()
    if isinstance(getattr(model, "sex_classifier", None), xvector.EncoderClassifier):
        # endtoend: the frozen in-graph x-vector comes from --external_classifier_ckpt where the checkpoint
        # does not carry it; reconstruct never runs it
        for k, v in want.items():
            if k.startswith("sex_classifier."):
                sd.setdefault(k, v)
    missing = [k for k in want if k not in sd]
    if missing:
        raise SystemExit(f"--recon_ckpt {ckpt_dir}: model.ckpt does not hold a {type(model).__name__}: "
                         f"missing key {missing[0]!r} ({len(missing)} of {len(want)} keys missing; wrong --model_type?)")
    unexpected = [k for k in sd if k not in want]
    if unexpected:
        raise SystemExit(f"--recon_ckpt {ckpt_dir}: model.ckpt does not hold a {type(model).__name__}: "
                         f"unexpected key {unexpected[0]!r} (wrong --model_type?)")
    try:
        model.load_state_dict(sd, strict=True)
    except RuntimeError as e:                             # same keys, other shapes
        raise SystemExit(f"--recon_ckpt {ckpt_dir}: model.ckpt does not fit a {type(model).__name__}: "
                         + " ".join(str(e).split())[:200])
    for p in model.parameters():
        p.requires_grad = False
    return model.eval()


def load_recon_normalizer(ckpt_dir):
    """the anonymiser's own global InputNormalization (normalizer.ckpt of its checkpoint), frozen"""
    fn = os.path.join(ckpt_dir, "normalizer.ckpt")
    if not os.path.isfile(fn):
        raise SystemExit(f"recon_normalizer checkpoint: no normalizer.ckpt in {ckpt_dir}")
    norm = features.InputNormalization(norm_type="global", update_until_epoch=0)
    norm.load_state_dict(torch.load(fn, map_location="cpu", weights_only=True))
    return norm.eval()                                     # eval mode and not among Brain.modules: never updated


class GenderReconBrain(GenderBrain):
    """gender_classifier_train_recon.py:58-93: the x-vector classifier trained on what a frozen anonymiser
    makes of the features.  ``modules.model`` is the anonymiser (anything with ``reconstruct``); Brain.fit puts
    it in train mode with the other modules, as the reference's does, and reconstruct does not care.
    hparams.recon_normalizer: "own" -- the recipe's mean_var_norm feeds the anonymiser (what the reference
    runs); "checkpoint" -- the anonymiser's own frozen normaliser ``hparams.recon_norm`` does, while
    mean_var_norm still follows every training batch (it is saved with the classifier) unapplied.
    prepare_features is the recipe's only change; init_optimizers keeps the anonymiser's (frozen) parameters
    out of the optimiser's list, and the checkpointer never had them."""

    def prepare_features(self, wavs, lens, stage):
        wavs, lens = self.augment(wavs, lens, stage)
        feats = self.modules.compute_features(wavs)
        # no epoch is passed (reference :85): the global statistics follow every training batch
        normed = self.modules.mean_var_norm(feats, lens)
        if getattr(self.hparams, "recon_normalizer", "own") == "checkpoint":
            normed = self.hparams.recon_norm(feats, lens, epoch=1)
        return self.modules.model.reconstruct(normed)

    def init_optimizers(self):
        model = self.modules.pop("model")
        try:
            super().init_optimizers()
        finally:
            self.modules["model"] = model


# ---------------------------------------------------------------------------------------------------
# the eight recipes: one row each, one driver
# ---------------------------------------------------------------------------------------------------
def formant_transforms(checked):
    opts, pitch = checked
    return [formantnorm.FormantNormalizer(**opts)] + ([] if pitch is None else [pitchnorm.PitchNormalizer(**pitch)])


def formant_summary(settings, checked):
    opts, pitch = checked
    extra = dict({"formant_norm": True}, **_listed(opts), pitch_norm=pitch is not None)
    if pitch is not None:
        extra.update(pitch_target_hz=pitch["target_hz"], psola=True)
    return extra


def recon_setup(settings):
    """loads the frozen anonymiser before build() seeds and makes the classifier, as the script always has -> what
    puts it, and the checkpoint's normaliser where that is asked for, into the built hparams"""
    ext = None
    if settings["model_type"] == "endtoend" and settings.get("external_classifier_ckpt"):
        ext = load_external_classifier(settings["external_classifier_ckpt"])
    model = load_anonymiser(build_anonymiser(settings["model_type"], settings.get("precision", "bf16x3"), ext,
                                             int(settings["batch_size"])), settings["recon_ckpt"])

    def finish(hparams):
        if settings.get("recon_normalizer", "own") == "checkpoint":
            hparams["recon_norm"] = load_recon_normalizer(settings["recon_ckpt"])
        hparams["modules"]["model"] = model                # frozen: not a recoverable, not in the optimiser
    return finish


def _listed(opts):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in opts.items()}


PITCH_SUMMARY_KEYS = ("preserve_formants", "formant_ratio", "lifter", "phase", "contour_scale", "contour_smooth",
                      "f0_method", "psola")
# check(settings, run_opts[, environ]) -> checked: the script's refusals; transforms(checked) -> the list for
# hparams.waveform_transforms; summary(settings, checked) -> what the script adds to the JSON summary, in order;
# setup(settings): see recon_setup; own_flag: (key, why) of a flag that names the recipe itself and may only say true
# -- it is taken off the command line before the file is read, where the key is a block
Recipe = collections.namedtuple("Recipe", "check transforms summary brain setup own_flag",
                                defaults=(None, None, lambda settings, checked: {}, GenderBrain, None, None))
RECIPES = {
    "gender_classifier_train": Recipe(),
    "gender_classifier_train_recon": Recipe(
        check_recon_options, brain=GenderReconBrain, setup=recon_setup,
        summary=lambda st, _: {"recon_ckpt": st["recon_ckpt"], "model_type": st["model_type"]}),
    "gender_classifier_train_pitch_norm": Recipe(
        pitchnorm.check_pitch_options, lambda pn: [pitchnorm.PitchNormalizer(**pn)],
        lambda st, pn: dict({"pitch_target_hz": pn["target_hz"]}, **{k: pn[k] for k in PITCH_SUMMARY_KEYS if k in pn})),
    "gender_classifier_train_mcadams": Recipe(
        mcadams.check_recipe_options, lambda opts: [mcadams.McAdams(**opts)],
        lambda st, opts: dict({"mcadams": True}, **_listed(opts))),
    "gender_classifier_train_formant_norm": Recipe(
        formantnorm.check_recipe_options, formant_transforms, formant_summary,
        own_flag=("formant_norm", "this recipe normalises the formants; leave the flag out")),
    "gender_classifier_train_resynth": Recipe(
        sourcefilter.check_recipe_options, lambda opts: [sourcefilter.SourceFilter(**opts)],
        lambda st, opts: dict({"resynth": True}, **opts)),
    "gender_classifier_train_modspec": Recipe(
        modspec.check_recipe_options, lambda opts: [modspec.ModulationSmoother(**opts)],
        lambda st, opts: dict({"modspec": True}, **opts)),
    "gender_classifier_train_tempo": Recipe(
        timescale.check_recipe_options, lambda opts: [timescale.TimeScaler(**opts)],
        lambda st, opts: dict({"tempo_mode": True}, **_listed(opts))),
}


def recipe_brain(row, settings, run_opts, checked, checkpointer=True):
    """the brain of a RECIPES row on loaded ``settings`` and what its checker returned -> (brain, its hparams)"""
    finish = row.setup(settings) if row.setup else None
    hparams = dict(settings, **build(settings))
    if row.transforms:
        hparams["waveform_transforms"] = row.transforms(checked)
    if finish:
        finish(hparams)
    brain = row.brain(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams, run_opts=run_opts,
                      checkpointer=hparams["checkpointer"] if checkpointer else None)
    return brain, hparams


def run_recipe(name, argv):
    """``main(argv)`` of the script ``name``: parse, load the YAML, refuse, say what the augmentation does, build,
    train, evaluate the best checkpoint, and print the JSON summary as the last line"""
    row = RECIPES[name]
    hparams_file, run_opts, overrides = parse_arguments(argv)
    synthetic = overrides.pop("synthetic", None)
    flag = overrides.pop(row.own_flag[0], True) if row.own_flag else True
    with open(hparams_file) as fin:
        settings = load_hyperpyyaml(fin, overrides)
    if flag is not True:
        raise SystemExit(f"--{row.own_flag[0]} {flag}: {row.own_flag[1]}")
    checked = row.check(settings, run_opts) if row.check else None
    os.makedirs(settings["output_folder"], exist_ok=True)
    print(augment_notice(name, settings))
    run_opts.setdefault("max_grad_norm", settings.get("max_grad_norm", 5.0))
    brain, hparams = recipe_brain(row, settings, run_opts, checked)
    counter = hparams["epoch_counter"]
    train, valid, test = loaders(hparams, synthetic, counter)
    brain.fit(counter, train, valid)
    brain.evaluate(test, min_key="error")
    summary = {"test_loss": brain.last_stats["loss"], "test_error": brain.last_stats["error"],
               "best_checkpoint": getattr(brain, "best_checkpoint", None)}
    summary.update(row.summary(settings, checked))
    print(json.dumps(summary))
