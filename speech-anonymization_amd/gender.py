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
gender_classifier_train_recon.py; GenderReconBrain and the loading of the frozen anonymiser), and at its end the
recipe on PITCH-NORMALISED waveforms (gender_classifier_train_pitch_norm.py; GenderPitchNormBrain)."""
import functools
import os

import torch

from . import data, features, losses, xvector
from .brain import Brain, EpochCounter, FileTrainLogger, Stage
from .checkpoint import Checkpointer
from .data import SEX


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
    the lazy finite check, checkpoint resume)."""

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

    def compute_forward(self, batch, stage):
        # the loader's CPU lengths: the augmentation draws its chunk positions from them without a device read
        self._host_lens = None if batch.sig[1].is_cuda else batch.sig[1]
        batch = batch.to(self.device)
        wavs, lens = batch.sig
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
    environ = os.environ if environ is None else environ
    mt = settings.get("model_type")
    if mt not in RECON_MODEL_TYPES:
        raise SystemExit(f"unknown model_type {mt!r}: the anonymiser is one of convae, fcae and endtoend")
    if not settings.get("recon_ckpt"):
        raise SystemExit("--recon_ckpt DIR is required: a CKPT+* directory of speechbrain_convae_train.py "
                         "(model.ckpt, normalizer.ckpt)")
    if settings.get("recon_normalizer", "own") not in RECON_NORMALIZERS:
        raise SystemExit(f"unknown recon_normalizer {settings.get('recon_normalizer')!r}: own or checkpoint")
    if run_opts.get("distributed_launch") or int(environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("gender_classifier_train_recon runs on one GPU: data parallelism is not implemented for it")
    if run_opts.get("hip_graph") or settings.get("hip_graph"):   # (from the command line it arrives as a setting)
        raise SystemExit("gender_classifier_train_recon does not support --hip_graph")


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
# the same recipe on pitch-normalised waveforms (the reference's gender_classifier_train_pitch_norm.py)
# ---------------------------------------------------------------------------------------------------
class GenderPitchNormBrain(GenderBrain):
    """gender_classifier_train_pitch_norm.py: the reference's ``audio_pipeline`` pitch-normalises every waveform
    it loads, for train, valid and test alike, so ``hparams.pitch_normalizer`` (pitchnorm.PitchNormalizer; DESIGN
    section 15) runs at every stage, before augmentation and features.  Shapes and lengths are kept, so the rest
    of the recipe is GenderBrain's."""

    def prepare_features(self, wavs, lens, stage):
        return super().prepare_features(self.hparams.pitch_normalizer(wavs, lens), lens, stage)


class GenderFormantNormBrain(GenderBrain):
    """gender_classifier_train_formant_norm.py: ``hparams.formant_normalizer`` (formantnorm.FormantNormalizer; DESIGN
    section 26) brings every waveform's formants to the target at every stage, train, valid and test alike, before
    augmentation and features; with ``hparams.pitch_normalizer`` (a PitchNormalizer with psola=True, or None) the
    pitch of the result is normalised too.  Shapes and lengths are kept, so the rest of the recipe is GenderBrain's."""

    def prepare_features(self, wavs, lens, stage):
        wavs = self.hparams.formant_normalizer(wavs, lens)
        pn = getattr(self.hparams, "pitch_normalizer", None)
        if pn is not None:
            wavs = pn(wavs, lens)
        return super().prepare_features(wavs, lens, stage)


class GenderTempoBrain(GenderBrain):
    """gender_classifier_train_tempo.py: ``hparams.time_scaler`` (timescale.TimeScaler) plays every
    waveform at another tempo at every stage, train, valid and test alike, before augmentation and features.  The
    batch's width and its relative lengths change, so the scaler's own lengths go on to the normaliser and the
    pooling.  It is given the loader's CPU lengths: the output's width is then known without a device read."""

    def compute_forward(self, batch, stage):
        host_lens = batch.sig[1]
        batch = batch.to(self.device)
        wavs, lens = self.hparams.time_scaler(batch.sig[0], host_lens)
        self._host_lens = None                               # (the lengths changed: the augmentation reads the device's)
        feats = self.prepare_features(wavs, lens, stage)
        if self.__dict__.get("_aug"):
            lens = self._aug[0]
        return xvector.train_log_probs(self.modules.embedding_model, self.modules.classifier, feats, lens)
