"""The eight gender-classifier scripts on gender.RECIPES and gender.run_recipe, and GenderBrain's one hook for waveform
transforms (no GPU).  What every script prints -- the augmentation notice, the JSON summary and its key order, the
refusals -- and the ``max_grad_norm`` its brain receives are held to tests/golden/gender_recipe_summaries.json, which
tools/recipe_summaries.py wrote at the commit before the scripts were put onto run_recipe; the hook is run on stub
modules."""
import importlib.util
import json
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("recipe_summaries", os.path.join(ROOT, "tools", "recipe_summaries.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


TOOL = _tool()
with open(os.path.join(ROOT, "tests", "golden", "gender_recipe_summaries.json")) as _f:
    GOLDEN = json.load(_f)
CASES = [(suffix, case) for suffix, cases in TOOL.CASES.items() for case in cases]


def test_the_golden_file_holds_exactly_the_tools_cases():
    assert len(CASES) >= 50
    assert list(GOLDEN) == ["gender_classifier_train" + suffix for suffix in TOOL.CASES]
    for suffix, cases in TOOL.CASES.items():
        assert list(GOLDEN["gender_classifier_train" + suffix]) == [TOOL.case_name(c) for c in cases], suffix


@pytest.mark.parametrize("suffix,case", CASES, ids=[f"train{s}: {TOOL.case_name(c)}" for s, c in CASES])
def test_script_prints_and_refuses_what_it_did_before(suffix, case):
    want = GOLDEN["gender_classifier_train" + suffix][TOOL.case_name(case)]
    # (the printed lines are compared as text: the order of the summary's keys is part of the record)
    assert json.loads(json.dumps(TOOL.run_case(suffix, case))) == want


def test_every_script_is_one_call_of_run_recipe_and_no_recipe_sets_the_old_hooks():
    from speech_anonymization_amd import gender
    assert list(gender.RECIPES) == ["gender_classifier_train" + s for s in
                                    ("", "_recon", "_pitch_norm", "_mcadams", "_formant_norm", "_resynth", "_modspec",
                                     "_tempo")]
    for name, row in gender.RECIPES.items():
        assert row.brain is (gender.GenderReconBrain if name.endswith("_recon") else gender.GenderBrain), name
        with open(os.path.join(ROOT, name + ".py")) as f:
            text = f.read()
        assert f'gender.run_recipe("{name}", argv)' in text and "def main(argv):" in text, name
    for gone in ("GenderPitchNormBrain", "GenderFormantNormBrain", "GenderTempoBrain"):
        assert not hasattr(gender, gone)
    assert issubclass(gender.GenderReconBrain, gender.GenderBrain)
    assert "compute_forward" not in vars(gender.GenderReconBrain)        # the hook is inherited, not restated


# ---- the hook, on stub modules ------------------------------------------------------------------------------------
class _Modules(dict):
    __getattr__ = dict.__getitem__


def _brain(monkeypatch, seen, transforms, cls=None, augmentation=False, **modules):
    """a GenderBrain (or ``cls``) on the CPU whose front end, normaliser, augmentation and classifier record into
    ``seen`` as (name, what they were given ...)"""
    from speech_anonymization_amd import gender

    def fbank(wavs):
        seen.append(("fbank", wavs))
        return wavs[:, :, None]

    def norm(feats, lens, epoch=0):
        seen.append(("norm", feats, lens))
        return feats

    def augment(wavs, lens, host_lens=None):
        seen.append(("augment", wavs, lens, host_lens))
        return wavs, lens, 1

    def log_probs(emb, cl, feats, lens):
        seen.append(("log_probs", feats, lens))
        return feats

    monkeypatch.setattr(gender.xvector, "train_log_probs", log_probs)
    b = object.__new__(cls or gender.GenderBrain)
    b.device = torch.device("cpu")
    b.modules = _Modules(compute_features=fbank, mean_var_norm=norm, embedding_model=None, classifier=None, **modules)
    if augmentation:
        b.modules["augmentation"] = augment
    b.hparams = types.SimpleNamespace(**({} if transforms is None else {"waveform_transforms": transforms}))
    return b


def _batch(wav, lens):
    from speech_anonymization_amd.brain import Batch
    return Batch(wav, lens, torch.zeros(wav.shape[0], dtype=torch.long))


def test_two_length_keeping_transforms_run_in_order_at_every_stage_before_augmentation(monkeypatch):
    from speech_anonymization_amd.brain import Stage
    seen = []

    def stub(name, add):
        def call(wavs, lens):
            seen.append((name, wavs, lens))
            return wavs + add
        return call

    b = _brain(monkeypatch, seen, [stub("first", 1.0), stub("second", 2.0)], augmentation=True)
    wav, lens = torch.zeros(2, 8), torch.tensor([1.0, 0.5])
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        del seen[:]
        b.compute_forward(_batch(wav, lens), stage)
        names = [s[0] for s in seen]
        assert names == ["first", "second"] + (["augment"] if stage == Stage.TRAIN else []) + ["fbank", "norm", "log_probs"]
        by = {s[0]: s for s in seen}
        # the batch's own tensors (a CPU batch's .to("cpu") hands the same objects on: the moved lengths are these)
        assert by["first"][1] is wav and by["first"][2] is lens
        assert torch.equal(by["second"][1], wav + 1.0) and by["second"][2] is lens
        assert torch.equal(by["fbank"][1], wav + 3.0)
        if stage == Stage.TRAIN:
            assert torch.equal(by["augment"][1], wav + 3.0) and by["augment"][2] is lens
            assert by["augment"][3] is lens                  # lengths kept: the loader's CPU lengths still hold
        assert by["norm"][2] is lens and by["log_probs"][2] is lens


def test_a_length_changing_transform_gets_the_loaders_lengths_and_hands_its_own_on(monkeypatch):
    from speech_anonymization_amd import timescale
    from speech_anonymization_amd.brain import Stage
    assert timescale.TimeScaler.host_lengths is True
    seen = []
    new_lens = torch.tensor([1.0, 0.25])

    class Scaler:
        host_lengths = timescale.TimeScaler.host_lengths     # marked the way TimeScaler is

        def __call__(self, wavs, lens):
            seen.append(("scaler", wavs, lens))
            return wavs[:, :4] + 1.0, new_lens

    def keeper(wavs, lens):
        seen.append(("keeper", wavs, lens))
        return wavs

    b = _brain(monkeypatch, seen, [Scaler(), keeper], augmentation=True)
    wav, lens = torch.zeros(2, 8), torch.tensor([1.0, 0.5])

    class MovedBatch:
        """a batch whose .to() makes new tensors, as a move to the device does"""
        sig, gender = (wav, lens), torch.zeros(2, dtype=torch.long)

        def to(self, device):
            return types.SimpleNamespace(sig=(wav.clone(), lens.clone()), gender=self.gender)

    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        del seen[:]
        b.compute_forward(MovedBatch(), stage)
        by = {s[0]: s for s in seen}
        assert by["scaler"][2] is lens                       # the loader's host lengths, by identity
        assert by["scaler"][1] is not wav and torch.equal(by["scaler"][1], wav)      # the moved waveforms
        assert by["keeper"][2] is new_lens and by["keeper"][1].shape == (2, 4)
        assert by["fbank"][1].shape == (2, 4) and torch.equal(by["fbank"][1], wav[:, :4] + 1.0)
        assert by["norm"][2] is new_lens and by["log_probs"][2] is new_lens
        assert b._host_lens is None
        if stage == Stage.TRAIN:
            assert by["augment"][2] is new_lens and by["augment"][3] is None
        else:
            assert "augment" not in by


@pytest.mark.parametrize("transforms", [None, [], ()])
def test_without_transforms_the_batchs_waveforms_reach_prepare_features_untouched(monkeypatch, transforms):
    from speech_anonymization_amd.brain import Stage
    seen = []
    b = _brain(monkeypatch, seen, transforms)
    given = []
    inner = type(b).prepare_features
    b.prepare_features = lambda wavs, lens, stage: given.append((wavs, lens)) or inner(b, wavs, lens, stage)
    wav, lens = torch.zeros(2, 8), torch.ones(2)
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        b.compute_forward(_batch(wav, lens), stage)
    assert len(given) == 3 and all(w is wav and l is lens for w, l in given)
    assert b._host_lens is lens


def test_recon_brain_runs_its_transform_before_the_reconstruction_sees_features(monkeypatch):
    from speech_anonymization_amd import gender
    from speech_anonymization_amd.brain import Stage
    seen = []

    class Model:
        def reconstruct(self, feats):
            seen.append(("reconstruct", feats))
            return 2.0 * feats

    def transform(wavs, lens):
        seen.append(("transform", wavs, lens))
        return wavs + 1.0

    b = _brain(monkeypatch, seen, [transform], cls=gender.GenderReconBrain, model=Model())
    wav, lens = torch.zeros(2, 8), torch.ones(2)
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        del seen[:]
        out = b.compute_forward(_batch(wav, lens), stage)
        assert [s[0] for s in seen] == ["transform", "fbank", "norm", "reconstruct", "log_probs"]
        assert seen[0][1] is wav and torch.equal(seen[1][1], wav + 1.0)
        assert torch.equal(seen[3][1], (wav + 1.0)[:, :, None]) and torch.equal(out, 2.0 * (wav + 1.0)[:, :, None])
