"""InputNormalization.forward_pair (sa_fbank_normalize_pair) against two successive forward calls from a
cloned state: both outputs and the state, bit for bit."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

BATCH, N = 3, 5000                       # T = 1 + 5000 // 160 = 32 frames, padded to 36
LENS = [1.0, 0.7, 0.31]
UNTIL = 4


def _features(kind, top_db_mode):
    """the normaliser's input: Fbank's raw features with their tile maxima, or a plain [B, T, 80] tensor"""
    import speech_anonymization_amd as pkg
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5000)
    t = torch.arange(N) / 16000.0
    wav = 0.1 * torch.randn(BATCH, N, generator=g) + 0.3 * torch.sin(2 * torch.pi * 440.0 * t)[None, :]
    wav = (wav * torch.tensor([1.0, 0.5, 0.05])[:, None]).to(dev)
    feats = pkg.Fbank(16000, 400, 80, top_db_mode=top_db_mode).to(dev)(wav)
    assert feats.shape == (BATCH, 32, 80)
    return feats if kind == "fbank" else feats.clamped().clone()


def _normaliser(state):
    import speech_anonymization_amd as pkg
    dev = torch.device("cuda:0")
    nrm = pkg.InputNormalization("global", update_until_epoch=UNTIL).to(dev)
    if state != "fresh":                 # a state an earlier epoch left: count > 0
        g = torch.Generator().manual_seed(3)
        nrm.load_state_dict(dict(count=5, glob_mean=-30.0 + torch.randn(80, generator=g),
                                 glob_std=8.0 + torch.rand(80, generator=g)))
    nrm.train(state != "eval")
    return nrm


# state, epoch, count after the pair
STATES = [("fresh", 1, 2), ("running", 1, 7), ("frozen", UNTIL, 7), ("eval", 1, 5)]


@pytest.mark.parametrize("kind,top_db_mode", [("fbank", "utterance"), ("fbank", "batch"), ("tensor", "utterance")],
                         ids=["fbank", "fbank-batchmax", "tensor"])
@pytest.mark.parametrize("state,epoch,count", STATES, ids=[s[0] for s in STATES])
def test_forward_pair_equals_two_forwards(state, epoch, count, kind, top_db_mode):
    feats = _features(kind, top_db_mode)
    lens = torch.tensor(LENS)
    a = _normaliser(state)
    b = copy.deepcopy(a)
    assert torch.equal(a.state, b.state)
    r1 = a(feats, lens, epoch=epoch, pad_multiple=36)
    r2 = a(feats, lens, epoch=epoch, pad_multiple=36)
    o1, o2 = b.forward_pair(feats, lens, epoch=epoch, pad_multiple=36)
    torch.cuda.synchronize()
    assert o1.shape == (BATCH, 36, 80) and o2.shape == o1.shape
    assert torch.equal(o1, r1)
    assert torch.equal(o2, r2)
    assert torch.equal(a.state, b.state)
    assert b.count == count
    assert float(o1[:, 32:].abs().max()) == 0.0 and float(o2[:, 32:].abs().max()) == 0.0
    if state == "running":
        assert not torch.equal(r1, r2)                    # the second call did see other statistics
    if state in ("frozen", "eval"):
        assert torch.equal(r1, r2) and o1 is o2           # one tensor where the statistics cannot move


def test_frozen_epoch_with_unknown_count_writes_both():
    """epoch >= update_until_epoch on a state written behind the module's back (the host does not know
    count > 0; here it is 0, so the first update DOES set the statistics): two tensors, still the bits"""
    feats = _features("fbank", "utterance")
    lens = torch.tensor(LENS)
    a = _normaliser("fresh")
    b = copy.deepcopy(a)
    r1 = a(feats, lens, epoch=UNTIL, pad_multiple=36)
    r2 = a(feats, lens, epoch=UNTIL, pad_multiple=36)
    o1, o2 = b.forward_pair(feats, lens, epoch=UNTIL, pad_multiple=36)
    torch.cuda.synchronize()
    assert o1 is not o2
    assert torch.equal(o1, r1) and torch.equal(o2, r2) and torch.equal(a.state, b.state)
    assert b.count == 2
