"""The train step with the front end run once (run_opts front_end_once) and decoder.8's backward in one
launch (ConvAutoencoder.fused_bwd1c) against the step with both off = the launch sequence before either
existed: loss, loss terms, every parameter and the normaliser's state after three steps, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N = 2, 36 * 160 * 2 - 160             # T = 72 frames
SCALES = (1.0, 0.9, 0.8)


def _batches():
    from tests import smoke_step
    from speech_anonymization_amd.brain import Batch
    wav = smoke_step.make_wave(B, N)
    return [Batch(wav * s, torch.tensor([1.0, 0.83]), torch.arange(B) % 2) for s in SCALES]


def _run(on, graph=False, endtoend=False, by_hand=False, steps=None):
    from oracle.convae import numpy_params
    from tests import smoke_step
    dev = torch.device("cuda:0")
    torch.manual_seed(8886)
    br = smoke_step.build("bf16x3", dev, None if endtoend else numpy_params(8886),
                          run_opts={"front_end_once": on, "hip_graph": graph})
    if endtoend:
        from tests.test_endtoend_gpu import hip_classifier, oracle_classifier
        from speech_anonymization_amd.endtoend import ConvReconstruction
        br.modules["ConvAE"] = ConvReconstruction(hip_classifier(oracle_classifier())).to(dev)
        br.optimizer = None
        br.init_optimizers()
        hp = br.hparams
        hp.model_type, hp.recon_loss_weight, hp.sex_loss_weight, hp.confusion_loss_weight = "endtoend", 0.5, 0.4, 0.1
    model = br.modules["ConvAE"]
    model.fused_bwd1c = on
    assert br.front_end_once == on
    out = []
    batches = _batches()
    if steps:                            # hipGraph: warm-up steps, the capture and replays
        batches = [batches[i % len(batches)] for i in range(steps)]
    for batch in batches:
        br.step += 1
        loss = br.fit_batch(batch)
        out.append(dict(loss=loss.clone(), recon=br.last_losses["recon"].clone(), sex=br.last_losses["sex"].clone()))
        if by_hand:
            # a features() call outside fit_batch is never served the step's stored target: it runs the
            # front end (and moves the running statistics) like any call did before
            assert br.__dict__.get("_target_stash") is None
            wavs, lens = batch.to(dev).sig
            before = br.modules["normalize"].state.clone()
            f = br.features(wavs, lens)
            assert not torch.equal(br.modules["normalize"].state, before)
            out[-1]["by_hand"] = f.clone()
    torch.cuda.synchronize()
    if graph:
        assert any("graph" in e for e in br._graphs.values())
    return out, {k: v.detach().clone() for k, v in model.state_dict().items()}, br.modules["normalize"].state.clone()


def _same(a, b):
    (la, pa, sa), (lb, pb, sb) = a, b
    assert len(la) == len(lb)
    for i, (x, y) in enumerate(zip(la, lb)):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), (i, k, x[k], y[k])
    assert pa.keys() == pb.keys()
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert torch.equal(sa, sb)
    assert float(sa[0]) == 2 * len(la) + sum("by_hand" in x for x in la)


def test_three_steps_equal_with_both_knobs():
    _same(_run(False), _run(True))


def test_three_steps_equal_endtoend():
    _same(_run(False, endtoend=True), _run(True, endtoend=True))


def test_features_by_hand_between_steps_is_not_served_from_the_stash():
    _same(_run(False, by_hand=True), _run(True, by_hand=True))


def test_hip_graph_steps_equal():
    """GRAPH_WARMUP eager steps, the capture and two replays, knobs off against knobs on"""
    _same(_run(False, graph=True, steps=6), _run(True, graph=True, steps=6))
