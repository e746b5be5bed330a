"""SpecAugment of the input features on the GPU (csrc/sa_specaug.hip, specaug.py) against the fp64
restatement tests/specaug_ref.py of the plan's own fp32 tables.  Bars, per element (specaug_ref.check_output):

    warp        |y - y64| <= 8 * 2^-24 * sum_k |w[o][k]| * max |x_b|; rows with weights (0, 1, 0, 0) are ==
    fill values all frequency-filled cells bit-equal to one value, all time-filled cells to one value, each within
                the largest warp bar + 2^-23 |ref| of the fp64 mean; == 0 with replace_with_zero

Every figure is printed before it is asserted."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import specaug_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F = 80
REFERENCE = dict(freq_mask_width=30, time_mask_width=40, replace_with_zero=False)     # reference convae.yaml:273-283


def _x(B, T, seed, F=F):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, F, generator=g) * torch.linspace(0.5, 3.0, B).view(B, 1, 1) + 0.7


def _run(x, plan):
    from speech_anonymization_amd import specaug
    xd = x.to(DEV)
    keep = xd.clone()
    out = specaug.apply_plan(xd, plan)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "the input was written"
    assert out.data_ptr() != xd.data_ptr()
    return out


# ---------------------------------------------------------------------------------------------------
# the warp
# ---------------------------------------------------------------------------------------------------
def _warp_cases():
    cases = []
    for T in (72, 36, 33):                 # 72: three tiles, the last partial; 33: one frame in the second tile
        cases += [(3, T, 5, 1), (3, T, 5, 10), (3, T, T - 6, T - 1), (3, T, T // 2, T // 2), (3, T, T // 2, T // 2 - 3)]
    return cases + [(3, 7, None, None), (3, 10, None, None), (2, 1008, 504, 500)]


@pytest.mark.parametrize("B,T,c,w", _warp_cases())
def test_warp(B, T, c, w):
    """no masks: the three launches give the warp, and the output of the warp launch alone bit for bit"""
    from speech_anonymization_amd import ops, specaug
    plan = specaug.make_plan(B, T, F, c, w, cfg=REFERENCE)
    x = _x(B, T, T + (c or 0))
    out = _run(x, plan)
    r = R.check_output(out, x, plan, f"warp T={T} c={c} w={w}")
    assert not r.fm.any() and not r.tm.any()
    only, part = ops.specaug_warp_sums(x.to(DEV), plan.words().to(DEV))
    assert torch.equal(only, out)
    S = float(part.sum(0)[0])
    print(f"   sum of the warped tensor {S:.9g} (fp64 restatement {float(r.warp.sum()):.9g}), S_fm {float(part.sum(0)[1])}")
    assert abs(S - float(r.warp.sum())) <= r.val_bar * x.numel() and float(part.sum(0)[1]) == 0.0
    if c is None or c == w:
        assert bool(r.exact.all()) and torch.equal(out.cpu(), x)


def test_short_input_drawn_is_the_identity():
    from speech_anonymization_amd import specaug
    aug = specaug.SpecAugment(freq_mask=False, time_mask=False)
    for T in (7, 10):
        x = _x(3, T, T).to(DEV)
        assert torch.equal(aug(x), x) and aug.last_plan.c is None


# ---------------------------------------------------------------------------------------------------
# the masks
# ---------------------------------------------------------------------------------------------------
EIGHT_F = [(2 + 9 * k, 1 + k % 4) for k in range(8)]
EIGHT_T = [(1 + 8 * k, 1 + (k * 3) % 5) for k in range(8)]
MASKS = {
    "length-0": dict(freq=[[(10, 0)], [], [(0, 0), (79, 0)]], time=[[(5, 0)], [(71, 0)], []]),
    "ending-at-D": dict(freq=[[(70, 10)], [(79, 1)], []], time=[[(62, 10)], [], [(71, 1)]]),
    "overlapping": dict(freq=[[(10, 10), (15, 10)], [(3, 2), (4, 1)], []], time=[[(20, 10), (25, 3)], [], [(30, 4), (33, 9)]]),
    "time-and-frequency": dict(freq=[[(8, 5)], [(0, 29)], [(40, 7)]], time=[[(0, 39)], [(31, 2)], []]),
    "freq-only": dict(freq=[[(8, 5)], [(1, 29)], [(40, 7)]], time=()),
    "time-only": dict(freq=(), time=[[(0, 39)], [(31, 2)], []]),
    "eight-per-axis": dict(freq=[EIGHT_F, EIGHT_F[::-1], EIGHT_F[:3]], time=[EIGHT_T, EIGHT_T[:5], EIGHT_T[::-1]]),
}


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("case", list(MASKS))
def test_masks(case, zero):
    """B = 3, T = 72 (a partial tile), warp c = 36 -> w = 33.  check_output: every filled cell of an axis bit-equal
    to one value within the bar of the fp64 mean (== 0 with replace_with_zero), a cell both time- and
    frequency-masked carries the time value, everything else is the warp"""
    from speech_anonymization_amd import specaug
    plan = specaug.make_plan(3, 72, F, 36, 33, cfg=dict(REFERENCE, replace_with_zero=zero), **MASKS[case])
    x = _x(3, 72, 11)
    out = _run(x, plan)
    r = R.check_output(out, x, plan, f"{case} zero={zero}")
    if case == "length-0":
        assert not r.fm.any() and not r.tm.any()
    if case == "ending-at-D":
        assert bool(r.fm[0, 70:].all()) and bool(r.tm[0, 62:].all()) and not bool(r.fm[0, :70].any())
    if case == "time-and-frequency" and not zero:
        assert r.val_f != r.val_t
        assert bool((out[0, :39, 8:13].cpu() == out[0, 0, 0].cpu()).all())        # both masks: the time value
    if case == "eight-per-axis":
        assert int(r.fm[0].sum()) == sum(n for _, n in EIGHT_F) and int(r.tm[0].sum()) == sum(n for _, n in EIGHT_T)
    again = _run(x, plan)
    assert torch.equal(out, again)


def test_drawn_plans_at_the_reference_settings():
    """ten drawn plans (B = 4, T = 108), module call: draw + apply"""
    from speech_anonymization_amd import specaug
    aug = specaug.SpecAugment(seed=3, **REFERENCE)
    aug.reseed(1)
    x = _x(4, 108, 5)
    xd = x.to(DEV)
    seen = set()
    for i in range(10):
        out = aug(xd)
        torch.cuda.synchronize()
        R.check_output(out, x, aug.last_plan, f"drawn {i}")
        seen.add((aug.last_plan.c, aug.last_plan.w))
    assert len(seen) > 1 and torch.equal(xd.cpu(), x)


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals():
    from speech_anonymization_amd import _lib, ops, specaug
    aug = specaug.SpecAugment()
    with pytest.raises(ValueError, match="GPU only"):
        aug(torch.zeros(2, 36, 80))
    with pytest.raises(ValueError, match="float32"):
        aug(torch.zeros(2, 36, 80, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        aug(torch.zeros(2, 80, 36, device=DEV).transpose(1, 2))
    with pytest.raises(ValueError, match="multiple of 4"):
        aug(torch.zeros(2, 36, 78, device=DEV))
    with pytest.raises(ValueError, match="multiple of 4"):
        aug(torch.zeros(2, 36, 132, device=DEV))
    with pytest.raises(ValueError, match="no plan was drawn"):
        aug.apply(torch.zeros(2, 36, 80, device=DEV))
    with pytest.raises(ValueError, match="drawn for"):
        specaug.apply_plan(torch.zeros(2, 37, 80, device=DEV), specaug.make_plan(2, 36, 80))
    x = torch.zeros(2, 36, 80, device=DEV)
    words = specaug.make_plan(2, 36, 80).words().to(DEV)
    with pytest.raises(_lib.SaHipError, match="GPU tensors"):
        ops.specaug_warp_sums(x.cpu(), words)
    with pytest.raises(_lib.SaHipError, match="float32"):
        ops.specaug_warp_sums(x.double(), words)
    with pytest.raises(_lib.SaHipError, match="words"):
        ops.specaug_warp_sums(x, words[:100])
    with pytest.raises(_lib.SaHipError, match="multiple of 4"):
        ops.specaug_fill(torch.zeros(2, 36, 78, device=DEV), words, torch.zeros(2, device=DEV))
    with pytest.raises(_lib.SaHipError, match="aligned"):
        ops.specaug_warp_sums(torch.zeros(2 * 36 * 80 + 1, device=DEV)[1:].view(2, 36, 80), words)
    # the C entry points themselves: -EINVAL before any launch
    lib, st = _lib.load(), _lib.stream()
    out, part, vals = torch.empty_like(x), torch.empty(4, 2, dtype=torch.float64, device=DEV), torch.zeros(2, device=DEV)
    p = _lib.ptr
    for B, T, Fq in ((2, 0, 80), (0, 36, 80), (2, 36, 78), (2, 36, 132), (2, 36, 0), (65536, 36, 80)):
        assert lib.sa_specaug_warp_sums(p(x), p(words), B, T, Fq, p(out), p(part), st) == -22, (B, T, Fq)
        assert lib.sa_specaug_finalize(p(part), p(words), B, T, Fq, p(vals), st) == -22
        assert lib.sa_specaug_fill(p(words), p(vals), B, T, Fq, p(out), st) == -22
    assert lib.sa_specaug_warp_sums(p(x), p(words), 2, 36, 80, p(x), p(part), st) == -22         # in place
    assert lib.sa_specaug_warp_sums(None, p(words), 2, 36, 80, p(out), p(part), st) == -22
    assert lib.sa_specaug_warp_sums(ctypes.c_void_p(x.data_ptr() + 4), p(words), 2, 35, 80, p(out), p(part), st) == -22
    assert lib.sa_specaug_fill(None, p(vals), 2, 36, 80, p(out), st) == -22
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# the train step
# ---------------------------------------------------------------------------------------------------
def _brain(model_type, on, graph=False, seed=7):
    from oracle.convae import numpy_params
    from speech_anonymization_amd import specaug
    from speech_anonymization_amd.brain import Stage
    from tests import smoke_step
    dev = torch.device(DEV)
    torch.manual_seed(8886)
    br = smoke_step.build("bf16x3", dev, numpy_params(8886) if model_type == "convae" else None,
                          run_opts={"hip_graph": graph})
    hp = br.hparams
    if model_type == "endtoend":
        from tests.test_endtoend_gpu import hip_classifier, oracle_classifier
        from speech_anonymization_amd.endtoend import ConvReconstruction
        br.modules["ConvAE"] = ConvReconstruction(hip_classifier(oracle_classifier())).to(dev)
        hp.model_type, hp.recon_loss_weight, hp.sex_loss_weight, hp.confusion_loss_weight = "endtoend", 0.5, 0.4, 0.1
    elif model_type == "fcae":
        from speech_anonymization_amd import fcae
        br.modules["ConvAE"] = fcae.FullyConnectedAutoencoder(80, 4, pooling_noise=False).to(dev)
        hp.model_type = "fcae"
    if model_type != "convae":
        br.optimizer = None
        br.init_optimizers()
    br.modules.train()
    hp.spec_augment = on
    if on:
        hp.augmentation = specaug.SpecAugment(seed=seed, **REFERENCE)
        hp.augmentation.debug = True
    seen = br.seen = dict(inputs=[], targets=[])
    br.modules["ConvAE"].register_forward_pre_hook(lambda m, a: seen["inputs"].append(a[0].detach().clone()))
    loss_r = hp.loss_reconstruction

    def recording(pred, target):
        seen["targets"].append(target.detach().clone())
        return loss_r(pred, target)
    hp.loss_reconstruction = recording
    br.on_stage_start(Stage.TRAIN, 1)
    return br


def _batch(B=4, N=8000):
    from speech_anonymization_amd.brain import Batch
    from tests import smoke_step
    return Batch(smoke_step.make_wave(B, N), torch.tensor([1.0, 0.83, 0.61, 1.0][:B]), torch.arange(B) % 2)


def _step(br, batch, step):
    """step 2 is fit_batch spelled out (smoke_step.hip_step: compute_forward outside fit_batch, so the features()
    path, and the gradients can be read); steps 1 and 3 are fit_batch (input and target from one normalisation pass)"""
    from tests import smoke_step
    torch.manual_seed(100 + step)
    br.seen["inputs"].clear(), br.seen["targets"].clear()
    if step == 2:
        loss, grads = smoke_step.hip_step(br, batch)
    else:
        br.step += 1
        loss, grads = br.fit_batch(batch), None
    torch.cuda.synchronize()
    return loss.clone(), grads


@pytest.mark.parametrize("model_type", ["convae", "endtoend", "fcae"])
def test_fit_batch(model_type):
    """B = 4, 8000 samples (51 frames; 72 after the pad for convae and endtoend).  A forward pre-hook on the model
    records its input, a wrapper of the reconstruction loss the target.  Brains: on, off, and on2 = on again."""
    from speech_anonymization_amd.brain import Stage
    on, off, on2 = _brain(model_type, True), _brain(model_type, False), _brain(model_type, True)
    aug = on.hparams.augmentation
    assert on._specaug is aug and off._specaug is None
    batch = _batch()
    for br in (on, off, on2):                               # VALID: never augmented
        br.modules.eval()
        with torch.no_grad():
            br.compute_forward(batch, Stage.VALID)
        br.modules.train()
    assert torch.equal(on.seen["inputs"][-1], off.seen["inputs"][-1]) and aug.last_plan is None
    T = on.seen["inputs"][-1].shape[1]
    assert T == (51 if model_type == "fcae" else 72)
    losses, words = [], []
    for step in (1, 2, 3):
        loss, grads = _step(on, batch, step)
        losses.append(loss)
        words.append(aug.last_plan.words())
        assert bool(torch.isfinite(loss))
        if grads is not None:
            # every trainable parameter has a finite gradient; every matrix / filter a non-zero one (a conv bias
            # in front of InstanceNorm has a structurally zero gradient: tests/test_convae_gpu.py NULL_BIAS)
            want = [k for k, p in on.modules["ConvAE"].named_parameters() if p.requires_grad]
            filled = sum(grads[k] is not None and bool(torch.isfinite(grads[k]).all()) for k in want)
            mats = [k for k in want if grads[k] is not None and grads[k].dim() >= 2]
            moving = sum(float(grads[k].abs().sum()) > 0 for k in mats)
            print(f"{model_type}: loss {float(loss):.6f}, {filled} of {len(want)} gradients filled, {moving} of "
                  f"{len(mats)} matrices with a non-zero one")
            assert want and filled == len(want) and mats and moving == len(mats)
        if step == 3:
            break
        _step(off, batch, step)
        clean, got = off.seen["inputs"][0], on.seen["inputs"][0]
        assert torch.equal(aug.last_input, clean) and torch.equal(aug.last_output, got)
        plan = aug.last_plan
        assert (plan.B, plan.T, plan.F) == tuple(clean.shape) == (4, T, 80)
        R.check_output(got, clean.cpu(), plan, f"{model_type} step {step}")
        assert plan.c is not None and not torch.equal(got, clean)
        assert len(on.seen["targets"]) == len(off.seen["targets"]) == 1
        assert torch.equal(on.seen["targets"][0], off.seen["targets"][0])          # the target is not augmented
    assert not torch.equal(words[0], words[1])
    # the same seed, epoch and rank: the same plans and, bit for bit, the same losses over three steps
    aug2 = on2.hparams.augmentation
    for step in (1, 2, 3):
        loss2, _ = _step(on2, batch, step)
        assert torch.equal(aug2.last_plan.words(), words[step - 1])
        assert torch.equal(loss2, losses[step - 1]), (step, float(loss2), float(losses[step - 1]))
    # a second epoch draws other plans; reseeding the first rewinds
    on2.on_stage_start(Stage.TRAIN, 2)
    _step(on2, batch, 1)
    assert not any(torch.equal(aug2.last_plan.words(), w) for w in words)
    on2.on_stage_start(Stage.TRAIN, 1)
    _step(on2, batch, 1)
    assert torch.equal(aug2.last_plan.words(), words[0])


def _graph_run():
    """six hipGraph steps at B = 4 (three eager, the capture, two replays).  Under replay no hook runs: the model's
    input is read from the module's own output tensor of the captured step (``debug`` keeps a reference to it and
    to the normaliser's output it was made from; both live in the graph's pool and are rewritten by every replay)."""
    br = _brain("convae", True, graph=True)
    aug = br.hparams.augmentation
    batches = [_batch(), _batch()]
    batches[1].sig = (batches[1].sig[0] * 0.8, batches[1].sig[1])
    res = dict(plans=[], worst=[])
    for step in range(1, 7):
        br.step += 1
        loss = br.fit_batch(batches[step % 2])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        if step >= 5:
            assert any("graph" in e for e in br._graphs.values())
            plan = aug.last_plan
            R.check_output(aug.last_output, aug.last_input.cpu(), plan, f"hipGraph step {step}")
            res["plans"].append(plan.words().tolist())
            res["inputs_differ"] = not torch.equal(aug.last_output, aug.last_input)
    res["captured"] = sum("graph" in e for e in br._graphs.values())
    res["hook_calls"] = len(br.seen["inputs"])
    res["plans_differ"] = res["plans"][0] != res["plans"][1]
    del res["plans"]
    print("RESULT " + json.dumps(res))


def test_hip_graph_steps():
    """one fresh process, six steps with hip_graph on; the model's input of steps 5 and 6 (replays) is the
    restatement of that step's plan, and the two plans differ"""
    r = subprocess.run([sys.executable, "-m", "tests.test_specaug_gpu"], capture_output=True, text=True, timeout=180,
                       cwd=ROOT)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["captured"] == 1 and res["plans_differ"] and res["inputs_differ"]
    assert res["hook_calls"] == 4                           # three eager steps and the capture; no hook under replay


# ---------------------------------------------------------------------------------------------------
# the entry script
# ---------------------------------------------------------------------------------------------------
def test_entry_script(tmp_path):
    """--synthetic 12 --spec_augment true --number_of_epochs 1 in a fresh process: the "on" line, a checkpoint
    that a second run resumes from; without --spec_augment the line is absent"""
    base = [sys.executable, os.path.join(ROOT, "speechbrain_convae_train.py"),
            os.path.join(ROOT, "speechbrain_configs", "convae.yaml"), "--device", DEV, "--synthetic", "12"]
    LINE = "SpecAugment of the input features on"

    def run(folder, *more):
        r = subprocess.run(base + ["--folder", str(folder)] + list(more), capture_output=True, text=True,
                           timeout=180, cwd=ROOT)
        print(r.stdout[-1500:], r.stderr[-1500:])
        assert r.returncode == 0
        return r.stdout

    out = run(tmp_path / "on", "--spec_augment", "true", "--number_of_epochs", "1")
    assert LINE in out and "window 5" in out and "under 30 bins" in out and "under 40 frames" in out
    log = tmp_path / "on" / "8886" / "train_log.txt"
    assert len(open(log).read().strip().splitlines()) == 1
    assert any(d.startswith("CKPT+") for d in os.listdir(tmp_path / "on" / "8886" / "save"))
    out = run(tmp_path / "on", "--spec_augment", "true", "--number_of_epochs", "2")
    lines = open(log).read().strip().splitlines()
    assert LINE in out and len(lines) == 2 and lines[1].startswith("epoch: 2, ")
    out = run(tmp_path / "off", "--number_of_epochs", "1", "--synthetic_samples", "16000")
    assert LINE not in out and "SpecAugment" not in out


if __name__ == "__main__":
    _graph_run()
