"""Whole-step parity on the GPU (Brain hooks -> HIP library) against the oracle's step."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_train_step_fp32_matches_oracle():
    from tests import smoke_step
    smoke_step.run(torch.float32)


def test_train_step_bf16x3_matches_oracle():
    from tests import smoke_step
    smoke_step.run("bf16x3")


def test_train_step_bf16_runs_and_tracks_oracle():
    from tests import smoke_step
    smoke_step.run(torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, "bf16x3"], ids=["f32", "bf16x3"])
def test_teacher_forced_four_steps(dtype):
    """steps 2-4 pinned at the step-1 tolerance (loss 3e-5 / 3e-4, every gradient 2e-5 / 1e-4)"""
    from tests import smoke_step
    smoke_step.run_teacher_forced(dtype, steps=4)


@pytest.mark.parametrize("dtype", [torch.float32, "bf16x3"], ids=["f32", "bf16x3"])
def test_endtoend_adversarial_sign_branch(dtype):
    """model_type endtoend: recon_w*recon - sex_w*sex + util_w*util - conf_w*confusion
    (speechbrain_convae_train.py:111-121), including a non-zero confusion weight"""
    from tests import smoke_step
    smoke_step.run_teacher_forced(dtype, steps=2, model_type="endtoend",
                                  weights=dict(recon=0.3, sex=0.6, utility=0.0, confusion=0.2))
    # and its "sex only" sub-branch (:112-113)
    smoke_step.run_teacher_forced(dtype, steps=1, model_type="endtoend",
                                  weights=dict(recon=0.0, sex=0.7, utility=0.0, confusion=0.2))


@pytest.mark.parametrize("dtype", [torch.float32, "bf16x3"], ids=["f32", "bf16x3"])
def test_epoch_parity_schedule_both_halves(dtype):
    """HEAD's schedule (speechbrain_convae_train.py:212-235): odd epoch = only the sex classifier
    trains (sex 0.5; encoder + decoder frozen: the backward stops at the classifier input), even
    epoch = classifier frozen, encoder/decoder train against it (sex 0.8).  The sequence
    odd, odd, even, odd also exercises torch 1.10's zero-filled gradients of frozen parameters
    (Adam keeps moving them on their moments)."""
    from tests import smoke_step
    smoke_step.run_teacher_forced(dtype, steps=4, epoch_parity_schedule=True, epochs=[1, 1, 2, 3])


def test_hip_graph_step_equals_eager_steps():
    """run_opts hip_graph=True: three eager steps, capture, then replays -- against the same steps
    launched eagerly (same kernels in the same order; Adam differs only in where its bias
    corrections are evaluated: on the device in the capturable form)."""
    from oracle.convae import numpy_params
    from tests import smoke_step
    from speech_anonymization_amd.brain import Batch
    dev = torch.device("cuda:0")
    wav = smoke_step.make_wave(4, 11360)
    batches = [Batch(wav * s, torch.tensor([1.0, 0.83, 0.61, 1.0]), torch.arange(4) % 2) for s in (1.0, 0.9, 0.8, 1.1, 0.7, 1.05, 0.95)]
    runs = []
    for graph in (False, True):
        br = smoke_step.build("bf16x3", dev, numpy_params(8886))
        if graph:
            import functools
            br.hip_graph, br.optimizer = True, None
            br.init_optimizers()
            assert torch.is_tensor(br.optimizer.param_groups[0]["lr"])
        losses = []
        for b in batches:
            br.step += 1
            losses.append(float(br.fit_batch(b)))
        torch.cuda.synchronize()
        if graph:
            assert len(br._graphs) == 1 and "graph" in next(iter(br._graphs.values()))
        runs.append((losses, {k: v.detach().clone() for k, v in br.modules["ConvAE"].state_dict().items()},
                     br.hparams.noam_annealing.n_steps, br.modules["normalize"].count))
    (l0, p0, n0, c0), (l1, p1, n1, c1) = runs
    assert n0 == n1 == len(batches) and c0 == c1
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (l0, l1)
    for k in p0:
        if p0[k].dtype.is_floating_point:
            assert float((p0[k] - p1[k]).abs().max()) <= 2e-6 + 1e-5 * float(p0[k].abs().max()), k


def test_hip_graph_follows_the_epoch_parity_schedule():
    """hipGraph mode over epochs 0, 1, 2 of HEAD's epoch-parity schedule
    (speechbrain_convae_train.py:212-235).  Epoch 0 freezes the classifier while it has no Adam
    moments (it stays out of the update); epoch 1 trains it; in epoch 2 it is frozen again but now
    HAS moments, and torch 1.10's zero-filled gradients keep moving it -- the same requires_grad
    pattern as epoch 0 with a different step.  The graph key carries the optimizer state of the
    frozen parameters, so epoch 2 captures its own graph; parameters equal the eager run's."""
    from oracle.convae import numpy_params
    from tests import smoke_step
    from speech_anonymization_amd.brain import Batch
    dev = torch.device("cuda:0")
    wav = smoke_step.make_wave(4, 11360)
    scales = (1.0, 0.9, 0.8, 1.1, 0.7)
    runs = []
    for graph in (False, True):
        br = smoke_step.build("bf16x3", dev, numpy_params(8886))
        br.hparams.epoch_parity_schedule = True
        if graph:
            br.hip_graph, br.optimizer = True, None
            br.init_optimizers()
        for epoch in (0, 1, 2):
            br.hparams.epoch_counter.current = epoch
            for s_ in scales:
                br.step += 1
                br.fit_batch(Batch(wav * s_, torch.tensor([1.0, 0.83, 0.61, 1.0]), torch.arange(4) % 2))
        torch.cuda.synchronize()
        if graph:
            assert len(br._graphs) == 3, list(br._graphs)          # one per epoch: 0 and 2 differ by the moments
        runs.append({k: v.detach().clone() for k, v in br.modules["ConvAE"].state_dict().items()})
    p0, p1 = runs
    moved = 0
    for k in p0:
        if p0[k].dtype.is_floating_point:
            assert float((p0[k] - p1[k]).abs().max()) <= 5e-6 + 2e-5 * float(p0[k].abs().max()), k
    # the classifier did move in epoch 2 of the eager run (the semantics under test)
    ref = numpy_params(8886)
    assert float((p0["sex_classifier.classify.6.weight"].cpu() - ref["sex_classifier.classify.6.weight"]).abs().max()) > 0


def test_frozen_classifier_and_recon_only():
    """the reference's requires_grad toggling by name (speechbrain_convae_train.py:219-235) and
    config 1 (recon 1.0 only, MSE): frozen parameters get no gradient, the rest still match."""
    from oracle.convae import numpy_params
    from tests import smoke_step
    from speech_anonymization_amd.brain import Batch, Stage
    dev = torch.device("cuda:0")
    br = smoke_step.build(torch.float32, dev, numpy_params(8886))
    br.hparams.recon_loss_weight, br.hparams.sex_loss_weight = 1.0, 0.0
    for name, p in br.modules["ConvAE"].named_parameters():
        p.requires_grad = "sex_classifier" not in name
    wav = smoke_step.make_wave(3, 11360)
    batch = Batch(wav, torch.ones(3), torch.arange(3) % 2)
    out = br.compute_forward(batch, Stage.TRAIN)
    loss = br.compute_objectives(out, batch, Stage.TRAIN)
    loss.backward()
    torch.cuda.synchronize()
    for name, p in br.modules["ConvAE"].named_parameters():
        if "sex_classifier" in name:
            assert p.grad is None, name
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name


def test_entry_script_config1_plumbing(tmp_path):
    """BASELINE config 1 on the GPU path: speechbrain_convae_train.py + convae.yaml, recon 1.0 only
    (MSE), gradient accumulation 3, synthetic utterances; writes train_log.txt and a checkpoint
    directory with the reference's layout."""
    import os
    import speechbrain_convae_train as entry
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "speechbrain_configs", "convae.yaml")
    entry.main([cfg, "--device", "cuda:0", "--model_type", "convae", "--folder", str(tmp_path),
                "--number_of_epochs", "2", "--batch_size", "2", "--synthetic", "12",
                "--synthetic_samples", "11360"])
    out = tmp_path / "8886"
    lines = open(out / "train_log.txt").read().strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("epoch: 1, lr: ") and "train loss" in lines[0]
    assert "steps: 2" in lines[0]                       # 6 batches / gradient_accumulation 3
    l1 = float(lines[0].split("train loss: ")[1].split(" ")[0])
    l2 = float(lines[1].split("train loss: ")[1].split(" ")[0])
    assert l2 < l1                                      # recon-only MSE goes down
    ck = sorted(os.listdir(out / "save"))
    assert ck and ck[-1].startswith("CKPT+")
    assert {"model.ckpt", "normalizer.ckpt", "noam_scheduler.ckpt", "counter.ckpt", "CKPT.yaml"} <= set(
        os.listdir(out / "save" / ck[-1]))


def test_bench_plain_run_dumps_the_last_step(tmp_path):
    """`bench.py` without --full times the headline configuration only, and --dump-outputs writes
    the last timed step's loss and the model state it left as float32 .npy files"""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3",
                          "--warmup", "1", "--batch", "2", "--samples", str(36 * 160 * 2 - 160),
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["full"] is False
    assert rec["config"]["b10"] is None and rec["roofline"] is None and "cpu_baseline" not in rec
    arrays = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert float(arrays["loss"]) == rec["config"]["loss"]
    assert {"recon_loss", "sex_loss", "ConvAE.encoder.0.weight", "normalize.state"} <= set(arrays)
    assert all(np.isfinite(a).all() for a in arrays.values())


def test_fused_clip_takes_the_buckets_only_when_every_gradient_lives_there():
    """Brain._grad_flats: after a plain backward every .grad is a view of the three stage buckets (the two-launch
    clip applies); with a frozen stage, a frozen single parameter or an accumulated second backward it does not
    (torch's clip runs), and both clips move the parameters the same way."""
    from oracle.convae import numpy_params
    from tests import smoke_step
    from speech_anonymization_amd.brain import Batch, Stage
    dev = torch.device("cuda:0")
    wav = smoke_step.make_wave(4, 11360)
    batch = Batch(wav, torch.ones(4), torch.arange(4) % 2)

    def backward(br):
        out = br.compute_forward(batch, Stage.TRAIN)
        br.compute_objectives(out, batch, Stage.TRAIN).backward()
        return list(br.modules.parameters())
    br = smoke_step.build("bf16x3", dev, numpy_params(8886))
    params = backward(br)
    flats = br._grad_flats(params)
    assert flats is not None and len(flats) == 3 and sum(f.numel() for f in flats) == sum(p.numel() for p in params)
    params = backward(br)                                           # accumulated: .grad still lives in the first buckets
    assert br._grad_flats(params) is None
    br.optimizer.zero_grad()
    name, p0 = next(iter(br.modules["ConvAE"].named_parameters()))
    p0.requires_grad = False                                        # one parameter of a stage frozen: a hole in its bucket
    params = backward(br)
    assert br._grad_flats(params) is None
    p0.requires_grad = True
    br.optimizer.zero_grad()
    for n_, p in br.modules["ConvAE"].named_parameters():
        p.requires_grad = "sex_classifier" not in n_                # a whole stage frozen: two buckets
    params = backward(br)
    flats = br._grad_flats(params)
    assert flats is not None and len(flats) == 2
    # same step with either clip (max_grad_norm small enough to bite)
    res = []
    for fused in (True, False):
        b2 = smoke_step.build("bf16x3", dev, numpy_params(8886))
        b2.fused_clip, b2.max_grad_norm = fused, 0.05
        b2.step += 1
        b2.fit_batch(batch)
        torch.cuda.synchronize()
        res.append({k: v.detach().clone() for k, v in b2.modules["ConvAE"].state_dict().items() if v.dtype.is_floating_point})
    for k in res[0]:
        assert float((res[0][k] - res[1][k]).abs().max()) <= 1e-6 + 1e-5 * float(res[1][k].abs().max()), k


def _four_batches():
    from tests import smoke_step
    from speech_anonymization_amd.brain import Batch
    wav = smoke_step.make_wave(4, 11360)
    return [Batch(wav * s, torch.tensor([1.0, 0.83, 0.61, 1.0]), torch.arange(4) % 2) for s in (1.0, 0.9, 0.8, 1.1)]


def _steps(br, batches):
    for b in batches:
        torch.manual_seed(1234)
        br.step += 1
        br.fit_batch(b)
    torch.cuda.synchronize()


def _adam_state(br):
    st = br.optimizer.state
    return {k: {m: st[p][m].detach().clone() for m in ("exp_avg", "exp_avg_sq", "step") if m in st[p]}
            for k, p in br.modules["ConvAE"].named_parameters() if p in st and len(st[p])}


_RESUME_MODES = {"eager": dict(run_opts={}, adam={}), "hipGraph": dict(run_opts={"hip_graph": True}, adam={}),
                 "plain": dict(run_opts={}, adam={"fused": False})}
_RESUME_PAIRS = [("eager", "eager"), ("eager", "hipGraph"), ("hipGraph", "eager"), ("hipGraph", "hipGraph"),
                 ("plain", "plain")]


@pytest.mark.parametrize("writer,reader", _RESUME_PAIRS, ids=[f"{w}-to-{r}" for w, r in _RESUME_PAIRS])
def test_resume_continues_the_run(tmp_path, writer, reader):
    """A run resumed from a checkpoint continues the one that wrote it.  Writer: 3 steps, save, then 2 more steps
    as the reference.  Reader: a new Brain (its own mode: eager = torch's fused Adam, hipGraph = fused + capturable
    with a device learning rate, plain = Adam(fused=False)) resumes in on_fit_start.  BEFORE any step (a fused
    step with host step counts would hand the kernel host pointers): the optimizer groups carry the reader's own
    fused / foreach / capturable flags, not the writer's; lr is a float (eager) or a device tensor (hipGraph) and
    Noam's host copy is set; every Adam step count sits on its parameter's device for the fused and the capturable
    step, on the host for the plain one; the moments, Noam's step count, the epoch counter and the normaliser
    equal the writer's bit for bit.  Then the same 2 steps: same-mode pairs give the reference's bits (the step is
    deterministic: tests/test_shapes_gpu.py), cross-mode pairs agree to the tolerance of
    test_hip_graph_step_equals_eager_steps (the capturable Adam evaluates its bias corrections on the device),
    their moments to 1e-4 of their largest element."""
    from oracle.convae import numpy_params
    from tests import smoke_step
    from speech_anonymization_amd.checkpoint import Checkpointer
    dev = torch.device("cuda:0")
    batches = _four_batches() + _four_batches()[:1]
    wm, rm = _RESUME_MODES[writer], _RESUME_MODES[reader]
    br = smoke_step.build("bf16x3", dev, numpy_params(8886), checkpointer=Checkpointer(tmp_path / "save"), **wm)
    assert br.resumed_from is None
    _steps(br, batches[:3])
    saved = br.checkpointer.save(br, epoch=1)
    moments = _adam_state(br)
    nrm_state = br.modules["normalize"].state.detach().clone()
    _steps(br, batches[3:])
    ref_params = {k: v.detach().clone() for k, v in br.modules["ConvAE"].state_dict().items()}
    ref_moments = _adam_state(br)
    del br

    br = smoke_step.build("bf16x3", dev, numpy_params(8886), checkpointer=Checkpointer(tmp_path / "save"), **rm)
    assert br.resumed_from == saved
    opt = br.optimizer
    graph = reader == "hipGraph"
    fused = rm["adam"].get("fused", True)
    for g in opt.param_groups:
        assert bool(g.get("fused")) == fused and bool(g.get("capturable")) == graph, (g.get("fused"), g.get("capturable"))
        assert g.get("foreach") is None, g.get("foreach")
        if graph:
            assert torch.is_tensor(g["lr"]) and g["lr"].device == dev
        else:
            assert isinstance(g["lr"], float)
        assert isinstance(opt._sa_host_lr, float) and abs(opt._sa_host_lr - float(g["lr"])) <= 1e-7 * opt._sa_host_lr
        for p in g["params"]:
            step = opt.state[p]["step"]
            assert step.device == (p.device if fused or graph else torch.device("cpu")), (step.device, p.device)
            assert float(step) == 3.0
    for k, st in _adam_state(br).items():
        for m in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[m], moments[k][m]), (k, m)
    assert set(_adam_state(br)) == set(moments)
    assert br.hparams.noam_annealing.n_steps == 3 and br.hparams.epoch_counter.current == 1
    assert torch.equal(br.modules["normalize"].state, nrm_state)
    _steps(br, batches[3:])
    assert br.hparams.noam_annealing.n_steps == 5
    got, got_m = br.modules["ConvAE"].state_dict(), _adam_state(br)
    for k, v in ref_params.items():
        if writer == reader:
            assert torch.equal(got[k], v), k
        elif v.dtype.is_floating_point:
            assert float((got[k] - v).abs().max()) <= 2e-6 + 1e-5 * float(v.abs().max()), k
    for k, st in ref_moments.items():
        for m in ("exp_avg", "exp_avg_sq"):
            a, b = got_m[k][m], st[m]
            if writer == reader:
                assert torch.equal(a, b), (k, m)
            else:
                # step 5's gradient comes from parameters that may differ in a last bit (the classifier's
                # BatchNorm amplifies that ~1e3x), and the moment takes 1 - beta of it
                assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-30, (k, m)


def test_check_gradients_with_a_nan_gradient_fused_equals_torch():
    """Brain.check_gradients on a non-finite loss, one NaN written into one .grad (a view of a stage bucket): the
    fused clip (the buckets) and torch's clip_grad_norm_ leave the same gradients, NaN masks included, with the
    lazy device-side check (the clip runs: a NaN norm makes every gradient NaN, as in torch) and with the
    synchronous one (check_gradients returns False before any clip: the gradients stay as they were, count 1)."""
    from oracle.convae import numpy_params
    from tests import smoke_step
    from speech_anonymization_amd.brain import Stage
    dev = torch.device("cuda:0")
    batch = _four_batches()[0]
    nan_loss = torch.tensor(float("nan"), device=dev)
    for lazy in (True, False):
        br = smoke_step.build("bf16x3", dev, numpy_params(8886))
        br.lazy_finite_check = lazy
        out = br.compute_forward(batch, Stage.TRAIN)
        br.compute_objectives(out, batch, Stage.TRAIN).backward()
        params = list(br.modules.parameters())
        p0 = br.modules["ConvAE"].encoder[2].weight
        p0.grad.view(-1)[5] = float("nan")
        before = [p.grad.clone() for p in params]
        res = {}
        for fused in (True, False):
            for p, g in zip(params, before):
                p.grad.copy_(g)                               # in place: the views into the buckets stay
            br.fused_clip = fused
            br.nonfinite_count = 0
            if fused:
                assert br._grad_flats(params) is not None     # the fused path is the one taken
            ok = br.check_gradients(nan_loss)
            torch.cuda.synchronize()
            res[fused] = [p.grad.clone() for p in params]
            if lazy:
                assert ok and br.nonfinite_count == 0
                assert br._poll_nonfinite(wait=True) == 1     # the device counter has it
            else:
                assert ok is False and br.nonfinite_count == 1
        for a, b, g in zip(res[True], res[False], before):
            assert torch.equal(torch.isnan(a), torch.isnan(b))
            assert torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])
            if lazy:
                assert bool(torch.isnan(a).all())
            else:
                assert torch.equal(a.view(torch.int32), g.view(torch.int32))


_NONFINITE_MODES = {"eager-sync": dict(lazy_finite_check=False), "eager-lazy": dict(lazy_finite_check=True),
                    "hipGraph": dict(lazy_finite_check=True, hip_graph=True)}


@pytest.mark.parametrize("mode", list(_NONFINITE_MODES))
def test_corrupt_utterance_counts_against_its_own_epoch(mode):
    """Brain.fit over one short epoch whose last batch holds a NaN sample (a corrupt utterance); in hipGraph mode
    that batch replays the captured step.  The non-finite loss counts against THIS epoch (count 1 at its end:
    the lazy device counter is drained at the epoch's one host read, so a NaN on the last steps is not counted
    against the next epoch), and with nonfinite_patience=0 two such batches raise ValueError by the end of the
    epoch.  The synchronous check reports the step (check_gradients returns False, nothing is clipped) but, like
    the reference (speechbrain_convae_train.py:249-251 ignores check_gradients' result), the optimizer still
    steps.  No kernel of the step turns a data value into an address or a loop bound (lengths and labels only),
    so the NaN only travels as a value.
    The HIP Fbank and the fused normalisation map a non-finite sample to their floors (fmaxf drops the NaN that
    the reference's torch.clamp / torch.max would keep), so the corrupt utterance alone never reaches the loss as
    NaN: a hook adds 0 * (the utterance's first sample) to the normalised features, captured with the step,
    which carries the NaN on as the reference's features would."""
    from oracle.convae import numpy_params
    from tests import smoke_step
    from speech_anonymization_amd.brain import Batch, EpochCounter, Stage
    dev = torch.device("cuda:0")
    opts = dict(_NONFINITE_MODES[mode], gc_freeze=False)
    clean = _four_batches()
    wav, lens = clean[-1].sig
    bad = wav.clone()
    bad[2, 0] = float("nan")
    corrupt = Batch(bad, lens, clean[-1].gender)

    def run(batches, patience):
        br = smoke_step.build("bf16x3", dev, numpy_params(8886), run_opts=dict(opts, nonfinite_patience=patience))
        ec = br.hparams.epoch_counter = EpochCounter(1)
        feats = br.features
        br.features = lambda w, lens: feats(w, lens) + (w[:, :1] * 0.0).unsqueeze(-1)
        counts, checks = [], []
        stage_end, check = br.on_stage_end, br.check_gradients
        br.on_stage_end = lambda stage, loss, epoch=None: (
            counts.append(br.nonfinite_count) if stage == Stage.TRAIN else None, stage_end(stage, loss, epoch))
        br.check_gradients = lambda loss: checks.append(check(loss)) or checks[-1]
        br.fit(ec, batches)
        torch.cuda.synchronize()
        return br, counts, checks

    br, counts, checks = run(clean + [corrupt], 3)
    assert counts == [1], counts
    if mode == "eager-sync":
        assert checks == [True] * 4 + [False], checks
    if mode == "hipGraph":
        ent = next(iter(br._graphs.values()))
        assert len(br._graphs) == 1 and "graph" in ent and len(checks) == 4      # 3 warmups + the capture
    with pytest.raises(ValueError, match="not finite"):
        run(clean + [corrupt, corrupt], 0)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipGraph"])
def test_half_steps_clip_their_own_buckets(graph):
    """Epochs 1, 1, 2, 3, 0 of the epoch-parity schedule (odd: the classifier alone, its backward returns early;
    even: the classifier frozen), four steps each, with the fused clip biting (max_grad_norm 0.05).  At every
    check_gradients -- every eager step; in hipGraph mode the warmups and the capture each replay repeats -- the
    model's _last_flats are this backward's buckets: each holds one of this step's .grad, or there are none, and
    Brain._grad_flats returns either exactly them or None (torch's clip).  The same sequence with fused_clip off
    leaves the same parameters to the tolerance of
    test_fused_clip_takes_the_buckets_only_when_every_gradient_lives_there."""
    from oracle.convae import numpy_params
    from tests import smoke_step
    dev = torch.device("cuda:0")
    batches = _four_batches()
    runs = []
    for fused in (True, False):
        br = smoke_step.build("bf16x3", dev, numpy_params(8886),
                              run_opts={"hip_graph": graph, "fused_clip": fused, "max_grad_norm": 0.05})
        br.hparams.epoch_parity_schedule = True
        model, check = br.modules["ConvAE"], br.check_gradients
        seen = {"checks": 0, "fused": 0}

        def checked(loss):
            params = list(br.modules.parameters())
            ptrs = [p.grad.data_ptr() for p in params if p.grad is not None]
            flats = list(model._last_flats or [])
            for f in flats:
                lo, hi = f.data_ptr(), f.data_ptr() + 4 * f.numel()
                assert any(lo <= a < hi for a in ptrs), "stale gradient bucket"
            gf = br._grad_flats(params)
            assert gf is None or [f.data_ptr() for f in gf] == [f.data_ptr() for f in flats]
            seen["checks"] += 1
            seen["fused"] += gf is not None
            return check(loss)
        br.check_gradients = checked
        for epoch in (1, 1, 2, 3, 0):
            br.hparams.epoch_counter.current = epoch
            for b in batches:
                br.step += 1
                br.fit_batch(b)
        torch.cuda.synchronize()
        if graph:
            assert len(br._graphs) == 3 and all("graph" in e for e in br._graphs.values()), list(br._graphs)
            assert seen["checks"] == 3 * 4
        else:
            assert seen["checks"] == 20
        if fused:
            assert seen["fused"] > 0
        runs.append({k: v.detach().clone() for k, v in model.state_dict().items() if v.dtype.is_floating_point})
    for k in runs[0]:
        assert float((runs[0][k] - runs[1][k]).abs().max()) <= 1e-6 + 1e-5 * float(runs[1][k].abs().max()), k
