"""The short dependent launches between the forward's last convolution and the first big backward kernel:
the one-launch loss tail (run_opts step_tail: sa_recon_loss_part + sa_step_loss, backward started from the model
outputs), the pooling finaliser in the gather launch (ConvAutoencoder.fused_pool_fin: sa_pool_gather_fin) and the
head backward over 16 workgroups (ConvAutoencoder.wide_head_bwd: sa_head_bwd_wide), each against the launch
sequence it replaces, bit for bit: whole train steps (eager, hipGraph, with pooling noise, a non-finite loss, the
configurations that must stay on the old path) and every new entry point alone."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N = 2, 36 * 160 * 2 - 160             # T = 72 frames
SCALES = (1.0, 0.9, 0.8)
DEV = "cuda:0"


def _eq(a, b):
    """torch.equal that also holds where both sides carry a NaN"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    fix = lambda t: torch.nan_to_num(t, nan=1.5e38, posinf=2.5e38, neginf=-2.5e38)
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(fix(a), fix(b))


def _batches(scales=SCALES):
    from tests import smoke_step
    from speech_anonymization_amd.brain import Batch
    wav = smoke_step.make_wave(B, N)
    return [Batch(wav * s, torch.tensor([1.0, 0.83]), torch.arange(B) % 2) for s in scales]


class _StubASR:
    """a frozen `recogniser` whose posteriors are half its input features: differentiable, no parameters"""

    def get_predictions(self, feats, wav_lens, tokens_bos, batch=None, eval=True, do_ctc=True):
        return None, feats * 0.5


def _run(on, graph=False, steps=None, noise=None, seed=None, endtoend=False, accumulate=1, utility=0.0,
         batches=None, knobs=None, nan_hook=False):
    """three steps (or `steps`, cycling the batches) with the three knobs on or off (knobs: (step_tail,
    fused_pool_fin, wide_head_bwd) one by one) -> (per-step losses, model state, normaliser state, non-finite
    bookkeeping, calls of the native tail)"""
    tail, pool, wide = knobs or (on, on, on)
    from oracle.convae import numpy_params
    from tests import smoke_step
    dev = torch.device(DEV)
    torch.manual_seed(8886)
    br = smoke_step.build("bf16x3", dev, None if endtoend else numpy_params(8886),
                          run_opts={"step_tail": tail, "hip_graph": graph})
    hp = br.hparams
    if endtoend:
        from tests.test_endtoend_gpu import hip_classifier, oracle_classifier
        from speech_anonymization_amd.endtoend import ConvReconstruction
        br.modules["ConvAE"] = ConvReconstruction(hip_classifier(oracle_classifier())).to(dev)
        br.optimizer = None
        br.init_optimizers()
        hp.model_type, hp.recon_loss_weight, hp.sex_loss_weight, hp.confusion_loss_weight = "endtoend", 0.5, 0.4, 0.1
    if utility:
        from speech_anonymization_amd import losses
        br.asr_brain, hp.loss_utility, hp.utility_loss_weight = _StubASR(), losses.CosineSimilarityLoss(), utility
    hp.gradient_accumulation = accumulate
    if nan_hook:
        feats = br.features
        br.features = lambda w, lens: feats(w, lens) + (w[:, :1] * 0.0).unsqueeze(-1)
    model = br.modules["ConvAE"]
    model.wide_head_bwd, model.fused_pool_fin = wide, pool
    model.pooling_noise = noise.to(dev) if torch.is_tensor(noise) else noise
    assert br.step_tail == tail
    calls = [0]
    native = br._objectives_native

    def counted(*a, **kw):
        calls[0] += 1
        return native(*a, **kw)
    br._objectives_native = counted
    out = []
    batches = batches or _batches()
    if steps:
        batches = [batches[i % len(batches)] for i in range(steps)]
    if seed is not None:
        torch.manual_seed(seed)
    for batch in batches:
        br.step += 1
        loss = br.fit_batch(batch)
        out.append(dict(loss=loss.clone(), recon=br.last_losses["recon"].clone(), sex=br.last_losses["sex"].clone()))
    br.nonfinite_count += br._poll_nonfinite(wait=True)
    torch.cuda.synchronize()
    if graph:
        assert any("graph" in e for e in br._graphs.values())
    fin = dict(dev=br._finite_state["dev"].clone(), count=torch.tensor(br.nonfinite_count))
    return (out, {k: v.detach().clone() for k, v in model.state_dict().items()}, br.modules["normalize"].state.clone(),
            fin, calls[0])


def _same(a, b, native_calls):
    (la, pa, sa, fa, ca), (lb, pb, sb, fb, cb) = a, b
    assert ca == 0 and cb == native_calls, (ca, cb)
    assert len(la) == len(lb)
    for i, (x, y) in enumerate(zip(la, lb)):
        assert x.keys() == y.keys()
        for k in x:
            assert _eq(x[k], y[k]), (i, k, x[k], y[k])
    assert pa.keys() == pb.keys()
    for k in pa:
        assert _eq(pa[k], pb[k]), k
    assert _eq(sa, sb)
    for k in fa:
        assert torch.equal(fa[k], fb[k]), (k, fa[k], fb[k])


def test_three_steps_equal_eager():
    off, on = _run(False), _run(True)
    _same(off, on, native_calls=3)
    assert all(bool(torch.isfinite(x["loss"])) for x in on[0]) and int(on[3]["count"]) == 0


def test_hip_graph_steps_equal():
    """GRAPH_WARMUP eager steps, the capture and two replays: the native tail runs in the three eager steps and
    once more while the step is captured"""
    _same(_run(False, graph=True, steps=6), _run(True, graph=True, steps=6), native_calls=4)


def test_three_steps_equal_with_drawn_pooling_noise():
    """pooling_noise=True: the draw is torch's (same seed, same values), its normalisation moves into the launch"""
    _same(_run(False, noise=True, seed=123), _run(True, noise=True, seed=123), native_calls=3)


def test_three_steps_equal_with_given_pooling_noise():
    noise = torch.rand(B, 128, generator=torch.Generator().manual_seed(5))
    _same(_run(False, noise=noise), _run(True, noise=noise), native_calls=3)


def test_nonfinite_step_counts_and_updates_like_before():
    """a batch scaled by infinity: the loss is not finite; device counter, nonfinite_count after the poll and
    every parameter after the step are those of the old path.  (The HIP front end maps non-finite samples to its
    floors, so -- as in tests/test_train_step_gpu.py -- a hook adds 0 * (first sample) to the features, which
    carries the NaN on as the reference's features would.)"""
    scales = (1.0, float("inf"))
    off = _run(False, batches=_batches(scales), nan_hook=True)
    on = _run(True, batches=_batches(scales), nan_hook=True)
    _same(off, on, native_calls=2)
    assert not bool(torch.isfinite(on[0][1]["loss"]))
    assert int(on[3]["dev"]) == 1 and int(on[3]["count"]) == 1


@pytest.mark.parametrize("case", ["endtoend", "accumulation", "utility"])
def test_other_objectives_stay_on_the_old_path(case):
    """endtoend's signed sum (weights 0.5, 0.4, 0.1), gradient_accumulation = 2 and a non-zero utility weight
    with a recogniser attached never take the native tail, and equal a run with the knobs off"""
    kw = dict(endtoend=dict(endtoend=True), accumulation=dict(accumulate=2, steps=4),
              utility=dict(utility=0.2))[case]
    _same(_run(False, **kw), _run(True, **kw), native_calls=0)


@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("weights", [(0.1, 0.9), (1.0, 0.0), (0.0, 1.0)])
@pytest.mark.parametrize("Bn", [1, 2, 32])
def test_step_loss_equals_the_loss_modules_and_autograd(Bn, weights, kind):
    """ops.step_loss against recon_loss + cls_losses + `w_r * recon + w_s * sex + 0.0` + backward: the three
    scalars, d log p and d recon.  Row lengths: one with a tail past the last float4 (B = 1, 2), and 184 320
    elements = 180 partial sums, more than the finaliser's 64 lanes (B = 32)"""
    from speech_anonymization_amd import losses, ops
    g = torch.Generator().manual_seed(17 * Bn)
    row = 5760 if Bn == 32 else 5761
    pred = torch.randn(Bn, row, generator=g).to(DEV)
    target = torch.randn(Bn, row, generator=g).to(DEV)
    target[0, :7] = pred[0, :7]                                  # zero differences: sign(0) = 0 in the L1 gradient
    logp = torch.log_softmax(torch.randn(Bn, 2, generator=g), dim=1).to(DEV)
    label = (torch.arange(Bn) % 2).to(DEV)
    wr, ws = weights
    p, lp = pred.clone().requires_grad_(True), logp.clone().requires_grad_(True)
    recon = losses.ReconLoss(kind)(p, target)
    sex = losses.NLLLoss()(lp, label)
    total = wr * recon + ws * sex + 0.0
    total.backward()
    cnt = torch.zeros((), dtype=torch.int32, device=DEV)
    out, d_pred, d_logp = ops.step_loss(pred, target, kind, logp, label, wr, ws, nonfinite=cnt)
    torch.cuda.synchronize()
    assert torch.equal(out[0], recon.detach()) and torch.equal(out[1], sex.detach())
    assert torch.equal(out[2], total.detach()), (out[2], total)
    assert torch.equal(d_logp, lp.grad) and torch.equal(d_pred, p.grad)
    assert int(cnt) == 0


def test_step_loss_total_rounds_like_three_elementwise_kernels():
    """total = fl(fl(w_r*recon) + fl(w_s*sex)) + 0.0f over 300 value pairs: a multiply contracted into the add
    (one rounding less) differs from ATen's three kernels in about one pair in four"""
    from speech_anonymization_amd import ops
    g = torch.Generator().manual_seed(3)
    label = torch.tensor([0, 1], device=DEV)
    outs = []
    for _ in range(300):
        pred, target = torch.randn(2, 8, generator=g).to(DEV), torch.randn(2, 8, generator=g).to(DEV)
        logp = torch.log_softmax(3 * torch.randn(2, 2, generator=g), dim=1).to(DEV)
        outs.append(ops.step_loss(pred, target, "l1", logp, label, 0.1, 0.9)[0])
    out = torch.stack(outs)
    assert torch.equal(out[:, 2], 0.1 * out[:, 0] + 0.9 * out[:, 1] + 0.0)
    assert out[:, 0].unique().numel() > 250 and out[:, 1].unique().numel() > 250


def test_step_loss_counts_a_nonfinite_total():
    from speech_anonymization_amd import ops
    pred, target = torch.zeros(2, 64, device=DEV), torch.ones(2, 64, device=DEV)
    logp = torch.tensor([[-0.5, -1.0], [float("-inf"), -0.1]], device=DEV)
    label = torch.tensor([0, 0], device=DEV)
    cnt = torch.full((), 3, dtype=torch.int32, device=DEV)
    for expect in (4, 5):
        out, _, _ = ops.step_loss(pred, target, "l1", logp, label, 0.1, 0.9, nonfinite=cnt)
        assert float(out[2]) == float("inf") and int(cnt) == expect
    out, _, _ = ops.step_loss(pred, target, "l1", logp, label, 0.1, 0.9)      # no counter: nothing else changes
    assert float(out[0]) == 1.0 and int(cnt) == 5


@pytest.mark.parametrize("mode", ["raw", "given", "none"])
@pytest.mark.parametrize("Ln", [200, 1000, 1152])
@pytest.mark.parametrize("Bn", [1, 3])
def test_pool_finaliser_in_the_gather_launch(Bn, Ln, mode):
    """sa_pool_gather_fin against sa_pool_gather + sa_pool_fin (+ the three ATen steps that normalise a drawn
    noise): lengths that are no multiple of 128, and fewer 128-row groups than segments (L = 200)"""
    from speech_anonymization_amd import ops
    g = torch.Generator().manual_seed(Ln + Bn)
    r = torch.randn(Bn, Ln, 128, generator=g).abs().to(DEV)
    sc = (1 + 0.1 * torch.randn(128, generator=g)).to(DEV)
    sh = (0.1 * torch.randn(128, generator=g)).to(DEV)
    if mode == "raw":
        torch.manual_seed(99)
        old = ops.pool_fwd(r, sc, sh, noise=ops.pooling_noise(True, Bn, 128, r.device))
        torch.manual_seed(99)
        nz, raw = ops.pooling_noise_raw(True, Bn, 128, r.device)
        assert raw
        new = ops.pool_fwd(r, sc, sh, noise=nz, fused=True, raw=True)
    else:
        setting = torch.rand(Bn, 128, generator=g) if mode == "given" else None
        old = ops.pool_fwd(r, sc, sh, noise=ops.pooling_noise(setting, Bn, 128, r.device))
        nz, raw = ops.pooling_noise_raw(setting, Bn, 128, r.device)
        assert not raw and (nz is None) == (mode == "none")
        new = ops.pool_fwd(r, sc, sh, noise=nz, fused=True, raw=raw)
    torch.cuda.synchronize()
    for name, a, b in zip(("pooled", "mean", "stdraw"), old, new):
        assert torch.equal(a, b), name
    if mode != "none":                                           # (the noise reached the pooled mean)
        assert not torch.equal(new[0][:, :128], new[1])


def _head_case(M):
    from speech_anonymization_amd import ops
    g = torch.Generator().manual_seed(100 + M)
    cls = torch.nn.Sequential(torch.nn.Linear(256, 128), torch.nn.ReLU(), torch.nn.BatchNorm1d(128),
                              torch.nn.Linear(128, 64), torch.nn.ReLU(), torch.nn.BatchNorm1d(64),
                              torch.nn.Linear(64, 2))
    with torch.no_grad():
        for p_ in cls.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * (0.3 if p_.dim() == 1 else p_.shape[1] ** -0.5))
        cls[2].weight.add_(1.0); cls[5].weight.add_(1.0)
    P = {k: v.detach().to(DEV).contiguous() for k, v in cls.state_dict().items()
         if v.dtype.is_floating_point and "running" not in k}
    pooled = torch.randn(M, 256, generator=g).to(DEV)
    dlogp = (torch.randn(M, 2, generator=g) / M).to(DEV)
    fwd = ops.head_fwd(pooled, P, copy.deepcopy(cls[2]).to(DEV), copy.deepcopy(cls[5]).to(DEV))
    return P, pooled, dlogp, fwd


@pytest.mark.parametrize("frozen", [(), ("0.weight", "2.bias", "3.weight", "5.weight", "6.bias"),
                                    ("0.bias", "2.weight", "3.bias", "5.bias", "6.weight")])
@pytest.mark.parametrize("M", [1, 2, 10, 32, 64])
def test_wide_head_backward_equals_one_workgroup(M, frozen):
    """sa_head_bwd_wide against sa_head_bwd: d pooled and the ten parameter gradients; `frozen` gradients are
    NULL pointers (their buffers must stay untouched)"""
    from speech_anonymization_amd import ops
    assert ops.head_max_rows() == 64
    P, pooled, dlogp, (H1, f1, H2, f2, logp) = _head_case(M)
    res = []
    for wide in (False, True):
        grads = {k: torch.full_like(v, float("nan")) for k, v in P.items()}
        views = {k: v for k, v in grads.items() if k not in frozen}
        dpooled = ops.head_bwd(dlogp, logp, pooled, H1, f1, H2, f2, P, views, wide=wide)
        torch.cuda.synchronize()
        res.append((dpooled, grads))
    (dp0, g0), (dp1, g1) = res
    assert torch.equal(dp0, dp1) and bool(torch.isfinite(dp1).all())
    assert len(g0) == 10
    for k in g0:
        assert _eq(g0[k], g1[k]), k
        assert bool(torch.isnan(g1[k]).all()) if k in frozen else bool(torch.isfinite(g1[k]).all()), k
