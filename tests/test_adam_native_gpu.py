"""ops.adam_step / sa_adam_step (the arithmetic of torch.optim.Adam(fused=True).step() in one launch) against
torch's own step on cloned tensors: parameters, both moments and the step counters after every step, bit for bit
(compared as int32 so that NaNs and signed zeros count too)."""
import contextlib
import gc
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# around one thread's quad, one block's chunk (1 024) and torch's chunk (65 536)
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 65536 + 7]
STEPS = 30


@contextlib.contextmanager
def _capture(graph):
    """torch.cuda.graph with the garbage collected before it and no collection inside it: destructors of GPU objects
    in a dead cycle of an earlier test must not run while a capture is under way (Brain._fit_batch_graph does the same)"""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was_on:
            gc.enable()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _params(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.randn(n, generator=g) * 10.0 ** (i % 4 - 2)).to(dev)) for i, n in enumerate(SIZES)]
    ps.append(torch.nn.Parameter(torch.randn(17, generator=g).to(dev)))         # never gets a gradient
    return ps


def _grads(step, nonfinite=False):
    """per tensor: magnitudes spread over 1e-12 .. 1e3, both signs, exact zeros and a denormal"""
    g = torch.Generator().manual_seed(1000 + step)
    out = []
    for n in SIZES:
        mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 15.0 - 12.0)
        t = (mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float()
        t[torch.rand(n, generator=g) < 0.1] = 0.0
        if n >= 4:
            t[n // 2] = 1e-40                                                   # fp32 denormal
            t[n // 2 - 1] = -0.0
        if nonfinite and step >= 3 and n >= 5:
            t[1], t[n - 2] = float("nan"), float("inf")
        out.append(t)
    return out


def _set_grads(ps, grads, dev, flat):
    """flat: every gradient a view of one buffer, packed back to back (so most start off a 16-byte boundary); else
    a tensor of its own each.  The last parameter keeps grad None"""
    if flat:
        buf = torch.empty(sum(SIZES) + 1, device=dev)
        o = 1
        for p, g in zip(ps, grads):
            p.grad = buf[o:o + g.numel()].copy_(g)
            o += g.numel()
        return [buf]
    for p, g in zip(ps, grads):
        p.grad = g.to(dev)
    return None


def _optim(ps, lr_mode, dev, **kw):
    if lr_mode == "device":                 # what Brain.init_optimizers builds in hipGraph mode
        opt = torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, fused=True, capturable=True, **kw)
        for g in opt.param_groups:
            g["lr"] = torch.tensor(1e-3, dtype=torch.float32, device=dev)
    else:
        opt = torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, fused=True, **kw)
    return opt


def _set_lr(opt, s):
    """Noam-like: a new rate every step, not representable in fp32"""
    lr = 768 ** -0.5 * min((s + 1) ** -0.5, (s + 1) * 25000 ** -1.5) * (1000.0 if s % 2 else 1.0) + 1e-3 / (s + 3)
    for g in opt.param_groups:
        if torch.is_tensor(g["lr"]):
            g["lr"].fill_(lr)
        else:
            g["lr"] = lr


def _compare(pa, oa, pb, ob, tag):
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert _same(a, b), (tag, "param", i)
        sa, sb = oa.state.get(a, {}), ob.state.get(b, {})
        assert sorted(sa) == sorted(sb), (tag, "state keys", i)
        for k in sa:
            assert _same(sa[k], sb[k]), (tag, k, i, sa[k].flatten()[:4], sb[k].flatten()[:4])


@pytest.mark.parametrize("case", ["host-own", "host-flat", "device-own", "device-flat", "host-flat-nonfinite"])
def test_native_adam_equals_torch_fused_adam(case):
    from speech_anonymization_amd import ops
    lr_mode, flat, nonfinite = case.split("-")[0], "flat" in case, "nonfinite" in case
    dev = torch.device("cuda:0")
    ref_p, nat_p = _params(dev), _params(dev)
    ref, nat = _optim(ref_p, lr_mode, dev), _optim(nat_p, lr_mode, dev)
    native_steps = 0
    for s in range(STEPS):
        grads = _grads(s, nonfinite)
        _set_grads(ref_p, grads, dev, flat)
        flats = _set_grads(nat_p, grads, dev, flat)
        _set_lr(ref, s)
        _set_lr(nat, s)
        if s == 1:                  # one tensor far into its run: bias corrections near 1
            for ps, o in ((ref_p, ref), (nat_p, nat)):
                o.state[ps[5]]["step"].fill_(25000.0)
        ref.step()
        if ops.adam_step(nat, flats):
            native_steps += 1
        else:
            assert s == 0, "only the first step (no optimizer state yet) is torch's"
            nat.step()
        _compare(ref_p, ref, nat_p, nat, (case, s))
        assert nat_p[-1].grad is None and not nat.state.get(nat_p[-1])
    assert native_steps == STEPS - 1
    assert float(nat.state[nat_p[5]]["step"]) == 25000.0 + STEPS - 1 and float(nat.state[nat_p[0]]["step"]) == STEPS


def test_native_adam_table_follows_the_buckets():
    """gradients that are views of a bucket are recorded as (bucket, offset): a bucket at a new address reuses the
    cached device table, a gradient outside the bucket rebuilds it -- same bits either way"""
    from speech_anonymization_amd import ops
    dev = torch.device("cuda:0")
    ref_p, nat_p = _params(dev), _params(dev)
    ref, nat = _optim(ref_p, "host", dev), _optim(nat_p, "host", dev)
    tables, keep = [], []
    for s in range(5):
        grads = _grads(s)
        _set_grads(ref_p, grads, dev, True)
        flats = _set_grads(nat_p, grads, dev, s != 3)       # step 3: every gradient a tensor of its own
        keep.append(flats)                                  # (so that no two steps share a bucket address)
        ref.step()
        if not ops.adam_step(nat, flats):
            nat.step()
        else:
            tables.append(nat._sa_adam_tables[0][1])
        _compare(ref_p, ref, nat_p, nat, s)
    assert len({f[0].data_ptr() for f in keep if f}) == 4
    assert tables[0] is tables[1] and tables[2] is not tables[1] and tables[3] is not tables[2]


def test_native_adam_captured_table_outlives_a_rebuild():
    """a captured launch reads its device table on every replay: an eager step in between that rebuilds the table
    (gradients elsewhere) must leave the captured one alive, and a rebuild needed DURING a capture is torch's step"""
    from speech_anonymization_amd import ops
    dev = torch.device("cuda:0")
    ref_p, nat_p = _params(dev), _params(dev)
    ref, nat = _optim(ref_p, "device", dev), _optim(nat_p, "device", dev)

    def load(buf, grads):
        o = 1
        for g in grads:
            buf[o:o + g.numel()].copy_(g)
            o += g.numel()

    def ref_step(s):
        _set_grads(ref_p, _grads(s), dev, False)
        _set_lr(ref, s)
        ref.step()

    static = _set_grads(nat_p, _grads(0), dev, True)[0]         # the replayed step's gradient bucket
    views = [p.grad for p in nat_p]
    _set_lr(nat, 0)
    nat.step()
    ref_step(0)
    load(static, _grads(1))
    _set_lr(nat, 1)
    assert ops.adam_step(nat, [static])                         # eager: builds the table
    ref_step(1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _capture(graph):
        assert ops.adam_step(nat, [static])
    table = nat._sa_adam_tables[0][1]
    assert any(e[1] is table for e in nat._sa_adam_captured)
    for s in (2, 3):
        load(static, _grads(s))
        _set_lr(nat, s)
        graph.replay()
        ref_step(s)
        _compare(ref_p, ref, nat_p, nat, ("replay", s))
        if s == 2:                                              # an eager step on gradients of their own: a rebuild
            _set_grads(nat_p, _grads(10), dev, False)
            assert ops.adam_step(nat, None) and nat._sa_adam_tables[0][1] is not table
            _set_grads(ref_p, _grads(10), dev, False)
            ref.step()
            _compare(ref_p, ref, nat_p, nat, "eager between replays")
            for p, v in zip(nat_p, views):
                p.grad = v
    other = torch.cuda.CUDAGraph()
    _set_grads(nat_p, _grads(11), dev, False)                   # a layout no table describes, met while capturing
    x = torch.zeros(4, device=dev)
    with _capture(other):
        x.add_(1.0)
        assert ops.adam_step(nat, None) is False


@pytest.mark.parametrize("kw", [dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True)],
                         ids=["weight_decay", "amsgrad", "maximize"])
def test_native_adam_leaves_other_configurations_to_torch(kw):
    from speech_anonymization_amd import ops
    dev = torch.device("cuda:0")
    ref_p, nat_p = _params(dev), _params(dev)
    ref, nat = _optim(ref_p, "host", dev, **kw), _optim(nat_p, "host", dev, **kw)
    for s in range(3):
        grads = _grads(s)
        _set_grads(ref_p, grads, dev, False)
        _set_grads(nat_p, grads, dev, False)
        before = [p.detach().clone() for p in nat_p]
        assert ops.adam_step(nat, None) is False
        assert all(_same(a, b) for a, b in zip(before, nat_p)), "a refused step must not touch anything"
        if s:
            assert float(nat.state[nat_p[0]]["step"]) == s
        ref.step()
        nat.step()
        _compare(ref_p, ref, nat_p, nat, s)
    assert any(not _same(a, b) for a, b in zip(_params(dev), nat_p))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipGraph"])
def test_fit_batch_native_adam_equals_torch_adam(graph, monkeypatch):
    """the ConvAE train step at B = 2, T = 36 with native_adam off and on: every parameter, buffer and optimizer
    state tensor equal after every step; the native launch ran in every step but the first"""
    from oracle.convae import numpy_params
    from tests import smoke_step
    from speech_anonymization_amd import ops
    from speech_anonymization_amd.brain import Batch
    dev = torch.device("cuda:0")
    wav = smoke_step.make_wave(2, 5600)
    batches = [Batch(wav * s, torch.tensor([1.0, 0.83]), torch.arange(2) % 2) for s in (1.0, 0.9, 0.8, 1.1, 0.7, 1.05)]
    batches = batches if graph else batches[:4]
    took = []
    real = ops.adam_step
    monkeypatch.setattr(ops, "adam_step", lambda *a, **k: took.append(real(*a, **k)) or took[-1])
    brains = [smoke_step.build("bf16x3", dev, numpy_params(8886), run_opts=dict(native_adam=on, hip_graph=graph))
              for on in (False, True)]
    assert [b.native_adam for b in brains] == [False, True]
    for i, b in enumerate(batches):
        for br in brains:
            torch.manual_seed(1234)
            br.step += 1
            br.fit_batch(b)
        torch.cuda.synchronize()
        m0, m1 = (br.modules["ConvAE"].state_dict() for br in brains)
        for k in m0:
            assert torch.equal(m0[k], m1[k]), (i, k)
        s0, s1 = (br.optimizer.state_dict()["state"] for br in brains)
        assert sorted(s0) == sorted(s1) and len(s0) == 56
        for j in s0:
            for k in s0[j]:
                assert _same(s0[j][k], s1[j][k]), (i, j, k)
    if graph:
        assert all("graph" in e for br in brains for e in br._graphs.values())
    assert took == [False, True, True, True]        # eager: four steps; hipGraph: three warm-ups, then the capture
    assert math.isfinite(float(brains[1].optimizer.state_dict()["state"][0]["exp_avg"].sum()))
