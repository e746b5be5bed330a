"""model_type fcae on the GPU (csrc/sa_fcae.hip, speech_anonymization_amd/fcae.py) against the plain-torch
restatement tests/fcae_ref.py in fp64, the two reference fixtures, fp64 formulas per launch, and through the
entry script.  Pooling noise is off or injected everywhere.  Every figure is printed before it is asserted."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fcae_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# the two gradients that are mathematically zero (a bias directly in front of a BatchNorm): fp64 leaves ~1e-14,
# fp32 rounding noise of the size of 1e-5 of the layer's weight gradient; a rel-MSE on them is meaningless, so
# they are checked by magnitude.  No other tensor is exempt.
ZERO_GRADS = {"sex_classifier.classify.0.bias": "sex_classifier.classify.0.weight",
              "sex_classifier.classify.5.bias": "sex_classifier.classify.5.weight"}
MARGIN, FLOOR = 30.0, 1e-10          # 30x the reference's own fp32-vs-fp64 noise; fp32 per-kernel bar
KERNEL_BAR = 1e-10
DEV = "cuda:0"


def _models(B, seed, noise=False, state=None):
    from speech_anonymization_amd import fcae
    torch.manual_seed(seed)
    ref = R.FullyConnectedAutoencoder(80, B)
    if state is not None:
        ref.load_state_dict(state)
    hip = fcae.FullyConnectedAutoencoder(80, B, pooling_noise=noise)
    hip.load_state_dict(ref.state_dict())
    return ref, hip.to(DEV)


def _hip_step(hip, feats, gender, train=True, w=(0.5, 0.5)):
    hip.train(train)
    hip.zero_grad(set_to_none=True)
    x, g = feats.to(DEV), gender.to(DEV)
    with torch.set_grad_enabled(train):
        recon, logp = hip(x)
        loss = R.loss_fn(recon, logp, x, g, *w)
    grads = {}
    if train:
        loss.backward()
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in hip.named_parameters()}
    torch.cuda.synchronize()
    return dict(recon=recon.detach(), logp=logp.detach(), loss=loss.detach(), grads=grads,
                buffers={k: v.detach().clone() for k, v in hip.named_buffers()})


def _check(tag, got, r32, r64, failures):
    """got against the fp64 restatement, bar max(30 * n32, 1e-10) with n32 = rel-MSE(restatement fp32, fp64)"""
    n32 = R.relmse(r32, r64)
    e = R.relmse(got, r64)
    bar = max(MARGIN * n32, FLOOR)
    print(f"  {tag:48s} hip {e:.2e}  n32 {n32:.2e}  bar {bar:.2e}")
    if not e <= bar:
        failures.append((tag, e, bar))


def _check_zero_grad(tag, g_hip, g32, gw32, failures):
    m, bar = float(g_hip.abs().max()), MARGIN * max(float(g32.abs().max()), 1e-7 * float(gw32.abs().max()))
    print(f"  {tag:48s} max|g_hip| {m:.2e}  bar {bar:.2e}  (mathematically zero)")
    if not m <= bar:
        failures.append((tag, m, bar))


def _compare_run(h, r32, r64, train, failures, tag=""):
    for k in ("recon", "logp") + (("loss",) if train else ()):
        _check(tag + k, h[k], r32[k], r64[k], failures)
    if not train:
        return
    assert len(h["grads"]) == 30
    n = 0
    for k in r64["grads"]:
        if k in ZERO_GRADS:
            _check_zero_grad(tag + "grad " + k, h["grads"][k], r32["grads"][k], r32["grads"][ZERO_GRADS[k]], failures)
        else:
            _check(tag + "grad " + k, h["grads"][k], r32["grads"][k], r64["grads"][k], failures)
            n += 1
    assert n == 28
    stats = [k for k in r64["buffers"] if "running" in k]
    assert len(stats) == 6
    for k in stats:
        _check(tag + k, h["buffers"][k], r32["buffers"][k], r64["buffers"][k], failures)
    for k in r64["buffers"]:
        if "num_batches" in k:
            assert int(h["buffers"][k]) == int(r64["buffers"][k]) == 1


@pytest.mark.parametrize("B,T", [(3, 100), (4, 211), (10, 1008), (32, 1008)])
def test_whole_model_against_fp64_restatement(B, T):
    ref, hip = _models(B, B * 1000 + T)
    feats, gender = torch.randn(B, T, 80), torch.arange(B) % 2
    failures = []
    for train in (True, False):
        print(f"B={B} T={T} train={train}")
        r32 = R.run_step(copy.deepcopy(ref), feats, gender, train)
        r64 = R.run_step(copy.deepcopy(ref).double(), feats.double(), gender, train)
        if not train:                                   # eval runs on the initial running statistics, like the restatement
            hip.load_state_dict(ref.state_dict())
        h = _hip_step(hip, feats, gender, train)
        _compare_run(h, r32, r64, train, failures)
    assert not failures, failures


def _sub(t, n=2048):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n]


def test_fixture_S_train_step():
    """the reference class's own fp32 step (tests/golden/fcae_S.npz): HIP against the fixture's values, bar
    max(30 * n32, 1e-10) with n32 = rel-MSE(fixture, fp64 restatement)"""
    z = np.load(os.path.join(GOLD, "fcae_S.npz"))
    state = {k[len("init/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init/")}
    ref, hip = _models(3, 0, state=state)
    feats, gender = torch.from_numpy(z["feats"]), torch.from_numpy(z["gender"])
    r64 = R.run_step(copy.deepcopy(ref).double(), feats.double(), gender, True)
    h = _hip_step(hip, feats, gender, True)
    failures = []

    def chk(tag, got, fix, r):
        n32 = R.relmse(fix, r)
        e, bar = R.relmse(got, fix), max(MARGIN * n32, FLOOR)
        print(f"  {tag:48s} hip-vs-fixture {e:.2e}  n32 {n32:.2e}  bar {bar:.2e}")
        if not e <= bar:
            failures.append((tag, e, bar))
    for k in ("recon", "logp", "loss"):
        chk(k, h[k], torch.from_numpy(z[k]), r64[k])
    for k in r64["grads"]:
        fix = torch.from_numpy(z["grad_sub/" + k])
        if k in ZERO_GRADS:
            _check_zero_grad("grad " + k, h["grads"][k], fix, torch.from_numpy(z["grad_sub/" + ZERO_GRADS[k]]), failures)
        else:
            chk("grad " + k, _sub(h["grads"][k].cpu()), fix, _sub(r64["grads"][k]))
    for k in r64["buffers"]:
        if "running" in k:
            chk(k, h["buffers"][k], torch.from_numpy(z["buffer/" + k]), r64["buffers"][k])
    assert not failures, failures


def test_fixture_trained_checkpoint_eval():
    """the reference's trained weights (results/5_5_fc) through load_state_dict with the ModuleList prefix; eval
    outputs against the reference class's own fp32 outputs"""
    from speech_anonymization_amd import fcae
    z = np.load(os.path.join(GOLD, "fcae_trained.npz"))
    ck = {k[len("ckpt/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("ckpt/")}
    hip = fcae.FullyConnectedAutoencoder(80, 3, pooling_noise=False)
    torch.nn.ModuleList([hip]).load_state_dict(ck, strict=True)
    hip = hip.to(DEV).eval()
    ref = R.FullyConnectedAutoencoder(80, 3)
    ref.load_state_dict({k[2:]: v for k, v in ck.items()})
    feats = torch.from_numpy(z["feats"])
    ref = ref.double().eval()
    with torch.no_grad():
        r64 = ref(feats.double())
        recon, logp = hip(feats.to(DEV))
    assert not recon.requires_grad and recon.grad_fn is None
    failures = []
    for k, got, r in (("recon", recon, r64[0]), ("logp", logp, r64[1])):
        fix = torch.from_numpy(z["eval_" + k])
        n32 = R.relmse(fix, r)
        e, bar = R.relmse(got, fix), max(MARGIN * n32, FLOOR)
        print(f"  {k:8s} hip-vs-fixture {e:.2e}  n32 {n32:.2e}  bar {bar:.2e}")
        if not e <= bar:
            failures.append((k, e, bar))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------
# per launch, against fp64 formulas (inputs of each launch are the GPU tensors it was given, in fp64)
# ---------------------------------------------------------------------------------------------------
# (5, 2): T = 2, B*T below one tile.  (3, 100): ends mid-tile, channel boundaries at multiples of 5 frames.
# (4, 211): T not a multiple of 20 (channel boundaries inside frames), 3 full tiles + 19 frames.  (4, 128): whole tiles.
KERNEL_SHAPES = [(5, 2), (3, 100), (4, 211), (4, 128)]


def _k(tag, got, want, failures, bar=KERNEL_BAR):
    e = R.relmse(got, want)
    print(f"  {tag:40s} {e:.2e}")
    if not e <= bar:
        failures.append((tag, e))


def _d(t):
    return t.detach().double().cpu()


def _lin(x, w, b):
    return x @ _d(w).T + _d(b)


def _bn_channels(z, T):
    """[B, T, 20] -> [B, 20, T] as the reference reshapes it (a reinterpretation)"""
    return z.reshape(z.shape[0], 20, T)


@pytest.mark.parametrize("B,T", KERNEL_SHAPES)
def test_forward_launches(B, T):
    from speech_anonymization_amd import fcae
    ref, hip = _models(B, 7 * B + T)
    P = dict(hip.named_parameters())
    cls = hip.sex_classifier
    feats = (torch.randn(B, T, 80) * 1.5 + 0.2).to(DEV)
    wb = fcae.frame_table(P)
    failures = []
    with torch.no_grad():
        h1, h2, z, bnpart = fcae.enc_fwd(feats, wb)
        x = _d(feats)
        e1 = F.relu(_lin(x, P["encoder.0.weight"], P["encoder.0.bias"]))
        e2 = F.relu(_lin(_d(h1), P["encoder.2.weight"], P["encoder.2.bias"]))
        e3 = _lin(_d(h2), P["encoder.4.weight"], P["encoder.4.bias"])
        _k("enc_fwd h1", h1, e1, failures); _k("enc_fwd h2", h2, e2, failures); _k("enc_fwd z", z, e3, failures)
        # channel-map statistics
        zc = _bn_channels(_d(z), T)
        mean, var = zc.mean(dim=(0, 2)), zc.var(dim=(0, 2), unbiased=False)
        rm0, rv0 = _d(cls.norm.running_mean), _d(cls.norm.running_var)
        bnf = fcae.bn_fin(bnpart, P["sex_classifier.norm.weight"], P["sex_classifier.norm.bias"], cls.norm.running_mean,
                          cls.norm.running_var, B, T, True)
        _k("bn_fin mean", bnf[0], mean, failures)
        _k("bn_fin rstd", bnf[1], 1 / torch.sqrt(var + 1e-5), failures)
        n = B * T
        _k("bn_fin running_mean", cls.norm.running_mean, 0.9 * rm0 + 0.1 * mean, failures)
        _k("bn_fin running_var", cls.norm.running_var, 0.9 * rv0 + 0.1 * var * n / (n - 1), failures)
        g, b_ = _d(P["sex_classifier.norm.weight"]), _d(P["sex_classifier.norm.bias"])
        _k("bn_fin scale", bnf[2], g * _d(bnf[1]), failures)
        _k("bn_fin shift", bnf[3], b_ - _d(bnf[0]) * _d(bnf[2]), failures)
        bnf_eval = fcae.bn_fin(None, P["sex_classifier.norm.weight"], P["sex_classifier.norm.bias"], cls.norm.running_mean,
                               cls.norm.running_var, B, T, False)
        _k("bn_fin eval mean", bnf_eval[0], _d(cls.norm.running_mean), failures)
        _k("bn_fin eval rstd", bnf_eval[1], 1 / torch.sqrt(_d(cls.norm.running_var) + 1e-5), failures)
        # one pass over z
        a1, u, d1, d2, recon, poolpart = fcae.mid_fwd(z, bnf, wb)
        zd = _d(z)
        zn = (_bn_channels(zd, T) * _d(bnf[2])[None, :, None] + _d(bnf[3])[None, :, None]).reshape(B, T, 20)
        _k("mid_fwd a1", a1, F.relu(_lin(zn, P["sex_classifier.initial.0.weight"], P["sex_classifier.initial.0.bias"])), failures)
        _k("mid_fwd u", u, F.relu(_lin(_d(a1), P["sex_classifier.initial.2.weight"], P["sex_classifier.initial.2.bias"])), failures)
        _k("mid_fwd d1", d1, F.relu(_lin(zd, P["decoder.0.weight"], P["decoder.0.bias"])), failures)
        _k("mid_fwd d2", d2, F.relu(_lin(_d(d1), P["decoder.2.weight"], P["decoder.2.bias"])), failures)
        _k("mid_fwd recon", recon, _lin(_d(d2), P["decoder.4.weight"], P["decoder.4.bias"]), failures)
        ud = _d(u)
        _k("mid_fwd pool sums", poolpart.reshape(B, -1, 2, 40).sum(1)[:, 0], ud.sum(1), failures)
        _k("mid_fwd pool squares", poolpart.reshape(B, -1, 2, 40).sum(1)[:, 1], (ud * ud).sum(1), failures)
        # the head, train and eval mode, with an injected noise draw
        noise = torch.rand(B, 40, device=DEV)
        for train in (True, False):
            H = {k[len("sex_classifier.classify."):]: v for k, v in hip.state_dict().items() if "classify." in k}
            before = {k: _d(v) for k, v in H.items()}
            o = fcae.head_fwd(poolpart, noise, fcae.head_table(H), B, T, train)
            pooled = torch.cat((ud.mean(1) + 1e-5 * ((1 - 9) * _d(noise) + 9), ud.std(1) + 1e-5), 1)
            _k(f"head_fwd[{train}] pooled", o["pooled"], pooled, failures)
            _k(f"head_fwd[{train}] pst", o["pst"], torch.cat((ud.mean(1), ud.std(1)), 1), failures)
            hh1 = _lin(_d(o["pooled"]), H["0.weight"], H["0.bias"])
            _k(f"head_fwd[{train}] h1", o["h1"], hh1, failures)

            def bn(h, i):
                if train:
                    mu, var = h.mean(0), h.var(0, unbiased=False)
                else:
                    mu, var = before[f"{i}.running_mean"], before[f"{i}.running_var"]
                return (h - mu) / torch.sqrt(var + 1e-5) * before[f"{i}.weight"] + before[f"{i}.bias"], mu, var
            y1, mu1, var1 = bn(_d(o["h1"]), 1)
            _k(f"head_fwd[{train}] f1 mean", o["f1"][0], mu1, failures)
            _k(f"head_fwd[{train}] f1 rstd", o["f1"][1], 1 / torch.sqrt(var1 + 1e-5), failures)
            hh2 = F.relu(_lin(F.relu(y1), H["3.weight"], H["3.bias"]))
            _k(f"head_fwd[{train}] h2", o["h2"], hh2, failures)
            _k(f"head_fwd[{train}] h3", o["h3"], _lin(_d(o["h2"]), H["5.weight"], H["5.bias"]), failures)
            y2, mu2, var2 = bn(_d(o["h3"]), 6)
            _k(f"head_fwd[{train}] f2 mean", o["f2"][0], mu2, failures)
            _k(f"head_fwd[{train}] logp", o["logp"], F.log_softmax(_lin(y2, H["7.weight"], H["7.bias"]), 1), failures)
            if train:
                _k("head_fwd running_mean 1", H["1.running_mean"], 0.9 * before["1.running_mean"] + 0.1 * mu1, failures)
                _k("head_fwd running_var 6", H["6.running_var"],
                   0.9 * before["6.running_var"] + 0.1 * var2 * B / (B - 1), failures)
    torch.cuda.synchronize()
    assert not failures, failures


@pytest.mark.parametrize("B,T", KERNEL_SHAPES)
def test_backward_launches(B, T):
    """every data gradient and every weight / bias gradient (after the reducer) of the five backward launches,
    each against fp64 autograd of the same sub-graph fed the launch's own inputs"""
    from speech_anonymization_amd import fcae
    ref, hip = _models(B, 11 * B + T)
    P = {k: v.detach() for k, v in hip.named_parameters()}
    cls = hip.sex_classifier
    feats = (torch.randn(B, T, 80) * 1.5 + 0.2).to(DEV)
    wb = fcae.frame_table(P)
    H = {k[len("sex_classifier.classify."):]: v for k, v in hip.state_dict().items() if "classify." in k}
    hw = fcae.head_table(H)
    failures = []
    with torch.no_grad():
        h1, h2, z, bnpart = fcae.enc_fwd(feats, wb)
        bnf = fcae.bn_fin(bnpart, P["sex_classifier.norm.weight"], P["sex_classifier.norm.bias"], cls.norm.running_mean,
                          cls.norm.running_var, B, T, True)
        a1, u, d1, d2, recon, poolpart = fcae.mid_fwd(z, bnf, wb)
        o = fcae.head_fwd(poolpart, None, hw, B, T, True)
        dlogp = torch.randn(B, 2, device=DEV)
        d_recon = torch.randn(B, T, 80, device=DEV) / (B * T)
        dhead, dpooled = fcae.head_bwd(dlogp, o, hw, True)
        dzn, dzdec, wpart, bnbpart = fcae.mid_bwd(d_recon, dpooled, o["pst"], z, bnf, a1, u, d1, d2, wb)
        coef, dgamma, dbeta = fcae.bn_bwd_fin(bnbpart, P["sex_classifier.norm.weight"], bnf, B, T, True)
        fcae.enc_bwd(feats, h1, h2, z, dzn, dzdec, coef, wb, wpart)
        G = fcae.split_frame_grads(fcae.wreduce(wpart))
        GH = fcae.split_head_grads(dhead)
    torch.cuda.synchronize()

    def leaf(t):
        return _d(t).requires_grad_(True)

    def mrelu(x, act):
        """ReLU with the mask of the activation the forward launch stored (a pre-activation within rounding of
        zero may have the other sign in fp64)"""
        return x * (_d(act) > 0)

    # ---- head_bwd: classify + log_softmax.  The launch's inputs are pooled and the STORED h1, h2, h3, so the fp64
    # formulas start from those (a BatchNorm over 3 near-identical rows amplifies the fp32 rounding of its stored
    # input a few hundred times; that is the model's conditioning, which the whole-model bars measure as n32).  The
    # same graph in fp32 gives the rounding noise of the two mathematically zero bias gradients. ----
    def head_graph(dtype):
        c = lambda t: _d(t).to(dtype)
        hp = {k: c(v).requires_grad_(True) for k, v in H.items() if "running" not in k and "num_batches" not in k}
        h3s = c(o["h3"]).requires_grad_(True)
        t3 = F.batch_norm(h3s, None, None, hp["6.weight"], hp["6.bias"], True, 0.1, 1e-5)
        F.log_softmax(F.linear(t3, hp["7.weight"], hp["7.bias"]), 1).backward(c(dlogp))
        h1s = c(o["h1"]).requires_grad_(True)
        t1 = F.relu(F.batch_norm(h1s, None, None, hp["1.weight"], hp["1.bias"], True, 0.1, 1e-5))
        t2 = F.linear(t1, hp["3.weight"], hp["3.bias"]) * (c(o["h2"]) > 0)
        F.linear(t2, hp["5.weight"], hp["5.bias"]).backward(h3s.grad)
        pooled = c(o["pooled"]).requires_grad_(True)
        F.linear(pooled, hp["0.weight"], hp["0.bias"]).backward(h1s.grad)
        return hp, pooled
    hp, pooled = head_graph(torch.float64)
    hp32, _ = head_graph(torch.float32)
    _k("head_bwd dpooled", dpooled, pooled.grad, failures)
    for k in hp:
        if k in ("0.bias", "5.bias"):                   # mathematically zero (ZERO_GRADS): by magnitude
            _check_zero_grad("head_bwd d " + k, GH[k], hp32[k].grad, hp32[k.replace("bias", "weight")].grad, failures)
        else:
            _k("head_bwd d " + k, GH[k], hp[k].grad, failures)

    # ---- mid_bwd, decoder: d recon -> d z, decoder.* gradients ----
    dp = {k: leaf(P[k]) for k in P if k.startswith("decoder.")}
    zl = leaf(z)
    r = F.linear(mrelu(F.linear(mrelu(F.linear(zl, dp["decoder.0.weight"], dp["decoder.0.bias"]), d1),
                                dp["decoder.2.weight"], dp["decoder.2.bias"]), d2), dp["decoder.4.weight"], dp["decoder.4.bias"])
    r.backward(_d(d_recon))
    _k("mid_bwd dzdec", dzdec, zl.grad, failures)
    for k in dp:
        _k("wreduce d " + k, G[k], dp[k].grad, failures)

    # ---- mid_bwd, classifier: d pooled -> pooling backward -> initial -> d zn; initial.* gradients ----
    ip = {k: leaf(P[k]) for k in P if ".initial." in k}
    znl = leaf((_bn_channels(_d(z), T) * _d(bnf[2])[None, :, None] + _d(bnf[3])[None, :, None]).reshape(B, T, 20))
    uu = mrelu(F.linear(mrelu(F.linear(znl, ip["sex_classifier.initial.0.weight"], ip["sex_classifier.initial.0.bias"]), a1),
                        ip["sex_classifier.initial.2.weight"], ip["sex_classifier.initial.2.bias"]), u)
    pl = torch.cat((uu.mean(1), uu.std(1) + 1e-5), 1)
    pl.backward(_d(dpooled))
    _k("mid_bwd dzn (pooling + initial)", dzn, znl.grad, failures)
    for k in ip:
        _k("wreduce d " + k, G[k], ip[k].grad, failures)
    # pooling backward alone: d u
    ul = leaf(u)
    torch.cat((ul.mean(1), ul.std(1) + 1e-5), 1).backward(_d(dpooled))
    # (checked through d initial.2.bias = sum over frames of d u masked by u > 0, and d zn above)
    _k("pooling bwd via d initial.2.bias", G["sex_classifier.initial.2.bias"], (ul.grad * (_d(u) > 0)).sum((0, 1)), failures)

    # ---- bn_bwd_fin: BatchNorm(20) backward by the channel map with GradReverse ----
    gam, bet = leaf(P["sex_classifier.norm.weight"]), leaf(P["sex_classifier.norm.bias"])
    zl2 = leaf(z)
    y = F.batch_norm(_bn_channels(R.GradReverse.apply(zl2), T), None, None, gam, bet, True, 0.1, 1e-5).reshape(B, T, 20)
    y.backward(_d(dzn))
    _k("bn_bwd_fin d norm.weight", dgamma, gam.grad, failures)
    _k("bn_bwd_fin d norm.bias", dbeta, bet.grad, failures)
    ch = (torch.arange(T * 20) // T).reshape(T, 20)
    c = _d(coef)
    dz_cls = c[0][ch] * _d(dzn) + c[1][ch] * _d(z) + c[2][ch]
    _k("bn_bwd_fin c1 dzn + c2 z + c3", dz_cls, zl2.grad, failures)

    # ---- enc_bwd: d z -> encoder.* gradients ----
    ep = {k: leaf(P[k]) for k in P if k.startswith("encoder.")}
    zz = F.linear(mrelu(F.linear(mrelu(F.linear(_d(feats), ep["encoder.0.weight"], ep["encoder.0.bias"]), h1),
                                 ep["encoder.2.weight"], ep["encoder.2.bias"]), h2), ep["encoder.4.weight"], ep["encoder.4.bias"])
    zz.backward(_d(dzdec) + dz_cls)
    for k in ep:
        _k("wreduce d " + k, G[k], ep[k].grad, failures)
    assert len(G) == 16 and len(GH) == 12
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------
# behaviour
# ---------------------------------------------------------------------------------------------------
def test_two_identical_steps_are_bit_identical():
    ref, hip = _models(4, 5)
    feats, gender = torch.randn(4, 211, 80), torch.arange(4) % 2
    a = _hip_step(hip, feats, gender)
    hip.load_state_dict(ref.state_dict())
    b = _hip_step(hip, feats, gender)
    for k in ("recon", "logp", "loss"):
        assert torch.equal(a[k], b[k]), k
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    for k in a["buffers"]:
        assert torch.equal(a["buffers"][k], b["buffers"][k]), k


def test_accumulated_backward_is_the_sum_of_the_single_ones():
    ref, hip = _models(3, 6)
    f1, f2, gender = torch.randn(3, 100, 80), torch.randn(3, 100, 80), torch.arange(3) % 2
    g1 = _hip_step(hip, f1, gender)["grads"]
    g2 = _hip_step(hip, f2, gender)["grads"]
    hip.zero_grad(set_to_none=True)
    for f in (f1, f2):
        x = f.to(DEV)
        recon, logp = hip(x)
        R.loss_fn(recon, logp, x, gender.to(DEV)).backward()
    for k, p in hip.named_parameters():
        assert torch.equal(p.grad, g1[k] + g2[k]), k


def test_frozen_classifier_gets_no_gradient_and_nothing_else_changes():
    ref, hip = _models(3, 8)
    feats, gender = torch.randn(3, 100, 80), torch.arange(3) % 2
    full = _hip_step(hip, feats, gender)["grads"]
    hip.load_state_dict(ref.state_dict())
    for k, p in hip.named_parameters():
        p.requires_grad = "sex_classifier" not in k
    part = _hip_step(hip, feats, gender)["grads"]
    for k in full:
        if "sex_classifier" in k:
            assert part[k] is None, k
        else:                                           # the adversarial gradient still reaches the encoder
            assert torch.equal(part[k], full[k]), k


def test_injected_pooling_noise_matches_the_restatement():
    B, T = 4, 211
    noise = torch.rand(B, 40)
    ref, hip = _models(B, 9, noise=noise)
    ref.sex_classifier.stats_pooling.noise = noise
    feats, gender = torch.randn(B, T, 80), torch.arange(B) % 2
    r32 = R.run_step(copy.deepcopy(ref), feats, gender, True)
    r64 = R.run_step(copy.deepcopy(ref).double(), feats.double(), gender, True)
    h = _hip_step(hip, feats, gender, True)
    failures = []
    _compare_run(h, r32, r64, True, failures)
    # and the offset is really applied: the noise-free model gives other log-probabilities
    _, plain = _models(B, 9, noise=False)
    assert not torch.equal(_hip_step(plain, feats, gender)["logp"], h["logp"])
    assert not failures, failures


def test_bad_inputs_raise():
    from speech_anonymization_amd import fcae
    from speech_anonymization_amd._lib import SaHipError
    _, hip = _models(3, 10)
    x = torch.randn(3, 50, 80, device=DEV)
    with pytest.raises(SaHipError, match="float32"):
        hip(x.double())
    with pytest.raises(SaHipError, match="float32"):
        hip(x.bfloat16())
    with pytest.raises(SaHipError, match="GPU"):
        hip(x.cpu())
    with pytest.raises(SaHipError, match="contiguous"):
        hip(torch.randn(3, 80, 50, device=DEV).transpose(1, 2))
    with pytest.raises(SaHipError):
        hip(torch.randn(3, 50, 40, device=DEV))
    with pytest.raises(SaHipError):
        hip(torch.randn(3, 1, 80, device=DEV))
    with pytest.raises(SaHipError, match="at most"):
        hip(torch.randn(fcae.max_rows() + 1, 4, 80, device=DEV))
    hip.eval()
    with torch.no_grad():
        recon, logp = hip(x)
    assert recon.shape == (3, 50, 80) and logp.shape == (3, 2) and recon.grad_fn is None


# ---------------------------------------------------------------------------------------------------
# through the entry script
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(1.0, 0.0), (0.5, 0.5)])
def test_entry_script_fcae(tmp_path, weights):
    """speechbrain_convae_train.py --model_type fcae on synthetic utterances, batch size 3: the loss weights of
    results/5_5_fc (recon 1.0) and recon 0.5 / sex 0.5; train_log.txt with the reference's columns, a falling train
    loss, the reference's checkpoint file set, and a second run that resumes from it."""
    import speechbrain_convae_train as entry
    cfg = os.path.join(ROOT, "speechbrain_configs", "convae.yaml")
    args = [cfg, "--device", "cuda:0", "--model_type", "fcae", "--folder", str(tmp_path), "--batch_size", "3",
            "--synthetic", "54", "--synthetic_samples", "16000", "--recon_loss_weight", str(weights[0]),
            "--sex_loss_weight", str(weights[1]), "--lr_adam", "100000.0"]
    # (Noam's rate is lr_adam * d_model^-0.5 * step * 25000^-1.5 during the warm-up, 9e-9 * step at the reference's
    # lr_adam = 1.0: thousands of steps before the logged three-digit loss moves.  lr_adam = 1e5 makes it
    # 9e-4 * step, so that the twelve steps of this test do.)
    entry.main(args + ["--number_of_epochs", "2"])
    out = tmp_path / "8886"
    lines = open(out / "train_log.txt").read().strip().splitlines()
    assert len(lines) == 2
    for i, ln in enumerate(lines):
        assert ln.startswith(f"epoch: {i + 1}, lr: ")
        for col in ("steps: ", "optimizer: Adam", "train loss: ", "valid loss: ", "valid ACC: "):
            assert col in ln, (col, ln)
    assert "steps: 6" in lines[0]                           # 18 batches / gradient_accumulation 3
    l1 = float(lines[0].split("train loss: ")[1].split(" ")[0])
    l2 = float(lines[1].split("train loss: ")[1].split(" ")[0])
    print("train loss", l1, "->", l2)
    assert l2 < l1
    ck = sorted(os.listdir(out / "save"))
    assert ck and ck[-1].startswith("CKPT+")
    assert {"model.ckpt", "normalizer.ckpt", "noam_scheduler.ckpt", "counter.ckpt", "CKPT.yaml", "optimizer.ckpt"} <= set(
        os.listdir(out / "save" / ck[-1]))
    sd = torch.load(out / "save" / ck[-1] / "model.ckpt", weights_only=True, map_location="cpu")
    z = np.load(os.path.join(GOLD, "fcae_trained.npz"))
    assert list(sd) == [k[len("ckpt/"):] for k in z.files if k.startswith("ckpt/")]
    # resume: a third epoch continues from the checkpoint
    entry.main(args + ["--number_of_epochs", "3"])
    lines = open(out / "train_log.txt").read().strip().splitlines()
    assert len(lines) == 3 and lines[2].startswith("epoch: 3, lr: ") and "steps: 18" in lines[2]


# ---------------------------------------------------------------------------------------------------
# learning check
# ---------------------------------------------------------------------------------------------------
def _train(model, data, dev, steps, lr=1e-3):
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    model.train()
    last = []
    for i in range(steps):
        x, g = data[i % len(data)]
        x, g = x.to(dev), g.to(dev)
        recon, logp = model(x)
        loss = R.loss_fn(recon, logp, x, g)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
        opt.step()
        if i >= steps - len(data):
            last.append(float(loss.detach()))
    return sum(last) / len(last)


def test_learning_matches_the_restatement_within_its_seed_spread():
    """60 Adam steps (lr 1e-3, clip 5) on the same 10 synthetic batches of 8 utterances, from the same initialisation:
    HIP on the GPU against torch on the restatement (CPU, fp32).  Free-running trajectories agree only to about
    the learning rate after Adam's first step, so the final train loss (mean over the last pass)
    is compared, and the allowed gap is the restatement's own spread over three initialisation seeds -- measured
    here, not fixed in advance (DESIGN section 10 records both numbers).
    The utterances of a batch differ in offset and scale.  With batches of 3 statistically identical utterances the
    classifier's BatchNorms see 3 nearly equal rows and training is chaotic: the restatement's own final loss then
    moves by 0.07 when its initial weights are perturbed by 1e-7 (relative), as much as between seeds, and the
    comparison would say nothing.  In this set-up the same perturbation moves it by less than 1e-3."""
    from speech_anonymization_amd import fcae
    torch.set_num_threads(1)
    B, T, steps = 8, 60, 60
    g = torch.Generator().manual_seed(123)
    data = []
    for _ in range(10):
        lab = torch.arange(B) % 2
        off = torch.randn(B, 1, 80, generator=g) * 0.5 + lab.view(B, 1, 1) * 0.8
        sc = 0.5 + torch.rand(B, 1, 80, generator=g)
        data.append((torch.randn(B, T, 80, generator=g) * sc + off, lab))
    finals = []
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        m = R.FullyConnectedAutoencoder(80, B)
        if seed == 0:
            init = copy.deepcopy(m.state_dict())
        finals.append(_train(m, data, "cpu", steps))
    spread = max(finals) - min(finals)
    hip = fcae.FullyConnectedAutoencoder(80, B, pooling_noise=False)
    hip.load_state_dict(init)
    got = _train(hip.to(DEV), data, DEV, steps)
    print(f"final train loss: restatement seeds 0,1,2 = {finals}, spread {spread:.4f}; HIP (seed 0) = {got:.4f}, "
          f"gap {abs(got - finals[0]):.5f}")
    assert abs(got - finals[0]) <= spread
