"""x-vector gender classifier in TRAIN mode (speech_anonymization_amd.xvector.train_log_probs,
sa_xvector.hip) against the CPU oracle (oracle/xvector.py in float64, torch autograd):
one whole train step, each TDNN kernel per layer shape, bit-reproducibility, and the recipe end to
end (gender_classifier_train.py --synthetic, then its checkpoint as the external classifier)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(80, 512, 5, 1), (512, 512, 3, 2), (512, 512, 3, 3), (512, 512, 1, 1), (512, 1500, 1, 1)]
IDS = ["80-512k5", "512-512k3d2", "512-512k3d3", "512-512k1", "512-1500k1"]


def rel_mse(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b) ** 2).sum() / (b ** 2).sum().clamp_min(1e-30))


def _models(B, seed=1230):
    """oracle (float64, train mode) and HIP pair with the same numpy-seeded weights and the same
    pooling-noise tensor."""
    from oracle import endtoend as OE, xvector as OX
    from speech_anonymization_amd import xvector as HX
    g = torch.Generator().manual_seed(seed + B)
    noise = torch.rand(B, 1500, generator=g)
    oxv, ocl = OX.Xvector(pooling_noise=noise), OX.Classifier()
    holder = OE.OracleEncoderClassifier(oxv, ocl)
    holder.load_state_dict(OE.numpy_params(holder, seed))
    oxv, ocl = oxv.double().train(), ocl.double().train()
    for p in list(oxv.parameters()) + list(ocl.parameters()):
        p.requires_grad_(True)
    hxv = HX.Xvector(pooling_noise=noise)
    hcl = HX.Classifier(input_shape=[None, None, 128])
    hxv.load_state_dict({k[len("embedding_model."):]: v for k, v in holder.state_dict().items()
                         if k.startswith("embedding_model.")})
    hcl.load_state_dict({k[len("classifier."):]: v for k, v in holder.state_dict().items()
                         if k.startswith("classifier.")})
    hxv.to(DEV).train()
    hcl.to(DEV).train()
    return oxv, ocl, hxv, hcl


def _hip_step(hxv, hcl, feats, lens, label):
    from speech_anonymization_amd import xvector as HX
    for p in list(hxv.parameters()) + list(hcl.parameters()):
        p.grad = None
    logp = HX.train_log_probs(hxv, hcl, feats.to(DEV), None if lens is None else lens.to(DEV))
    loss = F.nll_loss(logp.squeeze(1), label.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return logp, loss


@pytest.mark.parametrize("B,T,lens", [(4, 200, [1.0, 0.8, 0.55, 0.3]), (2, 1008, None)], ids=["B4T200", "B2T1008"])
def test_train_step_matches_oracle(B, T, lens):
    """log-probs, loss, all 30 parameter gradients and the 7 BatchNorms' running statistics after
    one train-mode step, against the float64 oracle (rel-MSE <= 1e-4 each)."""
    oxv, ocl, hxv, hcl = _models(B)
    g = torch.Generator().manual_seed(7 + T)
    feats = torch.randn(B, T, 80, generator=g)
    label = torch.arange(B) % 2
    lens_t = None if lens is None else torch.tensor(lens)
    ologp = ocl(oxv(feats.double(), lens_t))
    oloss = F.nll_loss(ologp.squeeze(1), label)
    oloss.backward()
    logp, loss = _hip_step(hxv, hcl, feats, lens_t, label)
    errs = {"logp": rel_mse(logp, ologp), "loss": rel_mse(loss, oloss)}
    hp = dict(list((f"xv.{k}", v) for k, v in hxv.named_parameters()) +
              list((f"cl.{k}", v) for k, v in hcl.named_parameters()))
    op = dict(list((f"xv.{k}", v) for k, v in oxv.named_parameters()) +
              list((f"cl.{k}", v) for k, v in ocl.named_parameters()))
    assert len(hp) == 30 and hp.keys() == op.keys()
    for k in op:
        assert hp[k].grad is not None, k
        errs["grad " + k] = rel_mse(hp[k].grad, op[k].grad)
    hb = dict(list((f"xv.{k}", v) for k, v in hxv.named_buffers()) + list((f"cl.{k}", v) for k, v in hcl.named_buffers()))
    ob = dict(list((f"xv.{k}", v) for k, v in oxv.named_buffers()) + list((f"cl.{k}", v) for k, v in ocl.named_buffers()))
    nrun = 0
    for k in ob:
        if k.endswith("running_mean") or k.endswith("running_var"):
            errs[k] = rel_mse(hb[k], ob[k])
            nrun += 1
        elif k.endswith("num_batches_tracked"):
            assert int(hb[k]) == int(ob[k]) == 1, k
    assert nrun == 14
    worst = max(errs, key=errs.get)
    print(f"\nB={B} T={T}: worst rel-MSE {errs[worst]:.3e} ({worst}); logp {errs['logp']:.3e}, loss {errs['loss']:.3e}")
    for k, v in errs.items():
        assert v <= 1e-4, (k, v)


@pytest.mark.parametrize("cfg,T", [(c, 150) for c in SHAPES] + [(c, 126) for c in SHAPES],
                         ids=IDS + [i + "-T126" for i in IDS])
def test_tdnn_train_kernels(cfg, T):
    """one TDNN block in train mode, T not a multiple of the 128-frame tile: sa_xv_tdnn_fwd_train
    (z and the batch statistics), the BatchNorm/LeakyReLU backward (dpre, d gamma, d beta, d bias),
    sa_xv_tdnn_wgrad (d W) and sa_xv_tdnn_dgrad + sa_tdnn_fold (d x, reflected ends included)
    against fp64 autograd; rel-MSE <= 1e-8 each.  T = 126: the data gradient's extended range
    T + 2*pad takes two row tiles, the forward one."""
    from oracle import xvector as OX
    from speech_anonymization_amd import xvector as HX
    cin, cout, k, d = cfg
    B = 2
    g = torch.Generator().manual_seed(cin + cout + k + d)
    oc, ob = OX.Conv1d(cin, cout, k, d).double(), OX.BatchNorm1d(cout).double()
    with torch.no_grad():
        ob.norm.weight.uniform_(0.8, 1.2, generator=g)
        ob.norm.bias.normal_(0, 0.1, generator=g)
    x = torch.randn(B, T, cin, generator=g, dtype=torch.float64)
    s_in = t_in = None
    if cin != 80:                                   # the previous block's BatchNorm affine at staging
        s_in = torch.rand(cin, generator=g, dtype=torch.float64) + 0.5
        t_in = 0.1 * torch.randn(cin, generator=g, dtype=torch.float64)
    gy = torch.randn(B, T, cout, generator=g, dtype=torch.float64)
    hc, hb = HX._Conv(cin, cout, k, d), HX._BN(cout)
    hc.load_state_dict({kk: v.float() for kk, v in oc.state_dict().items()})
    hb.load_state_dict({kk: v.float() if v.is_floating_point() else v for kk, v in ob.state_dict().items()})
    hc.to(DEV)
    hb.to(DEV)
    xd = x.float().to(DEV)
    sd = None if s_in is None else s_in.float().to(DEV)
    td = None if t_in is None else t_in.float().to(DEV)
    z, sums = HX._tdnn_train(xd, sd, td, hc)
    f = HX._bn_train_stats(sums, hb.norm, B * T)

    # fp64 reference; the LeakyReLU branch of the backward follows the sign of the kernel's z (a
    # pre-activation within rounding of 0 may fall on either side, and its gradient then differs by
    # the factor 1/slope -- the same reason sa_tdnn_bwd_input takes the forward's branch mask)
    xr = (x * s_in + t_in if s_in is not None else x.clone()).requires_grad_(True)
    pre = oc(xr)
    branch = torch.where(z.double().cpu() > 0, 1.0, 0.01)
    zr = pre * branch
    yr = ob(zr)
    yr.backward(gy)
    zref = F.leaky_relu(pre.detach(), 0.01)
    mref = zref.mean(dim=(0, 1))
    vref = zref.var(dim=(0, 1), unbiased=False)
    errs = {"z": rel_mse(z, zref), "mean": rel_mse(f[0], mref),
            "rstd": rel_mse(f[1], 1.0 / torch.sqrt(vref + 1e-5)),
            "running_var": rel_mse(hb.norm.running_var, ob.norm.running_var),
            # the batch part of the update alone, against the unbiased n/(n-1) variance (n = B*T)
            "running_var batch part": rel_mse((hb.norm.running_var.double().cpu() - 0.9) / 0.1,
                                              zref.var(dim=(0, 1), unbiased=True)),
            "running_mean": rel_mse(hb.norm.running_mean.double().cpu() / 0.1, mref)}
    M = B * T
    dg, dbe, dbias = (torch.empty(cout, device=DEV) for _ in range(3))
    dpre = torch.empty_like(z)
    bsum = HX._bn_leaky_bwd(gy.float().to(DEV).view(M, -1), z.view(M, -1), hb.norm, f, M, dg, dbe, dpre.view(M, -1))
    HX._fin_bias(bsum, dbias)
    dW = torch.empty_like(hc.conv.weight)
    HX._tdnn_wgrad(dpre, xd, sd, td, hc, dW)
    dx = HX._tdnn_dgrad(dpre, hc)
    torch.cuda.synchronize()
    errs.update({"d gamma": rel_mse(dg, ob.norm.weight.grad), "d beta": rel_mse(dbe, ob.norm.bias.grad),
                 "d bias": rel_mse(dbias, oc.conv.bias.grad), "d W": rel_mse(dW, oc.conv.weight.grad),
                 "d x": rel_mse(dx, xr.grad)})
    pad = d * (k - 1) // 2
    if pad:
        errs["d x ends"] = rel_mse(torch.cat([dx[:, :2 * pad + 1], dx[:, -2 * pad - 1:]], 1),
                                   torch.cat([xr.grad[:, :2 * pad + 1], xr.grad[:, -2 * pad - 1:]], 1))
    print(f"\n{cfg} T={T}: " + ", ".join(f"{kk} {v:.2e}" for kk, v in errs.items()))
    for kk, v in errs.items():
        assert v <= 1e-8, (kk, v)


def test_train_step_is_bit_reproducible():
    """the same step twice from the same state: identical gradients and running statistics."""
    B, T = 8, 300
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(B, T, 80, generator=g)
    lens = torch.linspace(1.0, 0.5, B)
    label = torch.arange(B) % 2
    out = []
    for _ in range(2):
        _, _, hxv, hcl = _models(B, seed=99)
        logp, loss = _hip_step(hxv, hcl, feats, lens, label)
        st = [p.grad.clone() for p in list(hxv.parameters()) + list(hcl.parameters())]
        st += [b.clone() for b in list(hxv.buffers()) + list(hcl.buffers())]
        out.append([logp.detach().clone(), loss.detach().clone()] + st)
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_eval_after_fused_adam_step_sees_the_new_weights():
    """torch's fused Adam does not bump the parameters' version counters: after a train step and an
    optimizer step, the eval-mode forward must still use the updated weights (it equals a fresh
    classifier loaded with the same state)."""
    from speech_anonymization_amd import xvector as HX
    B, T = 4, 120
    _, _, hxv, hcl = _models(B)
    hxv.pooling_noise = hcl_noise = None
    enc = HX.EncoderClassifier(hxv, hcl)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(B, T, 80, generator=g).to(DEV)
    enc.eval()
    before = enc.classify_batch_feats(feats)[0].clone()       # fills the operand-image cache
    enc.train()
    opt = torch.optim.Adam(list(hxv.parameters()) + list(hcl.parameters()), lr=1e-2, fused=True)
    _hip_step(hxv, hcl, feats.cpu(), None, torch.arange(B) % 2)
    opt.step()
    enc.eval()
    after = enc.classify_batch_feats(feats)[0]
    fresh = HX.EncoderClassifier(HX.Xvector(pooling_noise=hcl_noise), HX.Classifier(input_shape=[None, None, 128]))
    fresh.load_state_dict(enc.state_dict())
    want = fresh.to(DEV).eval().classify_batch_feats(feats)[0]
    assert not torch.equal(after, before)
    assert torch.equal(after, want)


def test_train_path_needs_both_modules_in_the_same_mode():
    from speech_anonymization_amd import xvector as HX
    _, _, hxv, hcl = _models(4)
    hcl.eval()
    with pytest.raises(ValueError):
        HX.train_log_probs(hxv, hcl, torch.randn(4, 100, 80, device=DEV))


def test_pool_affine_against_the_formula():
    """sa_xv_pool_affine / _bwd directly: the pooling-noise offset eps*((1-9)*g + 9) on the mean, the
    std scaled by |s|, and the sign of s on the std half of the backward (negative s included)."""
    import ctypes as C
    from speech_anonymization_amd import _lib as L
    lib = L.load()
    B, Cc, eps = 3, 1500, 1e-5
    g = torch.Generator().manual_seed(11)
    pz = torch.randn(B, 2 * Cc, generator=g, dtype=torch.float64)
    pz[:, Cc:] = pz[:, Cc:].abs() + eps
    s = torch.randn(Cc, generator=g, dtype=torch.float64)
    t = torch.randn(Cc, generator=g, dtype=torch.float64)
    noise = torch.rand(B, Cc, generator=g, dtype=torch.float64)
    dev = lambda a: a.float().to(DEV).contiguous()
    pzd, sd, td, nd = dev(pz), dev(s), dev(t), dev(noise)
    for use_noise in (True, False):
        out = torch.empty(B, 2 * Cc, device=DEV)
        L.check(lib.sa_xv_pool_affine(L.ptr(pzd), L.ptr(sd), L.ptr(td), L.ptr(nd) if use_noise else None, B, Cc,
                                      C.c_float(eps), L.ptr(out), L.stream()), "sa_xv_pool_affine")
        torch.cuda.synchronize()
        pz32, s32, t32 = pzd.double().cpu(), sd.double().cpu(), td.double().cpu()
        mean = s32 * pz32[:, :Cc] + t32
        if use_noise:
            mean = mean + eps * ((1 - 9) * nd.double().cpu() + 9)
        std = s32.abs() * (pz32[:, Cc:] - eps) + eps
        got = out.double().cpu()
        assert (got[:, :Cc] - mean).abs().max() <= 1e-6 * (1 + mean.abs().max())   # offset >= 1e-5
        assert (got[:, Cc:] - std).abs().max() <= 1e-6 * (1 + std.abs().max())
    gp = dev(torch.randn(B, 2 * Cc, generator=g))
    gz = torch.empty_like(gp)
    L.check(lib.sa_xv_pool_affine_bwd(L.ptr(gp), L.ptr(sd), B, Cc, L.ptr(gz), L.stream()), "sa_xv_pool_affine_bwd")
    torch.cuda.synchronize()
    assert torch.equal(gz[:, :Cc], gp[:, :Cc])
    assert torch.equal(gz[:, Cc:], torch.where(sd < 0, -gp[:, Cc:], gp[:, Cc:]))
    assert bool((sd < 0).any())


def test_batch_of_one_raises():
    from speech_anonymization_amd import xvector as HX
    _, _, hxv, hcl = _models(1)
    with pytest.raises(ValueError):
        HX.train_log_probs(hxv, hcl, torch.randn(1, 100, 80, device=DEV))


def test_recipe_end_to_end(tmp_path):
    """gender_classifier_train.py --synthetic: trains on harmonic series at two fundamentals plus
    noise (data.synthetic_gender_dataset) within a minute of wall time (process start included) and
    reaches a test error <= 0.1 on held-out utterances.  The task is easy on purpose: the CPU oracle
    (oracle.xvector + oracle.features, torch autograd, Adam, clipping and the same ReduceLROnPlateau)
    trained on the same data, seed and budget (4 epochs of 96 utterances, batch 16) reaches test error
    0.0 from its first epoch, so the bar has a wide margin.  The best checkpoint then goes through
    speechbrain_convae_train.py's own `--external_classifier_ckpt` path (strict keys), and the VALID
    stage of that run logs ACC_external and ACC_external_orig."""
    import json
    import time
    out = tmp_path / "gender"
    cmd = [sys.executable, os.path.join(ROOT, "gender_classifier_train.py"),
           os.path.join(ROOT, "speechbrain_configs", "gender_classifier.yaml"), "--device", DEV,
           "--output_folder", str(out), "--synthetic", "96", "--number_of_epochs", "4", "--batch_size", "16"]
    t0 = time.monotonic()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    wall = time.monotonic() - t0
    print(r.stdout[-3000:], r.stderr[-3000:], f"\nrecipe wall time {wall:.1f} s")
    assert r.returncode == 0
    assert wall <= 60.0, wall
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["test_error"] <= 0.1, res
    ck = res["best_checkpoint"]
    for f in ("embedding_model.ckpt", "classifier.ckpt", "normalizer.ckpt", "counter.ckpt", "optimizer.ckpt",
              "CKPT.yaml", "label_encoder.txt"):
        assert os.path.exists(os.path.join(ck, f)), f

    folder = tmp_path / "convae"
    cmd = [sys.executable, os.path.join(ROOT, "speechbrain_convae_train.py"),
           os.path.join(ROOT, "speechbrain_configs", "convae.yaml"), "--device", DEV, "--folder", str(folder),
           "--synthetic", "8", "--batch_size", "4", "--number_of_epochs", "1", "--external_classifier_ckpt", ck]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    logs = [os.path.join(d, f) for d, _, fs in os.walk(folder) for f in fs if f == "train_log.txt"]
    assert len(logs) == 1
    line = open(logs[0]).read().splitlines()[-1]
    print(line)
    assert "valid ACC_external:" in line and "valid ACC_external_orig:" in line
