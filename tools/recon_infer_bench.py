#!/usr/bin/env python3
"""Times the inference path of gender_classifier_train_recon.py at B = 32, T = 1008 on one GPU.

Per model (fcae, convae, endtoend): the median of --steps calls of ``model.reconstruct(feats)`` against the
median of ``model.eval()(feats)`` under no_grad -- the only inference there was before reconstruct -- and the
launches of each, counted as the device kernels torch.profiler sees in one call.  Then the recipe's whole training
step (Fbank -> global normaliser -> reconstruct -> x-vector forward, NLL, backward, clip, Adam, as
GenderReconBrain.fit_batch runs it) for fcae and convae in ms and frames/s.  Device events around each call after
a warm-up.  Prints one JSON line."""
import argparse
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from tools.bench_common import time_calls  # noqa: E402


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception:                                            # no profiler in this build: the count is optional
        return None


def build(kind):
    from speech_anonymization_amd import convae, endtoend, fcae
    torch.manual_seed(0)
    if kind == "fcae":
        return fcae.FullyConnectedAutoencoder(80, 32, pooling_noise=False)
    if kind == "convae":
        return convae.ConvAutoencoder(pooling_noise=None)
    return endtoend.ConvReconstruction()


def recipe_step(kind, dev, B, n_samples, warmup, steps):
    from speech_anonymization_amd import features, gender, losses, xvector
    from speech_anonymization_amd.brain import Batch
    torch.manual_seed(0)
    emb, cl = xvector.Xvector(), xvector.Classifier(input_shape=[None, None, 128])
    modules = {"compute_features": features.Fbank(16000, 400, 80), "mean_var_norm": features.InputNormalization(),
               "embedding_model": emb, "classifier": cl, "model": build(kind)}
    for p in modules["model"].parameters():
        p.requires_grad = False
    brain = gender.GenderReconBrain(modules=modules, opt_class=functools.partial(torch.optim.Adam, lr=1e-3),
                                    hparams={"compute_cost": losses.NLLLoss(), "recon_normalizer": "own"},
                                    run_opts={"device": str(dev), "max_grad_norm": 5.0})
    brain.on_fit_start()
    brain.modules.train()
    wavs = 0.1 * torch.randn(B, n_samples)
    batch = Batch(wavs, torch.ones(B), torch.arange(B) % 2).to(dev)
    T = int(brain.prepare_features(batch.sig[0], batch.sig[1], None).shape[1])
    step = lambda: brain.fit_batch(batch)
    ms = time_calls(step, warmup, steps)
    return {"ms_per_step": round(ms, 4), "launches_per_step": launches(step), "frames": B * T,
            "frames_per_s": round(B * T / ms * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1008)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    from oracle.features import synthetic_feats
    feats = synthetic_feats(a.B, a.T, seed=1).to(dev)
    out = {"B": a.B, "T": a.T, "steps": a.steps}
    for kind in ("fcae", "convae", "endtoend"):
        m = build(kind).to(dev).eval()

        def fwd():
            with torch.no_grad():
                return m(feats)[0]
        rec = lambda: m.reconstruct(feats)
        assert torch.equal(rec(), fwd()), kind
        t_fwd, t_rec = time_calls(fwd, a.warmup, a.steps), time_calls(rec, a.warmup, a.steps)
        out[kind] = {"reconstruct_ms": round(t_rec, 4), "reconstruct_launches": launches(rec),
                     "eval_forward_ms": round(t_fwd, 4), "eval_forward_launches": launches(fwd),
                     "eval_forward_over_reconstruct": round(t_fwd / t_rec, 3),
                     "reconstruct_frames_per_s": round(a.B * a.T / t_rec * 1e3, 1)}
        del m
    n_samples = (a.T - 1) * 160                                  # Fbank: hop 160, centred -> T frames
    for kind in ("fcae", "convae"):
        out["recipe_step_" + kind] = recipe_step(kind, dev, a.B, n_samples, a.warmup, a.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
